"""csrc/batch.hip where its loops take another trip: imt_select_plan past one chunk of 16384 positions (the running base, the
clamped re-reads of position n - 1, a partly live last chunk) and imt_mass_mask / imt_mass_unmask at spans longer than a
workgroup (every ``+= 256`` loop wraps) and at spans CLIPPED by the row's end (``last = min(first + len, width)``), which
training reaches whenever mask_prob is drawn high.  Everything is integer: results are bit-exact against CPU boolean
indexing and against the loop-form oracle (oracle/batch_oracle.py) on the same counter-based draws.  Outputs go through
the C ABI into sentinel-filled buffers (tests/test_gpu_row_edges.py: Guarded); DESIGN.md, "Batch and object-stream edge
tests", lists case -> path reached."""
import ctypes
import functools

import pytest
import torch

from oracle import batch_oracle as BO
from oracle.reference_model import SyntheticTextProcessor
from tests.test_gpu_batch import _batch
from tests.test_gpu_row_edges import SENT, Guarded, _bits_equal

pytestmark = pytest.mark.gpu

CHUNK = 1024 * 16   # positions per trip of select_plan_kernel (1024 threads x SEL_ITEMS)


def _ops():
    from imagetranslate_amd import hip_ops as O
    from imagetranslate_amd import _lib as L
    return O, L, L.load()


# ------------------------------------------------------------------------------------------------ imt_select_plan
def _rand(B, T, seed, p=0.5):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, T, generator=g) < p, torch.randint(0, 30000, (B, T), generator=g)


def _flat_to_cell(p, T1, col0):
    return p // T1, col0 + p % T1


def _mask_case(name):
    """(mask [B, T] bool, ids [B, T], col0) of one named case."""
    if name in ("one-chunk", "second-trip-one-live", "three-trips"):
        B, T = {"one-chunk": (128, 129), "second-trip-one-live": (5, 3278), "three-trips": (3, 13335)}[name]
        mask, ids = _rand(B, T, B + T)
        return mask, ids, 1
    if name == "col0-0":
        mask, ids = _rand(5, 3278, 11)
        return mask, ids, 0
    if name == "col0-2":
        mask, ids = _rand(5, 3280, 12)
        return mask, ids, 2
    mask, ids = _rand(5, 3278, 13)
    if name == "all-ones":
        mask[:] = True
    elif name == "all-zero":
        mask[:] = False
    elif name == "last-set":
        mask[-1, -1] = True
    elif name == "last-clear":
        mask[-1, -1] = False
    else:
        raise KeyError(name)
    return mask, ids, 1


SELECT_CASES = {"one-chunk": CHUNK, "second-trip-one-live": CHUNK + 1, "three-trips": 40002, "all-ones": CHUNK + 1,
                "all-zero": CHUNK + 1, "last-set": CHUNK + 1, "last-clear": CHUNK + 1, "col0-0": 16390, "col0-2": 16390}


def _run_select(mask_dev, ids_dev, col0):
    """imt_select_plan into sentinel-filled idx / targets of n + 4 entries and a guarded count; returns (idx, targets, count)."""
    O, L, lib = _ops()
    B, T = ids_dev.shape
    n = B * (T - col0)
    dev = ids_dev.device
    idx, tg, cnt = Guarded(n, None, torch.int32, dev), Guarded(n, None, torch.int64, dev), Guarded(1, None, torch.int32, dev)
    L.check(lib.imt_select_plan(O._p(mask_dev), mask_dev.stride(0), O._p(ids_dev), ids_dev.stride(0), B, T - col0, col0, O._p(idx.view),
                                O._p(tg.view), O._p(cnt.view), O._stream()), "imt_select_plan")
    cnt.check("select_plan count")
    return idx.full.cpu(), tg.full.cpu(), int(cnt.view.cpu())


def _check_select(mask, ids, col0, got, what):
    idx, tg, k = got
    sel = mask[:, col0:]
    exp_idx = torch.nonzero(sel.reshape(-1)).view(-1)
    exp_tg = ids[:, col0:][sel]
    assert k == exp_idx.numel(), "%s: count %d, boolean indexing selects %d" % (what, k, exp_idx.numel())
    assert torch.equal(idx[:k].long(), exp_idx), what + ": idx"
    assert torch.equal(tg[:k], exp_tg), what + ": targets"
    # everything from the count onward -- the unused part of the n entries and the 4 behind them -- is untouched
    assert bool((idx[k:] == int(SENT)).all()) and bool((tg[k:] == int(SENT)).all()), what + ": wrote at or past the count"


@pytest.mark.parametrize("name", list(SELECT_CASES))
def test_select_plan_chunks(cuda, name):
    mask, ids, col0 = _mask_case(name)
    B, T = ids.shape
    n = B * (T - col0)
    assert n == SELECT_CASES[name]   # the trip count the case is named for: cdiv(n, 16384)
    got = _run_select(mask.to(torch.uint8).to(cuda), ids.to(cuda), col0)
    _check_select(mask, ids, col0, got, "select_plan " + name)
    if name == "all-ones":
        assert torch.equal(got[0][:n].long(), torch.arange(n))
    if name == "all-zero":
        assert got[2] == 0


def test_select_plan_last_position_counts_once(cuda):
    """n = 16385: in the second trip thread 0 owns position n - 1 and every other read is clamped to it.  With the last flag
    set the count grows by exactly one over the same mask with it clear."""
    counts = {}
    for name in ("last-set", "last-clear"):
        mask, ids, col0 = _mask_case(name)
        counts[name] = _run_select(mask.to(torch.uint8).to(cuda), ids.to(cuda), col0)[2]
    assert counts["last-set"] == counts["last-clear"] + 1


def test_select_plan_one_wave_of_the_second_chunk(cuda):
    """The only set flags lie in the 1024 positions owned by wave 5 of the second chunk: waves 0..4 contribute zero totals,
    s_base enters the chunk as 0, and the offsets inside the wave come from the shuffle scan alone."""
    B, T, col0 = 3, 13335, 1
    T1 = T - col0
    _, ids = _rand(B, T, 21)
    mask = torch.zeros(B, T, dtype=torch.bool)
    lo = CHUNK + 5 * 64 * 16
    g = torch.Generator().manual_seed(22)
    for p in (lo + torch.randperm(1024, generator=g)[:300]).tolist() + [lo, lo + 1023]:
        b, c = _flat_to_cell(p, T1, col0)
        mask[b, c] = True
    got = _run_select(mask.to(torch.uint8).to(cuda), ids.to(cuda), col0)
    _check_select(mask, ids, col0, got, "select_plan one wave")
    assert int(got[0][:got[2]].min()) == lo and int(got[0][:got[2]].max()) == lo + 1023


def test_select_plan_strided_views(cuda):
    """ld_mask != T and ld_ids != T: both operands are column slices of wider buffers whose other columns hold set flags and
    other ids."""
    B, T, col0 = 5, 3278, 1
    mask, ids = _rand(B, T, 31)
    g = torch.Generator().manual_seed(32)
    wide_mask = torch.ones(B, T + 5, dtype=torch.uint8)
    wide_ids = torch.randint(30000, 60000, (B, T + 3), generator=g)
    wide_mask[:, :T] = mask.to(torch.uint8)
    wide_ids[:, :T] = ids
    md, idd = wide_mask.to(cuda)[:, :T], wide_ids.to(cuda)[:, :T]
    assert md.stride(0) == T + 5 and idd.stride(0) == T + 3
    _check_select(mask, ids, col0, _run_select(md, idd, col0), "select_plan strided")


def test_select_plan_count_hint(cuda, monkeypatch):
    """count=: the wrapper trusts the host's number and reads nothing back; the selection is the same."""
    O, L, _ = _ops()
    monkeypatch.delenv("IMT_CHECK_COUNT", raising=False)
    mask, ids, col0 = _mask_case("three-trips")
    k = int(mask[:, col0:].sum())
    idx, tg = O.select_plan(mask.to(cuda), ids.to(cuda), col0=col0, count=k)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (k,) and tuple(tg.shape) == (k,)
    assert torch.equal(idx.cpu().long(), torch.nonzero(mask[:, col0:].reshape(-1)).view(-1))
    assert torch.equal(tg.cpu(), ids[:, col0:][mask[:, col0:]])
    idx2, tg2 = O.select_plan(mask.to(cuda), ids.to(cuda), col0=col0)
    assert _bits_equal(idx2, idx) and _bits_equal(tg2, tg)
    monkeypatch.setenv("IMT_CHECK_COUNT", "1")
    with pytest.raises(L.ImtError):
        O.select_plan(mask.to(cuda), ids.to(cuda), col0=col0, count=k + 1)


# ------------------------------------------------------------------------------------------------ imt_mass_mask / imt_mass_unmask
VOCAB = 500
# name -> (rows, width, seed, mask_prob)
MASS_CASES = {"wrap": (40, 600, 6, 0.3), "wrap-clipped": (40, 600, 6, 0.9), "clipped": (64, 64, 5, 0.9), "short-pads": (12, 24, 8, 0.3)}


def _mass_batch(name):
    n_rows, width, seed, _ = MASS_CASES[name]
    text, pad_idx = _batch(n_rows, width, seed, VOCAB)
    if name == "short-pads":   # pad indices 1, 2, 3 beside full rows: spans of 0 and 1 tokens
        for r, p in enumerate((1, 2, 3, 1, 2, 3, 1, 2)):
            pad_idx[r] = p
            text[r, p:] = 0
    return text, pad_idx


@functools.lru_cache(maxsize=None)
def _mass_case(name):
    """Batch, oracle outputs and the oracle's span starts of one case; shared and never modified."""
    n_rows, width, seed, p = MASS_CASES[name]
    tp = SyntheticTextProcessor(VOCAB)
    text, pad_idx = _mass_batch(name)
    draw_start = lambda r: (BO.counter_uniform(seed, 0, r), BO.counter_uniform(seed, 1, r))  # noqa: E731
    draw_token = lambda r, c: (BO.counter_uniform(seed, 2, r * width + c), BO.counter_uniform(seed, 3, r * width + c))  # noqa: E731
    exp = BO.mass_mask_reference(p, pad_idx, text, len(tp.special_tokens), VOCAB, tp.mask_token_id(), tp.pad_token_id(), draw_start,
                                 draw_token)
    first = torch.tensor([BO.span_start(p, int(pad_idx[r]), *draw_start(r)) for r in range(n_rows)])
    return dict(text=text, pad_idx=pad_idx, exp=exp, first=first, tp=tp)


def check_mass_case(name):
    """Oracle only, no device call: the clipped cases clip, the wrapping cases wrap, the short rows take the first = 2 branch.
    Run before every device call below, and without a GPU by tests/test_mass_span_starts.py."""
    n_rows, width, seed, p = MASS_CASES[name]
    c = _mass_case(name)
    span = c["pad_idx"] // 2
    clipped = int((c["first"] + span > width).sum())
    longest = int((torch.clamp(c["first"] + span, max=width) - c["first"]).max())
    print("MASSEDGE %s clipped rows %d, longest hidden span %d, targets %d of sum(pad // 2) = %d"
          % (name, clipped, longest, c["exp"]["targets"].numel(), int(span.sum())))
    assert (clipped >= 1) == ("clipped" in name)
    assert (longest > 256) == ("wrap" in name)
    if name == "short-pads":
        short = c["pad_idx"] <= 3
        assert set(span[short].tolist()) == {0, 1} and bool((c["first"][short] == 2).any()) and bool((c["first"][short] == 1).any())
        assert bool((c["pad_idx"] >= 1).all())
    if "clipped" in name:
        assert c["exp"]["targets"].numel() < int(span.sum())


@pytest.mark.parametrize("name", list(MASS_CASES))
def test_mass_mask_through_the_abi(cuda, name):
    """imt_mass_mask into guarded buffers sized as mass_mask_device sizes them; then imt_mass_unmask."""
    O, L, lib = _ops()
    from imagetranslate_amd.utils import mass_span_sizes, mass_span_starts
    n_rows, width, seed, p = MASS_CASES[name]
    check_mass_case(name)
    c = _mass_case(name)
    exp, tp = c["exp"], c["tp"]
    first = mass_span_starts(p, c["pad_idx"], seed)
    assert torch.equal(first, c["first"]), "host span starts differ from the oracle's"
    first, hidden = mass_span_sizes(first, c["pad_idx"], width)
    assert torch.equal(first, c["first"]), "no start of these cases needs the clamp"
    offsets = torch.cumsum(hidden, 0) - hidden
    total, rw = int(hidden.sum()), int(hidden.max()) + 1
    assert total == exp["targets"].numel() and rw == exp["to_recover"].shape[1]
    assert n_rows * width % 2 == 0
    mask_buf = Guarded(n_rows * width // 2, None, torch.int16, cuda)   # the byte mask in a 16-bit buffer: the sentinel needs 16 bits
    rec, pos = Guarded(n_rows, rw, torch.int64, cuda, ld=rw), Guarded(n_rows, rw, torch.int64, cuda, ld=rw)
    tg = Guarded(total, None, torch.int64, cuda)
    text = Guarded(n_rows, width, torch.int64, cuda, ld=width)
    text.view.copy_(c["text"])
    pad_dev, off_dev, first_dev = c["pad_idx"].to(cuda), offsets.to(cuda), first.to(cuda)
    a = L.MassArgs()
    a.n_rows, a.width, a.recover_width = n_rows, width, rw
    a.n_special, a.vocab = len(tp.special_tokens), VOCAB
    a.mask_prob, a.seed = p, seed
    a.mask_id, a.pad_id = tp.mask_token_id(), tp.pad_token_id()
    a.src_text, a.pad_indices, a.row_offsets, a.first = text.view.data_ptr(), pad_dev.data_ptr(), off_dev.data_ptr(), first_dev.data_ptr()
    a.src_mask, a.to_recover, a.positions, a.targets = mask_buf.view.data_ptr(), rec.view.data_ptr(), pos.view.data_ptr(), tg.view.data_ptr()
    L.check(lib.imt_mass_mask(ctypes.byref(a), O._stream()), "imt_mass_mask")
    for b, what in ((mask_buf, "src_mask"), (rec, "to_recover"), (pos, "positions"), (tg, "targets"), (text, "src_text")):
        b.check("mass_mask %s %s" % (name, what))
    mask = mask_buf.view.view(torch.uint8).view(n_rows, width)
    assert torch.equal(mask.cpu().bool(), exp["src_mask"]) and int(mask.max()) <= 1
    assert torch.equal(rec.view.cpu(), exp["to_recover"]), "to_recover"
    assert torch.equal(pos.view.cpu(), exp["positions"]), "positions"
    assert torch.equal(tg.view.cpu(), exp["targets"]) and torch.equal(tg.view.cpu(), exp["mask_idx"]), "targets"
    assert torch.equal(text.view.cpu(), exp["src_text"]), "src_text"
    L.check(lib.imt_mass_unmask(O._p(text.view), O._p(mask), O._p(tg.view), O._p(off_dev), n_rows, width, O._stream()), "imt_mass_unmask")
    text.check("mass_unmask %s" % name)
    assert torch.equal(text.view.cpu(), c["text"]), "unmask restores the batch"


@pytest.mark.parametrize("name", list(MASS_CASES))
def test_mass_mask_device_shapes_and_values(cuda, name):
    """The wrapper: all six outputs equal the oracle's, SHAPES INCLUDED (torch.equal), and the round trip restores the batch."""
    from imagetranslate_amd.utils import mass_mask_device, mass_unmask_device
    n_rows, width, seed, p = MASS_CASES[name]
    check_mass_case(name)
    c = _mass_case(name)
    dev_text = c["text"].clone().to(cuda)
    got = mass_mask_device(p, c["pad_idx"], dev_text, c["tp"], seed)
    for k in ("src_mask", "targets", "src_text", "to_recover", "positions", "mask_idx"):
        assert tuple(got[k].shape) == tuple(c["exp"][k].shape), "%s: shape %s, the oracle's %s" % (k, tuple(got[k].shape), tuple(c["exp"][k].shape))
        assert torch.equal(got[k].cpu(), c["exp"][k]), k
    assert got["src_text"].data_ptr() == dev_text.data_ptr(), "masked in place like the reference"
    mass_unmask_device(got)
    assert torch.equal(dev_text.cpu(), c["text"]), "unmask restores the batch"


@pytest.mark.parametrize("mask_prob", [0.15, 0.3, 0.5, 0.9, 1 - 1e-6])
def test_device_spans_start_where_the_host_says(cuda, mask_prob):
    """The grid of tests/test_mass_span_starts.py on the device: in every row with a non-empty span the first set bit of the
    mask is the host's span start and the span has the clipped length.  The kernel is HANDED the host's starts, so this checks
    that it honours its argument and the clip over 10 000 rows, not that two draws agree: that the host's draw is the
    generator's is the CPU test's comparison with the oracle."""
    from imagetranslate_amd.utils import mass_mask_device, mass_span_sizes, mass_span_starts
    n_rows, width, seed = 10000, 601, (0x5EED << 32) | 0x1234ABCD
    g = torch.Generator().manual_seed(17)
    pad = torch.randint(1, 601, (n_rows,), generator=g)
    pad[:600] = torch.arange(1, 601)
    text = torch.randint(7, VOCAB, (n_rows, width), generator=g)
    text[torch.arange(width)[None] >= pad[:, None]] = 0
    got = mass_mask_device(mask_prob, pad, text.to(cuda), SyntheticTextProcessor(VOCAB), seed)
    mask = got["src_mask"].cpu()
    first, hidden = mass_span_sizes(mass_span_starts(mask_prob, pad, seed), pad, width)
    assert torch.equal(mask.sum(1), hidden)
    live = hidden > 0
    assert int(live.sum()) > 9000
    assert torch.equal(mask.to(torch.int8).argmax(1)[live], first[live])
    assert int(got["targets"].numel()) == int(hidden.sum())
