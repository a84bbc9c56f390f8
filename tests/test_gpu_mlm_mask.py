"""imt_mlm_mask (csrc/batch.hip) against its restatement (tests/lm_oracle.mlm_mask), bit for bit: the mask, the ids after the
replacement, the compacted positions and originals, and the count -- at one position, a partly filled chunk, one position short
of, exactly at and one past the 1024 x 16 positions one trip of the kernel's loop covers, and over two chunk boundaries with a
row across each; ragged pads with an empty and a full row, holes inside a row, both settings of mask_eos."""
import pytest
import torch

from oracle import reference_model as R
from tests import lm_oracle as M

pytestmark = pytest.mark.gpu

V = 1000
# (1, 1) one position; (3, 7) / (8, 32) a partly filled chunk; 129 x 127 = 16383 and 128 x 128 = 16384: one short of and exactly
# one chunk; (1, 16385) one past it; 5 x 6554 = 32770: two chunk boundaries (16384, 32768), rows 2 and 5 lying across them
SHAPES = [(1, 1), (3, 7), (8, 32), (129, 127), (128, 128), (1, 16385), (5, 6554)]


def _batch(B, S, seed, holes=False):
    """Ragged rows ending in </s>: row 0 full, row 1 (if any) empty, the others of random length; ``holes``: pads inside rows."""
    g = torch.Generator().manual_seed(seed)
    texts = torch.randint(7, V, (B, S), generator=g)
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0] = S
    if B > 1:
        lens[1] = 0
    pads = torch.arange(S)[None] < lens[:, None]
    eos = torch.rand(B, S, generator=g) < 0.1   # </s> inside the rows too: with mask_eos off every one of them tells
    texts[eos] = 4
    if holes:
        pads &= torch.rand(B, S, generator=g) < 0.7
    return texts, pads


def _run(texts, pads, tp, p, seed, mask_eos=True, count=None):
    from imagetranslate_amd.utils import mask_text_device
    dev_texts = texts.cuda().contiguous()
    out = mask_text_device(p, pads.cuda(), dev_texts, tp, seed, mask_eos=mask_eos, count=count)
    torch.cuda.synchronize()
    assert out["texts"] is dev_texts
    return out


def _check(out, want, what):
    assert out["mask"].dtype == torch.bool and out["idx"].dtype == torch.int32 and out["targets"].dtype == torch.int64
    assert int(out["count"].item()) == want["count"], what
    assert torch.equal(out["mask"].cpu(), want["mask"]), what + ": mask"
    assert torch.equal(out["texts"].cpu(), want["texts"]), what + ": texts after the replacement"
    assert torch.equal(out["idx"].cpu(), want["idx"]), what + ": idx"
    assert torch.equal(out["targets"].cpu(), want["targets"]), what + ": targets"


@pytest.mark.parametrize("mask_eos", [True, False], ids=["eos", "noeos"])
@pytest.mark.parametrize("B,S", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_mlm_mask_is_the_oracles(cuda, B, S, mask_eos):
    from imagetranslate_amd.utils import mask_text_count, unmask_text_device
    tp = R.SyntheticTextProcessor(V)
    texts, pads = _batch(B, S, seed=B * 31 + S)
    p = 0.5 if B * S < 300 else 0.15
    seed = 2 ** 40 + 17 + B
    want = M.mlm_mask_for(texts, pads, p, seed, tp, mask_eos)
    n = mask_text_count(p, pads, texts, tp, seed, mask_eos=mask_eos)
    assert n == want["count"], "mask_text_count is the device's count"
    out = _run(texts, pads, tp, p, seed, mask_eos)                 # the count read back
    _check(out, want, "%dx%d" % (B, S))
    again = _run(texts, pads, tp, p, seed, mask_eos, count=n)      # the count from the host: nothing read back
    _check(again, want, "%dx%d with a host count" % (B, S))
    assert again["idx"].numel() == n
    if B * S > 1:
        assert 0 < n < int(pads.sum()) or int(pads.sum()) < 3
    if not mask_eos:
        assert not bool(want["mask"][texts == 4].any())
    unmask_text_device(out)
    assert torch.equal(out["texts"].cpu(), texts), "unmask_text_device restores the input"


def test_holes_inside_rows_are_read_per_position(cuda):
    tp = R.SyntheticTextProcessor(V)
    texts, pads = _batch(9, 301, seed=5, holes=True)
    assert bool((~pads[0]).any()) and bool(pads[0, 1:][~pads[0, :-1]].any()), "a real token after a pad in one row"
    want = M.mlm_mask_for(texts, pads, 0.3, 99, tp)
    _check(_run(texts, pads, tp, 0.3, 99), want, "holes")
    assert not bool(want["mask"][~pads].any()) and want["count"] > 100


def test_pads_with_a_row_stride(cuda):
    """The pad bytes may be a column slice of a wider tensor (the row stride is an argument); texts may not."""
    from imagetranslate_amd._lib import ImtError
    from imagetranslate_amd.utils import mask_text_device
    tp = R.SyntheticTextProcessor(V)
    texts, pads = _batch(6, 50, seed=8)
    wide = torch.ones(6, 64, dtype=torch.bool)   # set bytes outside the slice must not be read
    wide[:, 3:53] = pads
    want = M.mlm_mask_for(texts, pads, 0.3, 7, tp)
    assert want["count"] < M.mlm_mask_for(texts, wide[:, :50], 0.3, 7, tp)["count"], "reading with the wrong stride or offset would tell"
    for view in (wide.cuda()[:, 3:53], wide.to(torch.uint8).cuda()[:, 3:53]):   # bool and uint8: both reach the kernel as they are
        assert view.stride() == (64, 1) and not view.is_contiguous()
        _check(mask_text_device(0.3, view, texts.cuda(), tp, 7), want, "strided pads")
    # a pad tensor whose positions are not unit-stride is copied, not refused
    _check(mask_text_device(0.3, pads.t().contiguous().t().cuda(), texts.cuda(), tp, 7), want, "column-major pads")
    for bad in (texts.cuda().t().contiguous().t(), texts.cuda()[:, ::2], texts, texts.cuda().int()):
        with pytest.raises(ImtError, match="in place"):
            mask_text_device(0.3, pads[:, :bad.shape[1]].cuda(), bad, tp, 7)


def test_all_pad_batch_selects_nothing(cuda):
    tp = R.SyntheticTextProcessor(V)
    texts = torch.randint(7, V, (4, 33), generator=torch.Generator().manual_seed(1))
    out = _run(texts, torch.zeros(4, 33, dtype=torch.bool), tp, 0.9, 5)
    assert int(out["count"].item()) == 0 and out["idx"].numel() == 0 and out["targets"].numel() == 0
    assert torch.equal(out["texts"].cpu(), texts) and not bool(out["mask"].any())


def test_smallest_replacement_range_and_seeds(cuda):
    tp = R.SyntheticTextProcessor(len(R.SyntheticTextProcessor(V).special_tokens) + 1)   # vocab = n_special + 1
    n_special = len(tp.special_tokens)
    texts = torch.full((40, 100), n_special, dtype=torch.int64)
    texts[:, ::3] = 1
    pads = torch.ones(40, 100, dtype=torch.bool)
    want = M.mlm_mask_for(texts, pads, 0.5, 21, tp)
    out = _run(texts, pads, tp, 0.5, 21)
    _check(out, want, "vocab = n_special + 1")
    new = out["texts"].cpu()[want["mask"]]
    assert set(new.tolist()) == {1, 3, n_special}, "every random replacement is n_special"
    from imagetranslate_amd.utils import _counter_uniform
    import numpy as np
    u5 = _counter_uniform(21, 5, np.arange(4000))[want["mask"].view(-1).numpy()]
    rnd = torch.from_numpy((u5 >= np.float32(0.8)) & (u5 < np.float32(0.9)))
    assert int(rnd.sum()) > 50 and bool((new[rnd] == n_special).all())
    # the same seed twice: the same bits; another seed: another mask
    tp2 = R.SyntheticTextProcessor(V)
    texts, pads = _batch(16, 200, seed=3)
    a, b, c = _run(texts, pads, tp2, 0.15, 1234), _run(texts, pads, tp2, 0.15, 1234), _run(texts, pads, tp2, 0.15, 1235)
    for k in ("mask", "texts", "idx", "targets", "count"):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["mask"], c["mask"])
    # a shared seed does not reuse the MASS kernel's streams: the selection is not a function of streams 0-3
    sel = _counter_uniform(1234, 4, np.arange(3200))
    assert all(not np.array_equal(sel, _counter_uniform(1234, s, np.arange(3200))) for s in (0, 1, 2, 3, 5, 6))


def test_a_wrong_count_hint_is_caught_when_checked(cuda, monkeypatch):
    from imagetranslate_amd._lib import ImtError
    tp = R.SyntheticTextProcessor(V)
    texts, pads = _batch(8, 32, seed=2)
    want = M.mlm_mask_for(texts, pads, 0.3, 4, tp)
    monkeypatch.setenv("IMT_CHECK_COUNT", "1")
    _run(texts, pads, tp, 0.3, 4, count=want["count"])
    with pytest.raises(ImtError, match="count hint"):
        _run(texts, pads, tp, 0.3, 4, count=want["count"] + 1)
