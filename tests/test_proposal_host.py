"""Lexical proposals (--dict) without a GPU: the dictionary file and the per-sentence lookup, the datasets' ``proposal`` rows,
the flag, and the host-side argument validation of imt_proposal_attn_fwd / imt_proposal_attn_bwd."""
import marshal
import random

import pytest
import torch

from imagetranslate_amd import _lib as L
from imagetranslate_amd.dataset import ImageCaptionDataset, MassDataset, MTDataset, get_lex_dict, get_lex_suggestions
from oracle import dataset_oracle as DO

PAD = 0


def _lex(seed=0, lo=7, hi=999, n=400):
    rnd = random.Random(seed)
    return {k: sorted({rnd.randint(lo, hi) for _ in range(rnd.randint(1, 4))}) for k in rnd.sample(range(lo, hi + 1), n)}


def _want(lex, ids):
    found = sorted({v for w in ids for v in lex.get(int(w), ())})
    return found or [PAD]


def test_get_lex_dict_parses_a_file(tmp_path):
    path = tmp_path / "dict.txt"
    path.write_text("7 11 12\n8 13\n\n7 14\n9\n")
    d = get_lex_dict(str(path))
    assert dict(d) == {7: [11, 12, 14], 8: [13], 9: []}
    assert all(isinstance(k, int) for k in d)


def test_get_lex_suggestions_int_keys_sorted_unique():
    lex = {3: [9, 7], 4: [7, 20], 5: []}
    as_list = get_lex_suggestions(lex, [4, 3, 3, 100], PAD)
    as_tensor = get_lex_suggestions(lex, torch.LongTensor([4, 3, 3, 100]), PAD)
    assert as_list.dtype == torch.int64 and as_list.tolist() == [7, 9, 20]
    assert torch.equal(as_list, as_tensor)  # a tensor's elements are looked up by value, not by identity
    assert get_lex_suggestions(lex, torch.LongTensor([1, 2, 5]), PAD).tolist() == [PAD]
    assert get_lex_suggestions(lex, [], PAD).tolist() == [PAD]
    assert 100 not in lex  # the lookup adds no keys


def _check_rows(proposal, sentences, lex):
    assert proposal.dim() == 2 and proposal.size(0) == len(sentences)
    want = [_want(lex, s) for s in sentences]
    assert proposal.size(1) == max(len(w) for w in want)
    for row, w in zip(proposal, want):
        assert row.tolist() == w + [PAD] * (proposal.size(1) - len(w))


def test_mt_dataset_proposals_follow_the_sources_across_splits():
    from tests.test_dataset import _parallel_examples, _same
    ex = _parallel_examples(120, seed=4)
    lex = _lex(1)
    kw = dict(max_batch_capacity=40, max_batch=700, pad_idx=PAD, examples=ex)
    with_dict, plain = MTDataset(lex_dict=lex, **kw), MTDataset(**kw)
    assert len(with_dict.batches) == len(plain.batches) > 3  # max_batch forces splits in the middle of the list
    k = 0
    for b, p in zip(with_dict.batches, plain.batches):
        n = b["src_texts"].size(0)
        _check_rows(b["proposal"], [e[0] for e in ex[k:k + n]], lex)
        k += n
        assert {kk: v for kk, v in b.items() if kk != "proposal"}.keys() == {kk for kk in p if kk != "proposal"}
        for kk in p:
            if kk != "proposal":
                assert torch.equal(b[kk], p[kk]), kk
    assert k == len(ex)
    _same(plain.batches, DO.mt_batches(ex, 700, 40, 175, 1, PAD))  # lex_dict=None: byte for byte what it was


def test_mass_dataset_proposals_follow_the_sentences_across_splits():
    from tests.test_dataset import _same
    rnd = random.Random(9)
    ex = sorted(([5] + [rnd.randint(7, 999) for _ in range(rnd.randint(3, 40))] + [4] for _ in range(90)), key=len)
    parts = [[(s, 0) for s in ex[:50]], [(s, 0) for s in ex[50:]]]
    lex = _lex(2)
    kw = dict(batch_pickle_dir=None, max_batch_capacity=5, max_batch=400, pad_idx=PAD, max_seq_len=64, example_list=parts)
    with_dict, plain = MassDataset(lex_dict=lex, **kw), MassDataset(**kw)
    assert len(with_dict.batches) == len(plain.batches) > 3
    k = 0
    for b, p in zip(with_dict.batches, plain.batches):
        n = b["src_texts"].size(0)
        _check_rows(b["proposal"], ex[k:k + n], lex)
        k += n
        for kk in p:
            if kk != "proposal":
                assert torch.equal(b[kk], p[kk]), kk
    assert k == len(ex)
    _same(plain.batches, DO.mass_batches(parts, 400, 5, 64, 1, PAD))


def test_caption_dataset_proposals_follow_the_captions_across_splits(tmp_path):
    from tests.test_multimodal import _Feats, _TP, _caption_file
    path, caps = _caption_file(tmp_path, 50)
    lex = _lex(3, lo=6, hi=89, n=50)
    mk = lambda **kw: ImageCaptionDataset("", path, 50, _TP(), 8, features=_Feats(), **kw)
    with_dict, plain = mk(lex_dict=lex), mk()
    assert len(with_dict) == len(plain) > 3
    k = 0
    for i in range(len(plain)):
        b, p = with_dict[i], plain[i]
        n = b["captions"].size(0)
        _check_rows(b["proposal"], [c[1] for c in caps[k:k + n]], lex)
        k += n
        assert p["proposal"] is None and b.keys() == p.keys()
        for kk in p:
            if kk != "proposal":
                assert torch.equal(b[kk], p[kk]), kk
    assert k == len(caps)


def test_dict_flag_is_accepted_only_where_it_is_supported():
    from imagetranslate_amd.option_parser import get_img_options_parser
    from imagetranslate_amd.train_image_mt import reject_off_path
    o, _ = get_img_options_parser().parse_args(["--dict", "d"])
    reject_off_path(o, dict_supported=True)
    with pytest.raises(NotImplementedError):
        reject_off_path(o)
    with pytest.raises(NotImplementedError):
        reject_off_path(o, lm_supported=True)


# ------------------------------------------------------------------------------------------- host validation of the C ABI
BAD_ARG, UNSUPPORTED = -1, -2
PTR = 0x1000  # never dereferenced on the host


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _fwd(lib, dtype=0, x=PTR, table=PTR, prop=PTR, gate=PTR, gamma=PTR, beta=PTR, y=PTR, scores=PTR, stats=PTR, rows=6, rpg=3, P=4,
         d=64, vocab=100):
    return lib.imt_proposal_attn_fwd(dtype, x, table, prop, gate, gamma, beta, y, scores, stats, rows, rpg, P, d, vocab, 0, 1e-12, None)


def _bwd(lib, dtype=0, dy=PTR, dx=PTR, dtable=PTR, ws=PTR, ws_bytes=None, rows=6, rpg=3, P=4, d=64, vocab=100):
    if ws_bytes is None:
        ws_bytes = max(int(lib.imt_proposal_attn_ws_bytes(rows, rpg, P, d)), 0)
    return lib.imt_proposal_attn_bwd(dtype, dy, PTR, PTR, PTR, PTR, PTR, PTR, PTR, dx, dtable, PTR, PTR, PTR, ws, ws_bytes, rows, rpg,
                                     P, d, vocab, 0, None)


def test_proposal_attn_refuses_bad_arguments_before_any_launch(lib):
    for call in (_fwd, _bwd):
        assert call(lib, dtype=7) == BAD_ARG and b"dtype" in lib.imt_last_error()
        assert call(lib, P=0) == BAD_ARG
        assert call(lib, P=-3) == BAD_ARG
        assert call(lib, rpg=0) == BAD_ARG
        assert call(lib, rpg=-1) == BAD_ARG
        assert call(lib, rows=7) == BAD_ARG          # not a multiple of rows_per_group
        assert call(lib, rows=-3) == BAD_ARG
        assert call(lib, vocab=0) == BAD_ARG
        for d in (0, 2, 66, 1028, 2048):
            assert call(lib, d=d) == UNSUPPORTED, d
            assert b"multiple of 4" in lib.imt_last_error()
        assert call(lib, rows=0) == 0                # nothing to do, nothing launched (null pointers are not even looked at)
    assert _fwd(lib, rows=0, x=None, y=None) == 0
    for name in ("x", "table", "prop", "gate", "gamma", "beta", "y", "scores", "stats"):
        assert _fwd(lib, **{name: None}) == BAD_ARG, name
        assert b"null" in lib.imt_last_error()
    for name in ("dy", "dx", "dtable", "ws"):
        assert _bwd(lib, **{name: None}) == BAD_ARG, name
    need = int(lib.imt_proposal_attn_ws_bytes(6, 3, 4, 64))
    assert need > 0
    assert _bwd(lib, ws_bytes=need - 1) == BAD_ARG and b"workspace" in lib.imt_last_error()
    assert _bwd(lib, ws_bytes=0) == BAD_ARG
    assert _bwd(lib, ws=PTR + 4) == BAD_ARG          # not 16-byte aligned


def test_proposal_attn_workspace_size(lib):
    """O(rows * P + G * P * d) plus row- and workgroup-sized vectors: nothing of rows * P * d."""
    ws = lib.imt_proposal_attn_ws_bytes
    assert ws(6, 0, 4, 64) == BAD_ARG and ws(6, 3, 0, 64) == BAD_ARG and ws(6, 3, 4, 66) == UNSUPPORTED
    assert ws(0, 3, 4, 64) == 0
    rows, rpg, P, d = 64 * 20, 20, 256, 512
    G = rows // rpg
    n = int(ws(rows, rpg, P, d))
    floor = 4 * (2 * rows * P + G * P * d)
    assert floor <= n <= floor + 4 * (rows * d + (G + rows // 8 + G) * 3 * d + 2 * G * P) + 16 * 8
    assert n < rows * P * d * 4 // 8


# ------------------------------------------------------------------------------------------- the edge cases have their edges
# tests/test_gpu_proposal_edges.py runs these shapes on the GPU; here the inputs are shown to reach what the table claims.
from tests import proposal_oracle as PO  # noqa: E402

EDGE_IDS = lambda s: "G%d_r%d_P%d_d%d" % s


@pytest.mark.parametrize("shape", list(PO.EDGE_CASES), ids=EDGE_IDS)
def test_edge_cases_split_p_into_the_listed_tiles(shape):
    _, _, P, d = shape
    for name, nbytes in (("fp32", 4), ("bf16", 2)):
        assert PO.tile_splits(nbytes, d, P) == PO.EDGE_CASES[shape][name], name
        assert sum(PO.EDGE_CASES[shape][name]) == P
    want = {(3, 17, 9, 1024): (8, 16), (3, 8, 64, 260): (31, 63), (4, 9, 33, 516): (15, 31)}  # PT before the clip to P
    if shape in want:
        assert (32768 // (d * 4), 32768 // (d * 2)) == want[shape]


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", list(PO.EDGE_CASES), ids=EDGE_IDS)
def test_edge_case_references_are_not_near_zero(shape, dtype_name):
    """A max-norm relative tolerance says something only about a tensor with a maximum: every reference tensor's is above 0.1."""
    _, want = PO.edge_case(shape, dtype_name)
    for k, v in want.items():
        assert float(v.abs().max()) > 0.1, (k, float(v.abs().max()))


def _positions_by_id(c):
    flat = c["prop"].flatten()
    pos = {}
    for i in PO.live_entries(flat, c["table"].shape[0], c["pad_idx"]).nonzero().flatten().tolist():
        pos.setdefault(int(flat[i]), []).append(i)
    return pos


@pytest.mark.parametrize("shape", PO.CHAIN_CASES, ids=EDGE_IDS)
def test_chain_cases_cross_chunk_and_workgroup_boundaries(shape):
    c, _ = PO.edge_case(shape, "fp32")
    assert c["prop"].numel() > 2 * PO.CHAIN_CHUNK
    pos = _positions_by_id(c)
    assert any(len({i // PO.CHAIN_CHUNK for i in p}) >= 3 for p in pos.values()), "no id with entries in three chunks"
    assert any(len(p) > 1 and p[0] // PO.CHAIN_THREADS != p[1] // PO.CHAIN_THREADS for p in pos.values()), \
        "no id whose first and next entries are in different workgroups"
    # an entry of the last workgroup whose chain began in chunk 0, and a link that leaves its chunk
    last_wg = (c["prop"].numel() - 1) // PO.CHAIN_THREADS
    assert any(p[0] < PO.CHAIN_CHUNK and p[-1] // PO.CHAIN_THREADS == last_wg for p in pos.values())
    assert any(a // PO.CHAIN_CHUNK != b // PO.CHAIN_CHUNK for p in pos.values() for a, b in zip(p, p[1:]))


def test_chain_emulation_matches_the_oracle_and_a_forgetful_one_does_not():
    """The chain-and-scatter of the backward restated on the host, applied to the oracle's per-entry gradients: as the kernel
    forms its links it gives the oracle's dtable; restarting the links with every chunk of 1024 ids misses it by far more than
    the GPU test's tolerance.  So case (20, 3, 130, 64) tells the two apart, and no broken kernel has to run to show it."""
    from tests.util import rel_err
    shape = PO.CHAIN_CASES[0]
    c, want = PO.edge_case(shape, "fp32")
    V = c["table"].shape[0]
    de = PO.proposal_reference(entry_grads=True, **c)["de"].reshape(-1, shape[3])
    nxt, first = PO.chain_links(c["prop"], V, c["pad_idx"])
    pos = _positions_by_id(c)
    assert sorted(first.nonzero().flatten().tolist()) == sorted(p[0] for p in pos.values())
    assert all(int(nxt[a]) == b for p in pos.values() for a, b in zip(p, p[1:])) and all(int(nxt[p[-1]]) == -1 for p in pos.values())
    assert rel_err(PO.scatter_chains(c["prop"], de, nxt, first, V), want["dtable"]) < 1e-12
    nxt, first = PO.chain_links(c["prop"], V, c["pad_idx"], forget_across_chunks=True)
    assert rel_err(PO.scatter_chains(c["prop"], de, nxt, first, V), want["dtable"]) > 1e-4


@pytest.mark.parametrize("shape", PO.CHAIN_CASES, ids=EDGE_IDS)
def test_one_row_per_entry_problem_sums_to_the_original(shape):
    """The exact entry-order check of the GPU test, in double: the per-entry problem has the same y and dx, its dtable rows
    are the per-entry gradients, and their sum per id in entry order is the original dtable."""
    from tests.util import rel_err
    c, want = PO.edge_case(shape, "fp32")
    c2 = PO.one_row_per_entry(c)
    n = c["prop"].numel()
    assert c2["table"].shape[0] == n + 1 and torch.equal(c2["table"][c2["prop"]], c["table"][c["prop"]])
    assert torch.equal(c2["prop"] == 0, c["prop"] == 0)
    want2 = PO.proposal_reference(entry_grads=True, **c2)
    assert torch.equal(want2["y"], want["y"]) and torch.equal(want2["dx"], want["dx"])
    live = (c["prop"].flatten() != 0)
    assert torch.equal(want2["dtable"][1:][live], want2["de"].reshape(n, -1)[live])
    assert rel_err(PO.sum_in_entry_order(c["prop"], want2["dtable"], c["table"].shape[0]), want["dtable"]) < 1e-12


def test_out_of_range_reference_is_the_plain_one_without_such_ids():
    c, want = PO.edge_case((3, 5, 7, 128), "fp32")
    got = PO.out_of_range_reference(c)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    # with them: four ids outside [0, V), both groups keep live ids, the table gradient keeps its shape
    c = PO.with_out_of_range_ids(c)
    V = c["table"].shape[0]
    bad = (c["prop"] < 0) | (c["prop"] >= V)
    assert int(bad.sum()) == 4 and sorted(c["prop"][bad].tolist()) == [-1, V, V + 7, 2 ** 40]
    assert bool(PO.live_entries(c["prop"], V, 0)[:2].any(-1).all())
    got = PO.out_of_range_reference(c)
    assert got["dtable"].shape == c["table"].shape and not torch.equal(got["y"], want["y"])
