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
