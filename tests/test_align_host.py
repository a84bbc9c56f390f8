"""Word alignment without a GPU: the two ported reference rules against tables the reference's own scripts produced
(tests/golden/alignment_dict, tests/golden/dense_alignments), word links and the Pharaoh writer on hand cases, the dictionary
file through ``dataset.get_lex_dict``, the command line, and every refusal of imt_align_pairs and of its wrapper (a refusal
precedes any launch, so no GPU is needed to see it)."""
import ctypes
import os

import pytest
import torch

from tests import align_oracle as AO

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD_DICT = os.path.join(HERE, "golden", "alignment_dict")
GOLD_DENSE = os.path.join(HERE, "golden", "dense_alignments")
TOK = os.path.join(HERE, "golden", "marshal_kat", "tok")
ERR = -1


def _lines(path):
    with open(path, encoding="utf-8") as fp:
        return fp.read().split("\n")[:-1]


def _links(line):
    return [tuple(int(v) for v in a.split("-")) for a in line.strip().split(" ") if "-" in a]


# ---------------------------------------------------------------------------------------------- the reference's rules
def test_alignment_dict_equals_the_reference_scripts_output():
    from imagetranslate_amd import align_pairs as AP
    from imagetranslate_amd.textprocessor import TextProcessor
    tp = TextProcessor(TOK)
    ids = lambda name: [[tp.token_id(w) for w in ln.strip().split(" ")] for ln in _lines(os.path.join(GOLD_DICT, name))]
    src, dst = ids("src.txt"), ids("dst.txt")
    links = [_links(ln) for ln in _lines(os.path.join(GOLD_DICT, "align.txt"))]
    assert len(src) == len(dst) == len(links) == 7 and links[3] == []
    rows = AP.build_alignment_dict(src, dst, links)
    want = [[int(v) for v in ln.split()] for ln in _lines(os.path.join(GOLD_DICT, "expected.txt"))]
    assert rows == want
    # what the fixture is there for: a key with more than five translations cut to five, the cut decided by a tie
    assert len(want[0]) == 6 and want[0][0] == 0 and 0 in want[0][1:] and {8, 41, 85}.isdisjoint(want[0])


def test_alignment_dict_counts_and_order_by_hand():
    from imagetranslate_amd import align_pairs as AP
    # 5 -> 9 twice, 5 -> 7 once, 6 -> 7 once: key 5 prefers 9; key 7 has a tie (5, 6) kept in first-seen order
    rows = AP.build_alignment_dict([[5, 6]], [[9, 7]], [[(0, 0), (0, 0), (0, 1), (1, 1)]])
    assert rows == [[5, 9, 7], [9, 5], [7, 5, 6], [6, 7]]
    assert AP.build_alignment_dict([], [], []) == []


def test_dense_pairs_equals_the_reference_scripts_output():
    from imagetranslate_amd import align_pairs as AP
    src, dst = _lines(os.path.join(GOLD_DENSE, "src.txt")), _lines(os.path.join(GOLD_DENSE, "dst.txt"))
    align = _lines(os.path.join(GOLD_DENSE, "align.txt"))
    assert len(src) == len(dst) == len(align) == 9
    kept = []
    for s, d, a in zip(src, dst, align):
        if AP.dense_pairs(s.strip().split(" "), d.strip().split(" "), len(_links(a)), 0.5):
            kept.append(s.strip() + " ||| " + d.strip())
    assert kept == _lines(os.path.join(GOLD_DENSE, "expected.txt"))
    assert len(kept) == 3


def test_dense_pairs_conditions_by_hand():
    from imagetranslate_amd import align_pairs as AP
    w = lambda n: ["w"] * n
    assert AP.dense_pairs(w(10), w(10), 5, 0.5)
    assert not AP.dense_pairs(w(10), w(10), 4, 0.5)            # density
    assert not AP.dense_pairs(w(4), w(4), 4, 0.5)              # both sides short
    assert not AP.dense_pairs(w(4), w(5), 5, 0.5) and not AP.dense_pairs(w(5), w(4), 5, 0.5)
    assert AP.dense_pairs(w(5), w(10), 5, 0.5)                 # ratio 0.5, but the difference is 5 and both are >= 5
    assert not AP.dense_pairs(w(5), w(11), 6, 0.5)             # difference 6
    assert AP.len_condition(w(3), w(3)) and not AP.len_condition(w(3), w(4))   # the ratio alone is enough, whatever the lengths
    # the deviation: a pair without links has density 0 here (the reference's "".split(" ") counts one link: 1 / 5 = 0.2)
    assert not AP.dense_pairs(w(5), w(5), 0, 0.2)


# ---------------------------------------------------------------------------------------------- words and the writer
def test_word_links_by_hand():
    from imagetranslate_amd import align_pairs as AP
    sw, dw = [0, 0, 0, 1, 2, 2], [0, 1, 1, 2]
    # one-to-many tokens: three tokens of word 0 against one target word, two links between the same words, unsorted input
    assert AP.word_links([(4, 3), (0, 0), (1, 0), (2, 1), (5, 3)], sw, dw) == [(0, 0), (0, 1), (2, 2)]
    assert AP.word_links([], sw, dw) == []
    assert AP.word_links([(0, 0)], [], dw) == [] and AP.word_links([(0, 0)], sw, []) == []   # an empty side links nothing
    assert AP.word_links([(0, 0), (1, 1)], [None, 3], [None, 4]) == [(3, 4)]                   # tokens without a word
    assert AP.word_links([(6, 0), (0, 4), (-1, 0)], sw, dw) == []                              # positions beyond the words


def test_pharaoh_writer_orders_by_source_then_target():
    from imagetranslate_amd import align_pairs as AP
    assert AP.pharaoh_line([(10, 2), (2, 10), (2, 3), (0, 11), (2, 3)]) == "0-11 2-3 2-10 10-2"
    assert AP.pharaoh_line([]) == ""


def test_written_dictionary_loads_with_get_lex_dict(tmp_path):
    from imagetranslate_amd import align_pairs as AP
    from imagetranslate_amd import dataset
    rows = AP.build_alignment_dict([[11, 12, 13]], [[21, 22, 11]], [[(0, 0), (1, 1), (1, 0), (2, 2)]])
    path = str(tmp_path / "dict.txt")
    AP.write_alignment_dict(path, rows)
    lex = dataset.get_lex_dict(path)
    assert lex == {r[0]: r[1:] for r in rows}
    assert lex[11] == [21, 13] and lex[13] == [11] and lex[12] == [22, 21] and lex[21] == [11, 12]
    assert dataset.get_lex_suggestions(lex, [12, 99], 0).tolist() == [21, 22]
    assert dataset.get_lex_suggestions(lex, [99], 0).tolist() == [0]


def test_option_parsing():
    from imagetranslate_amd import align_pairs as AP
    base = ["--tok", "t", "--model", "m", "--src-lang", "en", "--dst-lang", "fa", "--output", "o"]
    o, _ = AP.get_option_parser().parse_args(base + ["--src", "a", "--dst", "b"])
    AP.check_options(o)
    assert (o.model_type, o.min_sim, o.batch, o.fp32, o.token_output, o.dict_output, o.dense_output) == ("mt", 0.0, 4000, False, None, None, None)
    o, _ = AP.get_option_parser().parse_args(base + ["--pairs", "p", "--model-type", "sensim", "--min-sim", "0.3", "--batch", "100", "--fp32",
                                                     "--min-density", "0.8", "--dense-output", "d", "--dict-output", "x", "--token-output", "y"])
    AP.check_options(o)
    assert (o.pairs_path, o.model_type, o.min_sim, o.batch, o.fp32, o.min_density, o.dense_output) == ("p", "sensim", 0.3, 100, True, 0.8, "d")
    bad = [base + ["--src", "a"], base + ["--pairs", "p", "--src", "a"], base[2:] + ["--pairs", "p"], base[:-2] + ["--pairs", "p"],
           base + ["--pairs", "p", "--min-density", "0.5"], base + ["--pairs", "p", "--dense-output", "d"],
           base + ["--pairs", "p", "--batch", "0"]]
    for argv in bad:
        o, _ = AP.get_option_parser().parse_args(argv)
        with pytest.raises(ValueError):
            AP.check_options(o)
    with pytest.raises(SystemExit):
        AP.get_option_parser().parse_args(base + ["--model-type", "other"])


def test_read_pairs_takes_what_mine_pairs_writes(tmp_path):
    from imagetranslate_amd import align_pairs as AP
    p = tmp_path / "pairs.txt"
    p.write_text("a b\tc d\t0.5\ne\tf\n", encoding="utf-8")
    o, _ = AP.get_option_parser().parse_args(["--pairs", str(p)])
    assert AP.read_pairs(o) == (["a b", "e"], ["c d", "f"])


# ---------------------------------------------------------------------------------------------- the oracle itself
def test_oracle_on_a_hand_case():
    x = torch.tensor([[[9., 9.], [1., 0.], [0., 2.], [1., 1.], [9., 9.]]])
    y = torch.tensor([[[0., 3.], [0., 1.], [5., 0.], [0., 0.]]])
    link, fi, fv, bi, bv, sim = AO.align_oracle(x, y, torch.tensor([[1, 4]]), torch.tensor([[0, 4]]))
    assert fi.tolist() == [[-1, 2, 0, 0, -1]] and bi.tolist() == [[2, 2, 1, 1]]   # ties to the lowest index; the zero row: 0 everywhere
    assert link.tolist() == [[-1, 2, 0, -1, -1]]
    assert fv[0, 1] == 1.0 and abs(float(fv[0, 3]) - 0.5 ** 0.5) < 1e-12 and fv[0, 0] == float("-inf") and bv[0, 3] == 0.0
    assert sim[0, 0].max() == float("-inf")
    link2 = AO.align_oracle(x, y, torch.tensor([[1, 4]]), torch.tensor([[0, 4]]), min_sim=1.0)[0]
    assert link2.tolist() == [[-1, 2, 0, -1, -1]]
    empty = AO.align_oracle(x, y, torch.tensor([[2, 2]]), torch.tensor([[-5, 99]]))
    assert empty[1].eq(-1).all() and empty[3].eq(-1).all() and empty[0].eq(-1).all()


# ---------------------------------------------------------------------------------------------- refusals
def _args(L, **kw):
    """A complete, valid argument block with fake (never dereferenced) device addresses; kw overrides fields."""
    a = L.AlignArgs()
    a.dtype, a.B, a.S, a.T, a.d = L.IMT_BF16, 8, 70, 90, 512
    a.x, a.ldx, a.bsx = 0x100000, 512, 70 * 512
    a.y, a.ldy, a.bsy = 0x2000000, 512, 90 * 512
    a.xr, a.yr = 0x300000, 0x310000
    a.min_sim = 0.0
    a.link, a.fwd_idx, a.fwd_val, a.bwd_idx, a.bwd_val = 0x400000, 0x410000, 0x420000, 0x430000, 0x440000
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_align_pairs_refuses_bad_arguments_before_any_launch():
    """Every refusal is IMT_ERR_BAD_ARG with nothing enqueued: no GPU is present, a launch would fail with another code."""
    from imagetranslate_amd import _lib as L
    lib = L.load()
    assert lib.imt_abi_sizeof(b"imt_align_args") == ctypes.sizeof(L.AlignArgs)
    huge = 1 << 62
    cases = [
        (dict(dtype=7), b"dtype"), (dict(x=None), b" x is null"), (dict(y=None), b" y is null"), (dict(xr=None), b" xr is null"),
        (dict(yr=None), b" yr is null"), (dict(link=None), b" link is null"), (dict(fwd_idx=None), b"fwd_idx"),
        (dict(fwd_val=None), b"fwd_val"), (dict(bwd_idx=None), b"bwd_idx"), (dict(bwd_val=None), b"bwd_val"),
        (dict(B=0), b" B = 0"), (dict(B=-2), b" B = -2"), (dict(S=0), b" S = 0"), (dict(S=513), b" S = 513"), (dict(T=0), b" T = 0"),
        (dict(T=513), b" T = 513"),
        (dict(d=0), b"d 0"), (dict(d=520, ldx=520, ldy=520, bsx=70 * 520, bsy=90 * 520), b"d 520"),
        (dict(dtype=L.IMT_F32, d=48, ldx=48, ldy=48), b"d 48"),
        (dict(ldx=448), b"below d"), (dict(ldy=448), b"below d"),
        (dict(ldx=516, bsx=70 * 516), b"ldx"), (dict(ldy=516, bsy=90 * 516), b"ldy"), (dict(bsx=70 * 512 + 4), b"bsx"),
        (dict(bsy=90 * 512 + 4), b"bsy"), (dict(x=0x100008), b"x / ldx"), (dict(y=0x2000004), b"y / ldy"),
        (dict(bsx=69 * 512), b"bsx"), (dict(bsy=89 * 512 + 504), b"bsy"), (dict(bsx=0), b"bsx"),
        (dict(ldx=huge, bsx=huge), b"overflow"), (dict(ldy=huge, bsy=huge), b"overflow"),
        (dict(bsx=huge), b"overflow"), (dict(bsy=huge), b"overflow"), (dict(B=1 << 30, bsx=1 << 40), b"overflow"),
    ]
    for kw, name in cases:
        assert lib.imt_align_pairs(ctypes.byref(_args(L, **kw)), None) == ERR, kw
        msg = lib.imt_last_error()
        assert msg.startswith(b"align_pairs:") and name in msg, (kw, msg)
    assert lib.imt_align_pairs(None, None) == ERR and b"null args" in lib.imt_last_error()


def test_align_supported():
    from imagetranslate_amd import _lib as L
    lib = L.load()
    for dtype, step in ((L.IMT_BF16, 64), (L.IMT_F32, 32)):
        assert [lib.imt_align_supported(dtype, d) for d in (step, 2 * step, 768, step - 8, step + 8, 0, -step)] == [1, 1, 1, 0, 0, 0, 0]
    assert lib.imt_align_supported(5, 64) == 0


def test_wrapper_refuses_mismatches_and_has_no_cpu_fallback():
    from imagetranslate_amd import hip_ops as O
    from imagetranslate_amd._lib import ImtError
    x, y = torch.zeros(2, 5, 64), torch.zeros(2, 7, 64)
    r = torch.zeros(2, 2, dtype=torch.int32)
    bad = [
        (x[0], y, r, r), (x, y[:1], r, r), (x, torch.zeros(2, 7, 32), r, r), (x, y.bfloat16(), r, r), (x.half(), y.half(), r, r),
        (x.long(), y.long(), r, r), (x, y, r[:1], r), (x, y, r, torch.zeros(2, 3, dtype=torch.int32)), (x, y, r.float(), r),
        (x, y, r, r.bool()),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            O.align_pairs(*args)
    with pytest.raises(ImtError):   # valid shapes on the CPU: an error, never another implementation
        O.align_pairs(x, y, r, r)
