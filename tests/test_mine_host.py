"""Sentence mining without a GPU: host-side argument validation of imt_knn_rows, its workspace size, the command line of
mine_pairs, the mining oracle against a table the reference's extract_best_comparable.py produced, and the Python tail of
``mine`` on precomputed neighbour lists against that oracle."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import mine_oracle as MO

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mine_mutual_best")
ERR = -1


def _args(lib, L, **kw):
    """A complete, valid argument block with fake (never dereferenced) device addresses; kw overrides fields."""
    a = L.KnnArgs()
    a.dtype, a.N, a.M, a.K, a.k = L.IMT_BF16, 300, 1000, 512, 4
    a.x, a.ldx, a.y, a.ldy = 0x10000, 512, 0x200000, 512
    a.index_base, a.splits = 0, 0
    a.val, a.idx = 0x400000, 0x500000
    a.ws = 0x600000
    for k, v in kw.items():
        setattr(a, k, v)
    if "ws_bytes" not in kw:
        a.ws_bytes = max(lib.imt_knn_ws_bytes(a.N, a.M, a.k, a.splits), 1 << 20)
    return a


def test_knn_rows_refuses_bad_arguments_before_any_launch():
    """Every refusal is IMT_ERR_BAD_ARG with nothing enqueued: no GPU is present, a launch would fail with another code."""
    from imagetranslate_amd import _lib as L
    lib = L.load()
    assert lib.imt_abi_sizeof(b"imt_knn_args") == ctypes.sizeof(L.KnnArgs)
    need = lib.imt_knn_ws_bytes(300, 1000, 4, 0)
    big = (1 << 31) // (512 * 2)   # bf16 rows of 512 elements: 2 GiB worth
    cases = [
        (dict(dtype=7), b"dtype"), (dict(x=None), b" x is null"), (dict(y=None), b" y is null"), (dict(val=None), b" val is null"),
        (dict(idx=None), b" idx is null"), (dict(N=0), b" N = 0"), (dict(M=-3), b" M = -3"), (dict(K=0), b" K = 0"),
        (dict(k=0), b" k = 0"), (dict(k=9), b" k = 9"), (dict(splits=-1), b"splits = -1"), (dict(splits=257), b"splits = 257"),
        (dict(K=520, ldx=520, ldy=520), b"K 520"), (dict(dtype=L.IMT_F32, K=48, ldx=48, ldy=48), b"K 48"),
        (dict(ldx=448), b"ldx"), (dict(ldy=448), b"ldy"), (dict(ldx=516), b"ldx"), (dict(ldy=516), b"ldy"),
        (dict(x=0x10008), b"ldx"), (dict(y=0x200004), b"ldy"),
        (dict(N=big - 256), b"2 GiB"), (dict(M=big - 256), b"2 GiB"), (dict(N=1000, ldx=1 << 21), b"2 GiB"),
        (dict(ws=None), b"ws_bytes"), (dict(ws_bytes=need - 1), b"ws_bytes"), (dict(ws=0x600008), b"ws must be"),
        (dict(splits=7, ws_bytes=lib.imt_knn_ws_bytes(300, 1000, 4, 7) - 1), b"ws_bytes"),
        (dict(index_base=-1), b"index_base"), (dict(index_base=2 ** 31 - 1000), b"index_base"),
    ]
    for kw, name in cases:
        assert lib.imt_knn_rows(ctypes.byref(_args(lib, L, **kw)), None) == ERR, kw
        msg = lib.imt_last_error()
        assert msg.startswith(b"knn_rows:") and name in msg, (kw, msg)
    assert lib.imt_knn_rows(None, None) == ERR and b"null args" in lib.imt_last_error()


def test_knn_supported_and_workspace_size():
    from imagetranslate_amd import _lib as L
    lib = L.load()
    for K in (64, 512, 768):
        assert lib.imt_knn_supported(L.IMT_BF16, K) == 1 and lib.imt_knn_supported(L.IMT_F32, K) == 1
    assert lib.imt_knn_supported(L.IMT_F32, 32) == 1 and lib.imt_knn_supported(L.IMT_BF16, 32) == 0
    assert lib.imt_knn_supported(L.IMT_F32, 100) == 0 and lib.imt_knn_supported(3, 64) == 0 and lib.imt_knn_supported(L.IMT_F32, 0) == 0
    for N, M in ((1, 9), (300, 1000), (16384, 16384), (65536, 65536)):
        for k in (1, 4, 8):
            for splits in (1, 2, 3, 7, 256):
                b = lib.imt_knn_ws_bytes(N, M, k, splits)
                assert N * splits * k * 8 <= b <= N * splits * k * 8 + 256
                assert lib.imt_knn_ws_bytes(N + 1, M, k, splits) >= b and lib.imt_knn_ws_bytes(N + 300, M, k, splits) > b
                if k < 8:
                    assert lib.imt_knn_ws_bytes(N, M, k + 1, splits) > b
                if splits < 256:
                    assert lib.imt_knn_ws_bytes(N, M, k, splits + 1) > b
            auto = lib.imt_knn_ws_bytes(N, M, k, 0)   # the host's choice is one of the allowed values
            assert N * k * 8 <= auto <= N * 256 * k * 8 + 256
            assert lib.imt_knn_ws_bytes(N, M + 256, k, 0) >= auto
    assert lib.imt_knn_ws_bytes(0, 10, 4, 1) == 0 and lib.imt_knn_ws_bytes(10, 10, 9, 1) == 0 and lib.imt_knn_ws_bytes(10, 10, 4, 257) == 0


def test_abi_entries_are_declared_exported_and_bound():
    import re
    from imagetranslate_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "imt_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(imt_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    for name in ("imt_knn_rows", "imt_knn_ws_bytes", "imt_knn_supported"):
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    assert "#define IMT_KNN_MAX_K 8" in hdr


def test_command_line_parses_and_requires_its_paths():
    from imagetranslate_amd import mine_pairs as P
    parse = lambda argv: P.get_option_parser().parse_args(argv)[0]
    o = parse([])
    assert (o.k, o.margin, o.min_score, o.bf16_search, o.fp32) == (4, "ratio", 0.0, False, False)
    full = ["--model", "m", "--tok", "t", "--src", "a", "--dst", "b", "--output", "o"]
    o = parse(full + ["--k", "8", "--margin", "none", "--min", "0.25", "--batch", "900", "--capacity", "30", "--fp32", "--bf16-search"])
    assert (o.model_path, o.tokenizer_path, o.src_dir, o.dst_dir, o.output) == ("m", "t", "a", "b", "o")
    assert (o.k, o.margin, o.min_score, o.batch, o.total_capacity, o.fp32, o.bf16_search) == (8, "none", 0.25, 900, 30, True, True)
    with pytest.raises(SystemExit):
        parse(["--margin", "distance"])
    for flag in ("--model", "--src", "--dst", "--output"):
        argv = list(full)
        at = argv.index(flag)
        del argv[at:at + 2]
        with pytest.raises(ValueError, match=flag):
            P.mine_pairs(parse(argv))


def _fixture():
    col = lambda name: open(os.path.join(GOLD, name)).read().split("\n")[:-1]
    src, dst, scores = col("src.txt"), col("dst.txt"), col("scores.txt")
    assert len(src) == len(dst) == len(scores) == 42
    N, M = 1 + max(int(s[1:]) for s in src), 1 + max(int(t[1:]) for t in dst)
    sim = np.full((N, M), -np.inf)
    for s, t, v in zip(src, dst, scores):
        sim[int(s[1:]), int(t[1:])] = float(v)
    want = []
    for line in col("expected.txt"):
        pair, v = line.split("\t")
        s, t = pair.split(" ||| ")
        want.append((int(s[1:]), int(t[1:]), float(v)))
    return sim, want


def test_oracle_margin_none_reproduces_the_reference_scripts_output():
    """tests/golden/mine_mutual_best: the candidate table and what the reference's extract_best_comparable.py wrote for it with
    --min 0.3 (generate.py beside it ran the script).  The table has ties on both sides, two kept pairs of one score and a
    mutual-best pair below --min."""
    sim, want = _fixture()
    assert len(want) == 3 and len({v for _, _, v in want}) == 2, "two of the kept pairs share a score"
    for k in (1, 4):
        assert MO.mine_reference(sim, k, "none", 0.3) == want
    lower = MO.mine_reference(sim, 1, "none", 0.0)
    assert len(lower) == 4 and (4, 4, 0.25) in lower, "the pair below --min is mutual best"


def _dyadic(N, M, seed, lo=-16):
    """Similarities that are multiples of 1/64: sums and halves of them are exact in any order, so the tail and the oracle
    must agree to the bit, and equal scores are common."""
    rng = np.random.RandomState(seed)
    return rng.randint(lo, 64, size=(N, M)).astype(np.float64) / 64.0


@pytest.mark.parametrize("N,M,k", [(40, 55, 4), (30, 30, 1), (3, 50, 8), (50, 3, 8), (1, 1, 4), (64, 64, 2)])
@pytest.mark.parametrize("margin", ["none", "ratio"])
def test_tail_of_mine_on_precomputed_lists_equals_the_oracle(N, M, k, margin):
    from imagetranslate_amd.mine_pairs import select_pairs
    for seed, lo in ((N + M + k, -16), (7 * N + k, 40), (N, -64)):   # mixed signs, crowded positives, mostly negative
        sim = _dyadic(N, M, seed, lo)
        fv, fi = MO.knn_from_sim(sim, k)
        bv, bi = MO.knn_from_sim(sim.T, k)
        for min_score in (0.0, 0.5, -10.0):
            want = MO.mine_reference(sim, k, margin, min_score)
            s, t, sc = select_pairs(torch.from_numpy(fv).float(), torch.from_numpy(fi), torch.from_numpy(bv).float(),
                                    torch.from_numpy(bi), margin, min_score)
            assert list(zip(s.tolist(), t.tolist(), sc.tolist())) == want, (seed, min_score)
    with pytest.raises(ValueError):
        select_pairs(torch.zeros(1, 1), torch.zeros(1, 1, dtype=torch.long), torch.zeros(1, 1), torch.zeros(1, 1, dtype=torch.long), "max")
