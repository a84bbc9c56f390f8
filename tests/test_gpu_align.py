"""imt_align_pairs on the GPU against the fp64 oracle (tests/align_oracle.py): exact links where the data decides them (planted
permutations, ties, ranges, the threshold), tolerance-aware parity on Gaussian inputs, determinism, and the entry point end to end.

The kernel's edges: a workgroup owns a pair and walks 64 x 64 tiles counted from the ranges' begins (row blocks of 64 source
positions, column tiles of 64 target positions), d in steps of 128 bytes (64 bf16 / 32 fp32 elements); with three workgroups
of 42.5 KiB LDS per CU at most 768 run at once.  There is no split of a pair over workgroups.

Tolerance: the project's fp32 bar of 1e-4 on the cosines.  The oracle reads the values as stored (bf16 inputs are upcast: the
product of two bf16 numbers is exact in fp32), so the same bar holds for both dtypes.  An index is compared where the oracle's
top-1 margin is at least 2e-4 (twice the bar: both candidates may move by 1e-4); elsewhere the returned index must be within
2e-4 of the best."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import align_oracle as AO

pytestmark = pytest.mark.gpu
TOL = 1e-4
BAND = 2 * TOL
DTYPES = [torch.float32, torch.bfloat16]
EDGES = [1, 63, 64, 65, 129, 512]     # 1, tile - 1, tile, tile + 1, two tiles + 1, the limit
NINF = float("-inf")
HERE = os.path.dirname(os.path.abspath(__file__))


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def _full(B, n):
    return torch.tensor([[0, n]] * B, dtype=torch.int32)


def _margins(sim):
    """fp64 top-1 margins of the rows (dim 2) and the columns (dim 1) of ``sim``; inf where fewer than two candidates."""
    def m(s, dim):
        if s.shape[dim] < 2:
            return torch.full_like(s.max(dim=dim).values, float("inf"))
        top = s.topk(2, dim=dim).values
        a, b = top.select(dim, 0), top.select(dim, 1)
        return torch.where(torch.isinf(b), torch.full_like(a, float("inf")), a - b)
    return m(sim, 2), m(sim, 1)


@functools.lru_cache(maxsize=None)
def planted(B, S, T, d, dtype, seed=0):
    """Pairs whose links the data decides: with n = min(S, T), n target rows are the source rows under a random permutation plus
    noise of norm 1e-3; the |S - T| extra rows of the longer side have cosine 0.8 to one row of the other side (cycling), so their
    best is decided too while that row still prefers its partner by 0.2.  Returns the operands in ``dtype`` and the oracle's
    outputs on them; asserts that every top-1 margin exceeds 0.1."""
    rng = np.random.RandomState(seed + 7 * S + 13 * T + d)
    n = min(S, T)
    x = np.zeros((B, S, d))
    y = np.zeros((B, T, d))
    for b in range(B):
        base = _unit(rng.randn(n, d))
        perm = rng.permutation(n)
        spos, tpos = rng.permutation(S), rng.permutation(T)   # where the matched rows sit; the rest are the extras
        x[b, spos[:n]] = base
        y[b, tpos[:n]] = base[perm] + 1e-3 * _unit(rng.randn(n, d))
        for side, pos, other in ((x, spos, y[b, tpos[:n]]), (y, tpos, x[b, spos[:n]])):
            for e, p in enumerate(pos[n:]):
                anchor = _unit(other[e % n])
                noise = rng.randn(d)
                noise = _unit(noise - noise.dot(anchor) * anchor)
                side[b, p] = 0.8 * anchor + 0.6 * noise
    scale = rng.uniform(0.5, 2.0, size=(B, S, 1)), rng.uniform(0.5, 2.0, size=(B, T, 1))   # the norms are the kernel's to take out
    xt, yt = torch.from_numpy(x * scale[0]).to(dtype), torch.from_numpy(y * scale[1]).to(dtype)
    ref = AO.align_oracle(xt, yt, _full(B, S), _full(B, T))
    mf, mb = _margins(ref[5])
    assert min(float(mf.min()), float(mb.min())) > 0.1, "planted margin %.3f / %.3f" % (float(mf.min()), float(mb.min()))
    if S == T:
        assert (ref[0] >= 0).all(), "every position of a square planted pair is linked"
    return xt, yt, ref


def run(x, y, xr, yr, min_sim=NINF):
    from imagetranslate_amd import hip_ops as O
    out = O.align_pairs(x.cuda(), y.cuda(), xr.cuda(), yr.cuda(), min_sim)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def assert_exact(out, ref, what=""):
    for name, a, b in zip(("link", "fwd_idx", "fwd_val", "bwd_idx", "bwd_val"), out, ref):
        if a.dtype.is_floating_point:
            fin = torch.isfinite(b)
            assert torch.equal(torch.isfinite(a), fin), (what, name)
            assert a[~fin].eq(NINF).all(), (what, name)
            err = float((a[fin].double() - b[fin]).abs().max()) if fin.any() else 0.0
            assert err <= TOL, (what, name, err)
        else:
            assert a.dtype == torch.int64 and torch.equal(a, b), (what, name, int((a != b).sum()))


# ---------------------------------------------------------------------------------------------- planted links
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("S", EDGES)
def test_planted_links_at_tile_edges(cuda, S, dtype):
    for T in EDGES:
        x, y, ref = planted(2, S, T, 128, dtype)
        assert_exact(run(x, y, _full(2, S), _full(2, T)), ref, "S %d T %d" % (S, T))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("d", ["step", 40, 768])
def test_planted_links_at_widths(cuda, d, dtype):
    """One K step (no prefetch in flight), a width the wrapper pads with zeros, the models' 768."""
    if d == "step":
        d = 128 // torch.empty(0, dtype=dtype).element_size()
    x, y, ref = planted(3, 34, 21, d, dtype)
    assert_exact(run(x, y, _full(3, 34), _full(3, 21)), ref, "d %d" % d)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 800])
def test_planted_links_at_batch_sizes(cuda, B, dtype):
    """One pair, and more pairs than workgroups that run at once (768)."""
    x, y, ref = planted(B, 20, 23, 64, dtype)
    assert_exact(run(x, y, _full(B, 20), _full(B, 23)), ref, "B %d" % B)


# ---------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_ties_go_to_the_lowest_index(cuda, dtype):
    S, T, d = 70, 131, 64
    x, y, base = planted(1, S, T, d, dtype)
    x, y = x.clone(), y.clone()
    # the partner of source row 17 gets two copies in other column tiles; source row 17 gets copies in another wave's rows and in
    # the second row block; one all-zero row on each side
    j0 = int(base[1][0, 17])
    js = sorted({j0, (j0 + 64) % T, (j0 + 100) % T})
    for j in js:
        y[0, j] = y[0, j0].clone()
    for i in (2, 66):
        x[0, i] = x[0, 17].clone()
    zi, zj = 5, min(j for j in range(T) if j not in js)
    x[0, zi] = 0
    y[0, zj] = 0
    ref = AO.align_oracle(x, y, _full(1, S), _full(1, T))
    out = run(x, y, _full(1, S), _full(1, T))
    link, fi, fv, bi, bv = out
    assert torch.equal(fi, ref[1]) and torch.equal(bi, ref[3]) and torch.equal(link, ref[0])
    assert fi[0, 2] == js[0] and fi[0, 17] == js[0] and fi[0, 66] == js[0]          # the lowest of the equal targets
    assert bi[0, js[0]] == 2 and bi[0, js[1]] == 2 and bi[0, js[2]] == 2            # the lowest of the equal sources
    assert link[0, 2] == js[0] and link[0, 17] == -1 and link[0, 66] == -1          # the mutual rule follows
    assert fi[0, zi] == 0 and fv[0, zi] == 0.0 and bi[0, zj] == 0 and bv[0, zj] == 0.0   # cosine 0 everywhere: the lowest index
    assert_exact(out, ref)


# ---------------------------------------------------------------------------------------------- ranges
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_ranges(cuda, dtype):
    B, S, T, d = 6, 67, 130, 64
    x, y, _ = planted(B, S, T, d, dtype)
    xr = torch.tensor([[1, 66], [0, 67], [5, 5], [0, 67], [-3, 900], [66, 2]], dtype=torch.int32)
    yr = torch.tensor([[1, 129], [64, 65], [0, 130], [130, 130], [-1, 131], [0, 130]], dtype=torch.int32)
    ref = AO.align_oracle(x, y, xr, yr)
    out = run(x, y, xr, yr)
    assert_exact(out, ref)
    link, fi, fv, bi, bv = out
    assert fi[0, 0] == -1 and fi[0, 66] == -1 and bi[0, 0] == -1 and bi[0, 129] == -1 and (fi[0, 1:66] >= 1).all() and (fi[0, 1:66] < 129).all()
    assert (fi[1] == 64).all() and (bi[1, :64] == -1).all() and bi[1, 64] >= 0
    for b in (2, 3, 5):   # an empty range on either side (begin == end, or end below begin): nothing anywhere
        assert (fi[b] == -1).all() and (bi[b] == -1).all() and (link[b] == -1).all() and (fv[b] == NINF).all() and (bv[b] == NINF).all()
    full = run(x[4:5], y[4:5], _full(1, S), _full(1, T))   # ranges beyond the tensors are clamped to them
    for a, c in zip(out, full):
        assert torch.equal(a[4:5], c)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("fill", [float("nan"), 1e30], ids=["nan", "1e30"])
def test_padding_rows_never_reach_a_result(cuda, fill, dtype):
    B, S, T, d = 3, 66, 70, 64
    x, y, _ = planted(B, S, T, d, dtype)
    xr = torch.tensor([[1, 40], [3, 66], [0, 65]], dtype=torch.int32)
    yr = torch.tensor([[2, 64], [0, 69], [1, 70]], dtype=torch.int32)
    xz, yz = x.clone(), y.clone()
    xp, yp = x.clone(), y.clone()
    for b in range(B):
        for t, z, r in ((xp, xz, xr), (yp, yz, yr)):
            t[b, :r[b, 0]] = fill
            t[b, r[b, 1]:] = fill
            z[b, :r[b, 0]] = 0
            z[b, r[b, 1]:] = 0
    want = run(xz, yz, xr, yr)
    got = run(xp, yp, xr, yr)
    for a, c in zip(got, want):
        assert torch.equal(a, c)
    assert_exact(got, AO.align_oracle(xp, yp, xr, yr))


# ---------------------------------------------------------------------------------------------- min_sim
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_min_sim_drops_links_below_it(cuda, dtype):
    """Orthonormal source rows; target row k has cosine c_k to source row k and is orthogonal to the others: half the pairs
    sit 0.01 above the threshold 0.6, half 0.01 below (both 100 tolerances away)."""
    n, d = 40, 64
    rng = np.random.RandomState(3)
    q, _ = np.linalg.qr(rng.randn(d, d))
    basis = q.T
    cos = np.where(np.arange(n) % 2 == 0, 0.61, 0.59)
    x = basis[:n][None]
    y = (cos[:, None] * basis[:n] + np.sqrt(1 - cos ** 2)[:, None] * basis[n:n + 1])[None]   # the rest along one spare direction
    xt, yt = torch.from_numpy(x).to(dtype), torch.from_numpy(y).to(dtype)
    ref_all = AO.align_oracle(xt, yt, _full(1, n), _full(1, n))
    ref = AO.align_oracle(xt, yt, _full(1, n), _full(1, n), min_sim=0.6)
    assert (ref_all[0][0] == torch.arange(n)).all() and ((ref_all[2][0] - 0.6).abs() > 50 * TOL).all()
    assert (ref[0][0, 0::2] == torch.arange(0, n, 2)).all() and (ref[0][0, 1::2] == -1).all()
    out = run(xt, yt, _full(1, n), _full(1, n), 0.6)
    assert_exact(out, ref)
    assert torch.equal(out[1], ref_all[1]) and torch.equal(out[3], ref_all[3])   # the arg-max itself is unaffected
    assert_exact(run(xt, yt, _full(1, n), _full(1, n)), ref_all)


# ---------------------------------------------------------------------------------------------- random inputs
@functools.lru_cache(maxsize=None)
def gaussian(B, S, T, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, d, generator=g).to(dtype)
    y = torch.randn(B, T, d, generator=g).to(dtype)
    xr = _full(B, S)
    yr = _full(B, T)
    if B > 1:   # the framed-sentence case on some pairs
        xr[1] = torch.tensor([1, S - 1])
        yr[1] = torch.tensor([1, T - 1])
    return x, y, xr, yr, AO.align_oracle(x, y, xr, yr)


def assert_parity(out, ref, xr, yr):
    """Values within TOL; indices equal where decided (margin >= BAND), else within BAND of the best; at least 97 % decided."""
    link, fi, fv, bi, bv = out
    r_link, r_fi, r_fv, r_bi, r_bv, sim = ref
    mf, mb = _margins(sim)
    live_f, live_b = r_fi >= 0, r_bi >= 0
    dec_f, dec_b = live_f & (mf >= BAND), live_b & (mb >= BAND)
    share = (int(dec_f.sum()) + int(dec_b.sum())) / max(1, int(live_f.sum()) + int(live_b.sum()))
    assert share >= 0.97, "only %.3f of the positions are decided" % share   # from the oracle alone
    for got_v, want_v in ((fv, r_fv), (bv, r_bv)):
        fin = torch.isfinite(want_v)
        assert torch.equal(torch.isfinite(got_v), fin) and got_v[~fin].eq(NINF).all()
        assert float((got_v[fin].double() - want_v[fin]).abs().max()) <= TOL
    assert torch.equal(fi[dec_f], r_fi[dec_f]) and torch.equal(bi[dec_b], r_bi[dec_b])
    assert torch.equal(fi >= 0, live_f) and torch.equal(bi >= 0, live_b)
    # the rest: the chosen index is one of the near-best
    pick_f = sim.gather(2, fi.clamp(min=0).unsqueeze(2)).squeeze(2)
    pick_b = sim.gather(1, bi.clamp(min=0).unsqueeze(1)).squeeze(1)
    assert ((r_fv - pick_f)[live_f] <= BAND).all() and ((r_bv - pick_b)[live_b] <= BAND).all()
    # the mutual rule on the kernel's own indices, and the oracle's links where both sides are decided
    back = bi.gather(1, fi.clamp(min=0))
    own = torch.where(live_f & (back == torch.arange(fi.shape[1])[None]), fi, torch.full_like(fi, -1))
    assert torch.equal(link, own)
    both = dec_f & dec_b.gather(1, r_fi.clamp(min=0))
    assert torch.equal(link[both], r_link[both])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", [(8, 65, 130, 64), (4, 257, 300, 96), (64, 33, 17, 768)], ids=lambda s: "x".join(map(str, s)))
def test_gaussian_inputs_against_fp64(cuda, shape, seed, dtype):
    x, y, xr, yr, ref = gaussian(*shape, dtype, seed)
    assert_parity(run(x, y, xr, yr), ref, xr, yr)


# ---------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_deterministic_and_independent_of_the_batch(cuda, dtype):
    x, y, xr, yr, _ = gaussian(8, 65, 130, 64, dtype, 0)
    a, b = run(x, y, xr, yr), run(x, y, xr, yr)
    for u, v in zip(a, b):
        assert torch.equal(u, v)   # (-inf == -inf; no NaN is ever written)
    for p in (0, 1, 7):
        alone = run(x[p:p + 1], y[p:p + 1], xr[p:p + 1], yr[p:p + 1])
        for u, v in zip(a, alone):
            assert torch.equal(u[p:p + 1], v)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_non_contiguous_views(cuda, dtype):
    from imagetranslate_amd import hip_ops as O
    x, y, xr, yr, _ = gaussian(8, 65, 130, 64, dtype, 1)
    want = run(x, y, xr, yr)
    xw = torch.zeros(8, 70, 192, dtype=dtype)   # a view the kernel takes as it is: rows and pairs further apart
    xw[:, 2:67, 64:128] = x
    yw = torch.zeros(130, 8, 64, dtype=dtype)   # pairs interleaved: batch stride below a pair's extent, the wrapper copies
    yw.copy_(y.transpose(0, 1))
    xv, yv = xw.cuda()[:, 2:67, 64:128], yw.cuda().transpose(0, 1)
    assert not xv.is_contiguous() and not yv.is_contiguous()
    assert O._align_operand(xv).data_ptr() == xv.data_ptr() and O._align_operand(yv).data_ptr() != yv.data_ptr()
    got = [t.cpu() for t in O.align_pairs(xv, yv, xr.cuda(), yr.cuda())]
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    xs = x.cuda()[:, ::2]   # every second source position: a row stride of two rows
    got = [t.cpu() for t in O.align_pairs(xs, y.cuda(), _full(8, 33).cuda(), yr.cuda())]
    for u, v in zip(got, run(x[:, ::2].contiguous(), y, _full(8, 33), yr)):
        assert torch.equal(u, v)


def test_empty_batch(cuda):
    from imagetranslate_amd import hip_ops as O
    out = O.align_pairs(torch.zeros(0, 5, 64, device="cuda"), torch.zeros(0, 7, 64, device="cuda"),
                        torch.zeros(0, 2, dtype=torch.int32, device="cuda"), torch.zeros(0, 2, dtype=torch.int32, device="cuda"))
    assert [tuple(t.shape) for t in out] == [(0, 5), (0, 5), (0, 5), (0, 7), (0, 7)]
    assert [t.dtype for t in out] == [torch.int64, torch.int64, torch.float32, torch.int64, torch.float32]


def test_kernel_refusals_surface_as_imt_error(cuda):
    from imagetranslate_amd import hip_ops as O
    from imagetranslate_amd._lib import ImtError
    r = torch.zeros(1, 2, dtype=torch.int32, device="cuda")
    with pytest.raises(ImtError):
        O.align_pairs(torch.zeros(1, 513, 64, device="cuda"), torch.zeros(1, 7, 64, device="cuda"), r, r)


# ---------------------------------------------------------------------------------------------- end to end
def _lines(path):
    with open(path, encoding="utf-8") as fp:
        return fp.read().split("\n")[:-1]


def _links(line):
    return [tuple(int(v) for v in a.split("-")) for a in line.split(" ") if "-" in a]


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    """A toy Seq2Seq (random weights) saved with the marshal_kat tokenizer, and one run of the entry point in fp32 on six pairs."""
    from imagetranslate_amd import align_pairs as AP
    from imagetranslate_amd.seq2seq import Seq2Seq
    from imagetranslate_amd.textprocessor import TextProcessor
    d = str(tmp_path_factory.mktemp("align"))
    tok = os.path.join(HERE, "golden", "marshal_kat", "tok")
    tp = TextProcessor(tok)
    torch.manual_seed(11)
    Seq2Seq(tp, lang_dec=False, enc_layer=2, dec_layer=1, embed_dim=64, intermediate_dim=128, num_attention_heads=2).save(os.path.join(d, "model"))
    gold = os.path.join(HERE, "golden", "sample_enfa")
    pick = [9, 11, 17, 24, 43, 13]
    en, fa = _lines(os.path.join(gold, "en.txt")), _lines(os.path.join(gold, "fa.txt"))
    src, dst = [en[i].strip() for i in pick], [fa[i].strip() for i in pick]
    p = lambda name: os.path.join(d, name)
    for name, lines in (("src.txt", src), ("dst.txt", dst), ("pairs.txt", [s + "\t" + t + "\t0.5" for s, t in zip(src, dst)])):
        with open(p(name), "w", encoding="utf-8") as w:
            w.write("\n".join(lines) + "\n")
    common = ["--tok", tok, "--model", p("model"), "--src-lang", "en", "--dst-lang", "fa", "--fp32", "--min-density", "0.3"]
    AP.main(common + ["--src", p("src.txt"), "--dst", p("dst.txt"), "--output", p("word.txt"), "--token-output", p("token.txt"),
                      "--dict-output", p("dict.txt"), "--dense-output", p("dense.txt")])
    AP.main(common + ["--pairs", p("pairs.txt"), "--output", p("word2.txt"), "--token-output", p("token2.txt"),
                      "--dict-output", p("dict2.txt"), "--dense-output", p("dense2.txt")])
    return dict(dir=d, tok=tok, src=src, dst=dst, p=p)


def test_entry_point_end_to_end(cuda, cli_run):
    from imagetranslate_amd import align_pairs as AP
    p, src, dst = cli_run["p"], cli_run["src"], cli_run["dst"]
    model, tp = AP.load_model("mt", p("model"), cli_run["tok"])
    model.set_compute_dtype(torch.float32)
    model = model.cuda().eval()
    enc = [(tp.tokenizer.encode(s), tp.tokenizer.encode(t)) for s, t in zip(src, dst)]
    sep, pad = tp.token_id("</s>"), tp.pad_token_id()
    fs = [tp.tokenize_one_sentence_with_langid(s, tp.token_id("<en>")) for s in src]
    fd = [tp.tokenize_one_sentence_with_langid(t, tp.token_id("<fa>")) for t in dst]
    assert all(f[-1] == sep and len(f) == len(e.ids) + 2 for f, (e, _) in zip(fs, enc))
    links, raw = AP.align_batch(model, fs, fd, tp.languages["<en>"], tp.languages["<fa>"], pad, min_sim=0.0, return_raw=True)
    assert raw["x_range"].tolist() == [[1, len(f) - 1] for f in fs] and raw["y_range"].tolist() == [[1, len(f) - 1] for f in fd]
    # token links: the oracle on the model's own states, under the decided-position rule (the threshold 0 counts as a candidate)
    ref = AO.align_oracle(raw["x"], raw["y"], raw["x_range"], raw["y_range"], min_sim=0.0)
    mf, mb = _margins(ref[5])
    token = [_links(ln) for ln in _lines(p("token.txt"))]
    assert len(token) == 6 and sum(len(t) for t in token) > 0
    decided = total = 0
    for b in range(6):
        got = dict(token[b])
        assert len(got) == len(token[b]) and token[b] == sorted(token[b])
        for i in range(1, len(fs[b]) - 1):
            j = int(ref[1][b, i])
            total += 1
            if mf[b, i] >= BAND and mb[b, j] >= BAND and abs(float(ref[2][b, i])) >= BAND:
                decided += 1
                want = int(ref[0][b, i])
                assert got.get(i - 1, -2) + 1 == want, (b, i, got.get(i - 1), want)
        assert all(0 <= i < len(enc[b][0].ids) and 0 <= j < len(enc[b][1].ids) for i, j in token[b])   # never the tag, never </s>
    assert 2 * decided >= total, (decided, total)   # states of a random model differ at O(1): near-ties are the exception
    # everything else is the host functions applied to those token links
    words = [(list(es.word_ids), list(ed.word_ids)) for es, ed in enc]
    wl = [AP.word_links(t, ws, wd) for t, (ws, wd) in zip(token, words)]
    assert _lines(p("word.txt")) == [AP.pharaoh_line(l) for l in wl]
    rows = AP.build_alignment_dict([list(es.ids) for es, _ in enc], [list(ed.ids) for _, ed in enc], token)
    assert _lines(p("dict.txt")) == [" ".join(str(v) for v in r) for r in rows] and len(rows) > 0
    dense = [s + " ||| " + t for s, t, l, (ws, wd) in zip(src, dst, wl, words)
             if AP.dense_pairs(range(AP.n_words(ws)), range(AP.n_words(wd)), len(l), 0.3)]
    assert _lines(p("dense.txt")) == dense
    # --pairs (what mine_pairs writes) gives the same lines
    for a, b in (("word.txt", "word2.txt"), ("token.txt", "token2.txt"), ("dict.txt", "dict2.txt"), ("dense.txt", "dense2.txt")):
        assert _lines(p(a)) == _lines(p(b)), b


def test_written_dictionary_feeds_dict_batches(cuda, cli_run):
    """The file is what ``train_image_mt --dict`` reads: get_lex_dict -> MTDataset -> batch["proposal"]."""
    from imagetranslate_amd import dataset
    from imagetranslate_amd.textprocessor import TextProcessor
    tp = TextProcessor(cli_run["tok"])
    lex = dataset.get_lex_dict(cli_run["p"]("dict.txt"))
    assert lex and all(1 <= len(v) <= 5 for v in lex.values())
    ex = [(tp.tokenize_one_sentence_with_langid(s, tp.token_id("<en>")), tp.tokenize_one_sentence_with_langid(t, tp.token_id("<fa>")), 0, 1)
          for s, t in zip(cli_run["src"], cli_run["dst"])]
    data = dataset.MTDataset(max_batch_capacity=600, max_batch=4000, pad_idx=tp.pad_token_id(), examples=ex, lex_dict=lex)
    prop = torch.cat([b["proposal"].reshape(-1) for b in data.batches])
    assert sum(b["proposal"].size(0) for b in data.batches) == 6
    assert any((row != tp.pad_token_id()).sum() > 1 for b in data.batches for row in b["proposal"])
    assert set(prop.tolist()) - {tp.pad_token_id()} <= {t for v in lex.values() for t in v}
