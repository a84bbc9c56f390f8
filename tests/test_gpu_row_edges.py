"""The training-side row kernels (loss.hip, optim.hip, rowops.hip) at the sizes where their strided loops take a second trip,
their vector tails begin and their dispatch changes kernel -- tests/test_gpu_ops.py runs each of them at one convenient
shape.  References are the fp64 restatements of tests/rowops_oracle.py; comparisons are ELEMENT-WISE against bounds scaled
by the magnitude of the terms an element is made of ("Row-kernel edge tests", lists case -> path -> measured
error / bound).  Every output is allocated with one extra row (four extra elements for vectors) and, where the leading
dimension exceeds the width, its pad columns, filled with a sentinel that must come back bit-unchanged: a tail that stores
a whole vector, or a wave that runs past the last row, shows there.

Each check prints ``ROWEDGE <case> <what> <worst error / bound>`` before it asserts (pytest -s shows the figures)."""
import functools

import pytest
import torch

from tests import rowops_oracle as RO

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
SENT = -7777.0   # finite, and nothing below computes it
BF16_ULP = 2.0 ** -7


def _ops():
    from imagetranslate_amd import hip_ops as O
    from imagetranslate_amd import _lib as L
    return O, L, L.load()


def _name(dtype):
    return "f32" if dtype == F32 else "bf16"


# ------------------------------------------------------------------------------------------------ guards and bounds
class Guarded:
    """[rows, width] view of a [rows + 1, ld] buffer (or [n] of [n + 4]) filled with SENT; ``check`` asserts that everything
    outside the view still holds it."""

    def __init__(self, rows, width, dtype, dev, ld=None):
        self.rows, self.width = rows, width
        if width is None:
            self.full = torch.full((rows + 4,), SENT, dtype=dtype, device=dev)
            self.view = self.full[:rows]
        else:
            self.ld = ld if ld is not None else (width + 7) // 8 * 8
            self.full = torch.full((rows + 1, self.ld), SENT, dtype=dtype, device=dev)
            self.view = self.full[:rows, :width]

    def check(self, what):
        f = self.full.float().cpu()
        s = float(torch.tensor(SENT, dtype=self.full.dtype).float())
        if self.width is None:
            assert bool((f[self.rows:] == s).all()), "%s: wrote past the last element" % what
        else:
            assert bool((f[self.rows:] == s).all()), "%s: wrote past the last row" % what
            assert bool((f[:self.rows, self.width:] == s).all()), "%s: wrote into the pad columns" % what


def _within(got, ref, bound, what):
    """|got - ref| <= bound element-wise (bound 0: exactly equal); prints and returns the worst error / bound."""
    got = got.detach().double().cpu()
    ref, bound = ref.double().expand_as(got), bound.double().expand_as(got)
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), "%s has non-finite values" % what
    err = (got - ref).abs()
    zero = bound == 0
    worst = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
    print("ROWEDGE %s %.3f" % (what, worst))
    assert bool((err[zero] == 0).all()), "%s: nonzero where the reference is exactly zero" % what
    assert worst <= 1.0, "%s: worst error / bound %.3f at flat index %d" % (what, worst, int((err / bound.clamp_min(1e-300)).argmax()))
    return worst


def _rowmax(t):
    return t.double().abs().max(dim=-1, keepdim=True).values


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------------------------ loss
N_LOSS, EPS, IGNORE, GS = 9, 0.1, 0, 1.0 / 9
# (dtype, V, leading dimension or None = the trainer's alloc_rows rule)
LOSS_CASES = [(F32, 3, None), (F32, 1030, None), (F32, 4099, None),
              (BF16, 7, None), (BF16, 2050, None), (BF16, 4099, None), (BF16, 16405, None), (BF16, 65536, None),
              (BF16, 65541, None), (BF16, 4100, 4108)]
LOSS_IDS = ["%s-V%d%s" % (_name(t), V, "-ld%d" % ld if ld else "") for t, V, ld in LOSS_CASES]


@functools.lru_cache(maxsize=None)
def _loss_case(dtype, V, ld):
    """Inputs (CPU, rounded to dtype), the fp64 oracle and the fp32 tolerance of one loss case; shared and
    never modified."""
    g = torch.Generator().manual_seed(7000 + V)
    N = N_LOSS
    z = (torch.randn(N, V, generator=g) * 3).to(dtype)
    ldv = ld if ld is not None else (V + 7) // 8 * 8
    lds_kernel = dtype == BF16 and V <= 65536 and ldv % 8 == 0          # imt_xent_fused_fwd_bwd's dispatch, restated
    grp = 8 if lds_kernel else 4                                         # elements per vector access of the kernel reached
    t = torch.randint(1, V, (N,), generator=g)
    t[0], t[1], t[2] = V - 1, 1, 0
    if V >= grp:
        t[3] = V // grp * grp - grp
    if V >= 8:
        t[4] = V + 5
    loss, dl, mag = RO.xent(z, t, EPS, IGNORE, GS)
    lp, lse = RO.log_softmax(z)
    # the same formula in plain fp32 torch on the CPU: what fp32 evaluation costs, measured rather than guessed
    zf = z.float()
    mx = zf.max(-1, keepdim=True).values
    lse32 = mx + (zf - mx).exp().sum(-1, keepdim=True).log()
    oh = torch.zeros(N, V)
    for r in range(N):
        if 0 <= int(t[r]) < V:
            oh[r, int(t[r])] = 1.0
    d32 = GS * ((zf - lse32).exp() - EPS / V - (1.0 - EPS) * oh) * (t != IGNORE).float().unsqueeze(-1)
    nz = mag > 0
    cpu_worst = float(((d32.double() - dl).abs()[nz] / mag[nz]).max())
    tol = min(16.0 * cpu_worst, 1e-4)
    print("ROWEDGE loss-%s-V%d fp32-cpu-worst %.3e tol %.3e" % (_name(dtype), V, cpu_worst, tol))
    return dict(z=z, t=t, loss=loss, dl=dl, mag=mag, lp=lp, lse=lse, tol=tol, ld=ldv, lds_kernel=lds_kernel)


def _logits_buffer(c, dtype, V, ld, dev):
    O, _, _ = _ops()
    buf = Guarded(N_LOSS, V, dtype, dev, ld)
    if ld is None:
        assert buf.view.stride(0) == max(O.alloc_rows(N_LOSS, V, dtype, dev).stride(0), V)   # the trainer's layout
    buf.view.copy_(c["z"])
    return buf


def _dl_bound(c, ref, mag, out_dtype):
    b = c["tol"] * mag
    return b + BF16_ULP * ref.abs() if out_dtype == BF16 else b


def _lsm_fwd(zv, dev):
    O, L, lib = _ops()
    N, V = zv.shape
    lp, lse = Guarded(N, V, F32, dev), Guarded(N, None, F32, dev)
    L.check(lib.imt_log_softmax_fwd(O.dt(zv), O._p(zv), zv.stride(0), O._p(lp.view), lp.view.stride(0), O._p(lse.view), N, V,
                                    O._stream()), "imt_log_softmax_fwd")
    return lp, lse


def _xent(zv, tgt, dev):
    O, L, lib = _ops()
    N, V = zv.shape
    rows = Guarded(N, None, F32, dev)
    L.check(lib.imt_xent_fused_fwd_bwd(O.dt(zv), O._p(zv), zv.stride(0), O._p(tgt), O._p(rows.view), N, V, EPS, IGNORE, GS,
                                       O._stream()), "imt_xent_fused_fwd_bwd")
    return rows


@pytest.mark.parametrize("dtype,V,ld", LOSS_CASES, ids=LOSS_IDS)
def test_xent_fused(cuda, dtype, V, ld):
    c = _loss_case(dtype, V, ld)
    tag = "xent-%s-V%d%s" % (_name(dtype), V, "-ld%d" % ld if ld else "")
    buf = _logits_buffer(c, dtype, V, ld, cuda)
    rows = _xent(buf.view, c["t"].to(cuda), cuda)
    buf.check(tag + " dlogits")
    rows.check(tag + " loss rows")
    _within(rows.view, c["loss"], (1e-5 if dtype == F32 else 1e-4) * c["loss"].abs(), tag + " loss")
    got = buf.view.double().cpu()
    _within(got, c["dl"], _dl_bound(c, c["dl"], c["mag"], dtype), tag + " dlogits")
    if dtype == F32:
        in_range = [r for r in range(N_LOSS) if r != 2 and 0 <= int(c["t"][r]) < V]
        sums = got[in_range].sum(-1)
        _within(sums, torch.zeros_like(sums), torch.full_like(sums, c["tol"] * GS), tag + " row-sums")
    if int(c["t"][4]) >= V:   # out of range and not ignored: a probability row shifted by eps / V, no (1 - eps) entry anywhere
        assert float(got[4].min()) > -0.5 * GS * (1.0 - EPS) and float(c["loss"][4]) > 0.0


@pytest.mark.parametrize("dtype,V,ld", LOSS_CASES, ids=LOSS_IDS)
def test_log_softmax_fwd(cuda, dtype, V, ld):
    c = _loss_case(dtype, V, ld)
    tag = "lsm-%s-V%d%s" % (_name(dtype), V, "-ld%d" % ld if ld else "")
    buf = _logits_buffer(c, dtype, V, ld, cuda)
    before = buf.full.clone()
    lp, lse = _lsm_fwd(buf.view, cuda)
    assert _bits_equal(buf.full, before), "the logits are an input here"
    lp.check(tag + " lp")
    lse.check(tag + " lse")
    scale = 1e-5 * _rowmax(c["lp"])
    _within(lp.view, c["lp"], scale, tag + " lp")
    _within(lse.view, c["lse"], scale.squeeze(-1), tag + " lse")


@pytest.mark.parametrize("V,out_dtype", [(3, F32), (1030, F32), (4099, F32), (1030, BF16), (4099, BF16)],
                         ids=["V3", "V1030", "V4099", "V1030-bf16out", "V4099-bf16out"])
def test_two_kernel_loss_path(cuda, V, out_dtype):
    """log_softmax_fwd -> smoothed_nll_fwd / smoothed_nll_bwd -> log_softmax_bwd on fp32 logits."""
    O, L, lib = _ops()
    c = _loss_case(F32, V, None)
    N = N_LOSS
    tag = "2k-V%d-%s" % (V, _name(out_dtype))
    buf = _logits_buffer(c, F32, V, None, cuda)
    tgt = c["t"].to(cuda)
    lp, _ = _lsm_fwd(buf.view, cuda)
    loss = Guarded(N, None, F32, cuda)
    L.check(lib.imt_smoothed_nll_fwd(O._p(lp.view), lp.view.stride(0), O._p(tgt), O._p(loss.view), N, V, EPS, IGNORE, O._stream()),
            "imt_smoothed_nll_fwd")
    loss.check(tag + " loss")
    _within(loss.view, c["loss"], 1e-5 * c["loss"].abs(), tag + " loss")
    # row 4 (target out of range where V allows one): the fused kernel reports the same loss
    fused = _xent(_logits_buffer(c, F32, V, None, cuda).view, tgt, cuda)
    _within(fused.view[4:5], loss.view[4:5].double().cpu(), 2e-5 * c["loss"][4:5].abs(), tag + " row4 fused-vs-2k loss")
    dloss = torch.full((N,), GS, device=cuda)
    dlp = Guarded(N, V, F32, cuda)
    L.check(lib.imt_smoothed_nll_bwd(O._p(dloss), O._p(tgt), O._p(dlp.view), dlp.view.stride(0), N, V, EPS, IGNORE, O._stream()),
            "imt_smoothed_nll_bwd")
    dlp.check(tag + " dlp")
    dlp_ref = RO.smoothed_nll_bwd(dloss.cpu(), c["t"], V, EPS, IGNORE)
    _within(dlp.view, dlp_ref, 1e-6 * dlp_ref.abs(), tag + " dlp")
    dz = Guarded(N, V, out_dtype, cuda)
    L.check(lib.imt_log_softmax_bwd(O._p(dlp.view), dlp.view.stride(0), O._p(lp.view), lp.view.stride(0), O.dt(dz.view), O._p(dz.view),
                                    dz.view.stride(0), N, V, O._stream()), "imt_log_softmax_bwd")
    dz.check(tag + " dlogits")
    dz_ref, mag = RO.log_softmax_bwd(dlp_ref, c["lp"])
    _within(dz.view, dz_ref, _dl_bound(c, dz_ref, mag, out_dtype), tag + " dlogits")
    rest = [r for r in range(N) if 0 <= int(c["t"][r]) < V]   # in-range rows: the two paths state the same gradient
    assert float((dz_ref[rest] - c["dl"][rest]).abs().max()) <= 1e-7 * GS   # (dloss holds fp32(1 / 9))


@pytest.mark.parametrize("n", [0, 63, 1025, 5000])
def test_scaled_sum(cuda, n):
    O, L, lib = _ops()
    g = torch.Generator().manual_seed(n)
    x = torch.randn(max(n, 1), generator=g)
    xd = x.to(cuda)
    outs = []
    for _ in range(2):
        out = Guarded(1, None, F32, cuda)
        L.check(lib.imt_scaled_sum(O._p(xd), n, 0.37, O._p(out.view), O._stream()), "imt_scaled_sum")
        out.check("scaled_sum n=%d" % n)
        outs.append(out.view.clone())
    assert _bits_equal(outs[0], outs[1]), "two calls on the same input differ"
    xs = x[:n].double()
    _within(outs[0], (0.37 * xs.sum()).view(1), (1e-6 * 0.37 * xs.abs().sum()).view(1), "scaled_sum-n%d" % n)
    assert _bits_equal(O.scaled_sum(xd[:n], 0.37).view(1), outs[0])   # the wrapper too; n = 0: an empty tensor (no address)


# ------------------------------------------------------------------------------------------------ optimizer
N_ARENA = 2048 * 2048 + 3
IDLE = slice(8192, 16384)
LONE = 100000   # the group of four [LONE, LONE + 4) has one nonzero gradient, at LONE + 1


@pytest.fixture(scope="module")
def arena():
    g = torch.Generator().manual_seed(11)
    sign = torch.randint(0, 2, (N_ARENA,), generator=g).float() * 2 - 1
    p0 = sign * (0.5 + torch.rand(N_ARENA, generator=g))   # away from zero: a bound relative to |p| means something everywhere
    return dict(p0=p0)


def _gradient(gen, sigma):
    grad = torch.randn(N_ARENA, generator=gen) * sigma
    grad[IDLE] = 0.0
    grad[LONE:LONE + 4] = torch.tensor([0.0, 0.75 * sigma, 0.0, 0.0])
    return grad


def test_sumsq(cuda, arena):
    O, _, _ = _ops()
    grad = _gradient(torch.Generator().manual_seed(12), 1.0)
    gd = torch.zeros(N_ARENA + 4, device=cuda)[:N_ARENA]
    gd.copy_(grad)
    for n in (N_ARENA, 1, 3, 4, 4097):
        ref = (grad[:n].double() ** 2).sum().view(1)
        outs = []
        for _ in range(2):
            out = Guarded(1, None, F32, cuda)
            out.view.zero_()
            O.sumsq(gd[:n], out.view)
            out.check("sumsq n=%d" % n)
            outs.append(out.view.clone())
        assert _bits_equal(outs[0], outs[1]), "sumsq n=%d: two calls on the same input differ" % n
        _within(outs[0], ref, 1e-5 * ref, "sumsq-n%d" % n)
        O.sumsq(gd[:n], out.view)   # no zeroing in between: the sum is ADDED to what `out` holds
        assert _bits_equal(out.view, outs[0] * 2), "sumsq n=%d: a second call into the same out must double it" % n


def test_clip_adam(cuda, arena):
    O, _, _ = _ops()
    n, lr, b1, b2, eps, gs = N_ARENA, 1e-3, 0.9, 0.98, 1e-8, 1.0 / 128
    gen = torch.Generator().manual_seed(13)
    bufs = {k: Guarded(n, None, F32, cuda) for k in "pgmv"}
    pb = Guarded(n, None, BF16, cuda)
    p, g, m, v = (bufs[k].view for k in "pgmv")
    p.copy_(arena["p0"])
    m.zero_()
    v.zero_()
    pb.view.fill_(SENT)
    p0_dev = p.clone()
    rp, rm, rv = arena["p0"].double(), torch.zeros(n).double(), torch.zeros(n).double()
    clipped = []
    # (step, gradient sigma, max_norm, zero_grad): the norm of the scaled gradient is 16 sigma
    for step, sigma, max_norm, zero_grad in ((1, 5.0, 1.0, True), (2, 0.001, 1.0, True), (10000, 5.0, 1.0, False), (10001, 5.0, 0.0, True)):
        tag = "adam-step%d" % step
        grad = _gradient(gen, sigma)
        g.copy_(grad)
        ss = torch.zeros(1, device=cuda)
        if max_norm > 0:
            O.sumsq(g, ss)
        else:
            ss.fill_(1e30)   # must be ignored
        ssv = float(ss.cpu())
        clipped.append(RO.clip_coef(ssv, max_norm, gs) < gs)
        # p is followed in fp64 over all steps; the moments are checked one step at a time from the state the kernel was
        # given (0.9 m + 0.1 g cancels, so an error inherited from an earlier step has no bound in THIS step's magnitudes)
        m_old, v_old = m.cpu().double(), v.cpu().double()
        rp, rm, rv = RO.adam_step(rp, grad, rm, rv, ssv, max_norm, gs, lr, b1, b2, eps, step)
        _, m_one, v_one = RO.adam_step(rp, grad, m_old, v_old, ssv, max_norm, gs, lr, b1, b2, eps, step)
        O.clip_adam(p, g, m, v, pb.view, ss, max_norm, gs, lr, b1, b2, eps, step, zero_grad=zero_grad)
        for k in "pgmv":
            bufs[k].check(tag + " " + k)
        pb.check(tag + " shadow")
        pc, mc, vc = p.cpu(), m.cpu(), v.cpu()
        _within(pc, rp, 1e-5 * rp.abs(), tag + " p")
        g_eff = grad.double().abs() * RO.clip_coef(ssv, max_norm, gs)
        _within(mc, m_one, 1e-5 * (b1 * m_old.abs() + (1 - b1) * g_eff), tag + " m")
        _within(vc, v_one, 1e-5 * v_one, tag + " v")
        # a group of four with one live gradient is updated as a whole
        _within(pc[LONE:LONE + 4], rp[LONE:LONE + 4], 1e-5 * rp[LONE:LONE + 4].abs(), tag + " p lone group")
        assert float(mc[LONE + 1]) != 0.0 and float(mc[LONE].abs() + mc[LONE + 2].abs() + mc[LONE + 3].abs()) == 0.0
        # idle groups (g = m = v = 0) are not written at all: not even the shadow is refreshed
        assert _bits_equal(p[IDLE], p0_dev[IDLE]) and float(m[IDLE].abs().max()) == 0.0 and float(v[IDLE].abs().max()) == 0.0
        shadow, want = pb.view.cpu(), pc.bfloat16()
        assert bool((shadow[IDLE].float() == float(torch.tensor(SENT).bfloat16())).all()), tag + ": idle groups must leave the shadow alone"
        want[IDLE] = shadow[IDLE]
        assert _bits_equal(shadow, want), tag + ": shadow != bf16(p)"
        if zero_grad:
            assert float(g.abs().max()) == 0.0 and float(g[-3:].abs().max()) == 0.0, tag + ": gradients not zeroed"
        else:
            assert _bits_equal(g.cpu(), grad), tag + ": zero_grad=False must leave the gradients alone"
    assert clipped == [True, False, True, False]


@pytest.mark.parametrize("n", [3, 4099, 20483])
def test_clip_scale(cuda, n):
    O, _, _ = _ops()
    gen = torch.Generator().manual_seed(n)
    grad = torch.randn(n, generator=gen)
    norm_sq = (grad.double() ** 2).sum().float().view(1)
    # (max_norm, grad_scale): above the norm -> clipped; below it with a scale -> scaled only; below it, scale 1 -> untouched
    big = 4.0 * float(norm_sq) ** 0.5
    for max_norm, gs in ((0.5 * float(norm_sq) ** 0.5, 1.0), (big, 0.5), (big, 1.0), (0.0, 0.5)):
        buf = Guarded(n, None, F32, cuda)
        buf.view.copy_(grad)
        O.clip_scale(buf.view, norm_sq.to(cuda), max_norm, gs)
        buf.check("clip_scale n=%d" % n)
        coef = RO.clip_coef(float(norm_sq), max_norm, gs)
        if gs == 1.0 and max_norm == big:
            assert coef == 1.0 and _bits_equal(buf.view.cpu(), grad), "coef == 1 must leave the gradients alone"
        else:
            assert coef != 1.0
            ref = grad.double() * coef
            _within(buf.view, ref, 1e-6 * ref.abs(), "clip_scale-n%d-max%.3g-gs%g" % (n, max_norm, gs))


def test_cast_f32_to_bf16_over_the_arena(cuda, arena):
    O, _, _ = _ops()
    src = arena["p0"] * 3.0
    dst = Guarded(N_ARENA, None, BF16, cuda)
    O.cast_f32_to_bf16(src.to(cuda), dst.view)
    dst.check("cast")
    assert _bits_equal(dst.view.cpu(), src.bfloat16())


# ------------------------------------------------------------------------------------------------ embeddings
EV, EP, ENT, EPAD, ES = 50, 16, 6, 0, 7
EMB_CASES = ["posmajor", "explicit_pos", "implicit_ragged", "no_types", "one_id", "third_pad"]


def _embed_ids(case, g):
    n = 147 if case in ("posmajor", "no_types", "third_pad") else 150   # 21 sentences of 7 | 150 % 7 != 0
    ids = torch.randint(0, EV, (n,), generator=g)
    if case == "one_id":
        ids.fill_(17)
    if case == "third_pad":
        ids[::3] = EPAD
    pos = torch.randint(0, EP, (n,), generator=g) if case == "explicit_pos" else None
    types = None if case == "no_types" else torch.randint(0, ENT, (n,), generator=g)
    return n, ids, pos, types


@pytest.mark.parametrize("case", EMB_CASES)
@pytest.mark.parametrize("d", [260, 512])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_embed_bwd(cuda, dtype, d, case):
    O, _, _ = _ops()
    g = torch.Generator().manual_seed(21)
    n, ids, pos, types = _embed_ids(case, g)
    dsum = torch.randn(n, d, generator=g).to(dtype)
    tabs = [Guarded(r, d, F32, cuda, ld=d) for r in (EV, EP, ENT)]
    init = [torch.randn(r, d, generator=g) for r in (EV, EP, ENT)]   # accumulation: the tables do not start from zero
    for t, i in zip(tabs, init):
        t.view.copy_(i)
    dev = lambda t: None if t is None else t.to(cuda)  # noqa: E731
    O.embed_bwd(dev(ids), dev(pos), dev(types), dsum.to(cuda), tabs[0].view, tabs[1].view, tabs[2].view, ES, EPAD)
    pos_full = pos if pos is not None else torch.arange(n) % ES
    types_full = types if types is not None else torch.zeros(n, dtype=torch.long)
    refs = RO.embed_grads(ids, pos_full, types_full, dsum, EV, EP, ENT, EPAD)
    mags = RO.embed_grad_mags(ids, pos_full, types_full, dsum, EV, EP, ENT, EPAD)
    tag = "embed_bwd-%s-d%d-%s" % (_name(dtype), d, case)
    for name, t, i, r, mg in zip(("dword", "dpos", "dtype"), tabs, init, refs, mags):
        t.check(tag + " " + name)
        # the order of the fp32 atomics is free: every partial sum is bounded by the summed magnitudes, old value included
        _within(t.view, i.double() + r, 1e-5 * (i.double().abs() + mg), tag + " " + name)
    assert _bits_equal(tabs[0].view[EPAD].cpu(), init[0][EPAD]), "the pad row takes no gradient"


@pytest.mark.parametrize("d", [260, 512])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_embed_fwd_and_fused_embed_ln(cuda, dtype, d):
    O, L, lib = _ops()
    g = torch.Generator().manual_seed(22)
    n = 150
    word, pos, typ = (torch.randn(r, d, generator=g).to(dtype) for r in (EV, EP, ENT))
    gam, bet = torch.randn(d, generator=g).to(dtype), (torch.randn(d, generator=g) * 0.2).to(dtype)
    ids = torch.randint(0, EV, (n,), generator=g)
    ids[5], ids[77], ids[149] = -1, EV, EV + 1000   # the documented clamp: out-of-range ids read row 0
    types = torch.randint(0, ENT, (n,), generator=g)
    pids = torch.randint(0, EP, (n,), generator=g)
    W, Pt, T, G, Bt = (t.to(cuda) for t in (word, pos, typ, gam, bet))
    idd, tyd = ids.to(cuda), types.to(cuda)
    clamped = torch.where((ids < 0) | (ids >= EV), torch.zeros_like(ids), ids)
    tol = 1e-6 if dtype == F32 else 1e-2
    for pos_ids in (None, pids):
        tag = "embed_fwd-%s-d%d-%s" % (_name(dtype), d, "pos" if pos_ids is not None else "implicit")
        pd = None if pos_ids is None else pos_ids.to(cuda)
        pfull = pos_ids if pos_ids is not None else torch.arange(n) % ES
        out = Guarded(n, d, dtype, cuda, ld=d)
        L.check(lib.imt_embed_fwd(O.dt(W), O._p(idd), O._p(pd), O._p(tyd), O._p(W), O._p(Pt), O._p(T), O._p(out.view),
                                  n, ES, d, EV, EP, ENT, O._stream()), "imt_embed_fwd")
        out.check(tag)
        ref = word.double()[clamped] + pos.double()[pfull] + typ.double()[types]
        _within(out.view, ref, tol * _rowmax(ref), tag)
        again = O.embed_fwd(clamped.to(cuda), pd, tyd, W, Pt, T, ES)
        assert _bits_equal(again, out.view.contiguous())
        # the fused gather + LayerNorm against the two launches, bit for bit, clamped ids included
        y2, m2, r2 = O.layernorm_fwd(again, G, Bt)
        ssum, y = Guarded(n, d, dtype, cuda, ld=d), Guarded(n, d, dtype, cuda, ld=d)
        mean, rstd = Guarded(n, None, F32, cuda), Guarded(n, None, F32, cuda)
        L.check(lib.imt_embed_ln_fwd(O.dt(W), O._p(idd), O._p(pd), O._p(tyd), O._p(W), O._p(Pt), O._p(T), O._p(G), O._p(Bt),
                                     O._p(ssum.view), O._p(y.view), O._p(mean.view), O._p(rstd.view), n, ES, d, EV, EP, ENT, 1e-12, 0.0, 0,
                                     O._stream()), "imt_embed_ln_fwd")
        for b, what in ((ssum, "sum"), (y, "y"), (mean, "mean"), (rstd, "rstd")):
            b.check(tag + " embed_ln " + what)
        assert _bits_equal(ssum.view.contiguous(), again) and _bits_equal(y.view.contiguous(), y2)
        assert _bits_equal(mean.view.contiguous(), m2) and _bits_equal(rstd.view.contiguous(), r2)


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_EPS = 1e-12


def _ln_fwd(x, gamma, beta, dev, resid=None):
    O, L, lib = _ops()
    rows, d = x.shape
    y, mean, rstd = Guarded(rows, d, x.dtype, dev, ld=d), Guarded(rows, None, F32, dev), Guarded(rows, None, F32, dev)
    if resid is None:
        L.check(lib.imt_layernorm_fwd(O.dt(x), O._p(x), O._p(gamma), O._p(beta), O._p(y.view), O._p(mean.view), O._p(rstd.view), rows, d,
                                      LN_EPS, 0.0, 0, O._stream()), "imt_layernorm_fwd")
        return y, mean, rstd
    ssum = Guarded(rows, d, x.dtype, dev, ld=d)
    L.check(lib.imt_add_layernorm_fwd(O.dt(x), O._p(x), O._p(resid), O._p(gamma), O._p(beta), O._p(ssum.view), O._p(y.view), O._p(mean.view),
                                      O._p(rstd.view), rows, d, LN_EPS, 0.0, 0, O._stream()), "imt_add_layernorm_fwd")
    return y, mean, rstd, ssum


@pytest.mark.parametrize("rows,d,partial", [(1, 4, False), (3, 260, False), (5, 516, False), (333, 1024, False), (8300, 128, False),
                                            (8300, 128, True)],
                         ids=["1x4", "3x260", "5x516", "333x1024", "8300x128", "8300x128-partial"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_layernorm_fwd_bwd(cuda, dtype, rows, d, partial):
    O, L, lib = _ops()
    g = torch.Generator().manual_seed(31)
    x = (torch.randn(rows, d, generator=g) * 2 + 0.5).to(dtype)
    gamma, beta = torch.randn(d, generator=g).to(dtype), torch.randn(d, generator=g).to(dtype)
    dy = torch.randn(rows, d, generator=g).to(dtype)
    y_ref, mean_ref, rstd_ref, dx_ref, dg_ref, db_ref = RO.layernorm_fwd_bwd(x, gamma, beta, dy, LN_EPS)
    tag = "ln-%s-%dx%d%s" % (_name(dtype), rows, d, "-partial" if partial else "")
    X, G, Bt, DY = (t.to(cuda) for t in (x, gamma, beta, dy))
    y, mean, rstd = _ln_fwd(X, G, Bt, cuda)
    for b, what in ((y, "y"), (mean, "mean"), (rstd, "rstd")):
        b.check(tag + " " + what)
    y_bound, mean_bound, rstd_bound = RO.layernorm_bounds(x, y_ref, rstd_ref, dtype)   # shared with test_gpu_dense_ln_edges.py
    _within(y.view, y_ref, y_bound, tag + " y")
    _within(mean.view, mean_ref, mean_bound, tag + " mean")
    _within(rstd.view, rstd_ref, rstd_bound, tag + " rstd")
    grads = Guarded(2 * d, None, F32, cuda)
    init = torch.randn(2 * d, generator=g)
    grads.view.copy_(init)
    dx = Guarded(rows, d, dtype, cuda, ld=d)
    ws = torch.zeros(O.LN_PARTIAL_COPIES, 2, d, device=cuda) if partial else None
    mean_c, rstd_c = mean.view.contiguous(), rstd.view.contiguous()
    L.check(lib.imt_layernorm_bwd(O.dt(X), O._p(DY), O._p(X), O._p(G), O._p(mean_c), O._p(rstd_c), O._p(dx.view), O._p(grads.view[:d]),
                                  O._p(grads.view[d:]), rows, d, 0.0, 0, None, 0.0, 0, O._p(ws), O._stream()), "imt_layernorm_bwd")
    dx.check(tag + " dx")
    _within(dx.view, dx_ref, RO.layernorm_dx_bound(dx_ref, dtype), tag + " dx")
    if partial:
        assert _bits_equal(grads.view.cpu(), init), "with a workspace the gradients are untouched until the reduce"
        O.ln_partial_reduce(ws.view(1, O.LN_PARTIAL_COPIES, 2, d), grads.view, [0], [d])
    grads.check(tag + " dgamma/dbeta")
    mg, mb = RO.layernorm_param_grad_mags(x, dy, LN_EPS)
    ptol = 1e-4 if dtype == F32 else 1e-2
    i64 = init.double()
    _within(grads.view[:d], i64[:d] + dg_ref, ptol * (i64[:d].abs() + mg), tag + " dgamma")
    _within(grads.view[d:], i64[d:] + db_ref, ptol * (i64[d:].abs() + mb), tag + " dbeta")


@pytest.mark.parametrize("rows,d", [(5, 516), (3, 1024)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_add_layernorm_fwd(cuda, dtype, rows, d):
    g = torch.Generator().manual_seed(32)
    x, res = (torch.randn(rows, d, generator=g).to(dtype).to(cuda) for _ in range(2))
    gam, bet = (torch.randn(d, generator=g).to(dtype).to(cuda) for _ in range(2))
    y, mean, rstd, ssum = _ln_fwd(x, gam, bet, cuda, resid=res)
    tag = "add_ln-%s-%dx%d" % (_name(dtype), rows, d)
    for b, what in ((y, "y"), (mean, "mean"), (rstd, "rstd"), (ssum, "sum")):
        b.check(tag + " " + what)
    s2 = (x.float() + res.float()).to(dtype)
    y2, m2, r2 = _ln_fwd(s2, gam, bet, cuda)
    assert _bits_equal(ssum.view.contiguous(), s2) and _bits_equal(y.view, y2.view)
    assert _bits_equal(mean.view, m2.view) and _bits_equal(rstd.view, r2.view)


# ------------------------------------------------------------------------------------------------ column sums and friends
@pytest.mark.parametrize("M,scale", [(65, None), (1, None), (65, 0.25)], ids=["65rows", "1row", "scaled"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_colsum_scalar_columns(cuda, dtype, M, scale):
    O, _, _ = _ops()
    g = torch.Generator().manual_seed(41)
    Ncol = 263   # the last group of four columns is cut: the scalar path
    X = torch.randn(M, 264, generator=g).to(dtype)
    init = torch.randn(Ncol, generator=g)
    out = Guarded(Ncol, None, F32, cuda)
    out.view.copy_(init)   # colsum ADDS to out
    sd = None if scale is None else torch.tensor([scale], device=cuda)
    O.colsum(X.to(cuda)[:, :Ncol], out.view, sd)
    out.check("colsum")
    s = 1.0 if scale is None else scale
    xs = X.double()[:, :Ncol]
    _within(out.view, init.double() + s * xs.sum(0), 1e-5 * (init.double().abs() + s * xs.abs().sum(0)),
            "colsum-%s-M%d%s" % (_name(dtype), M, "-scaled" if scale else ""))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_gather_scatter_rows_strided(cuda, dtype):
    O, L, lib = _ops()
    g = torch.Generator().manual_seed(42)
    rows, d, ld = 40, 260, 264
    src = torch.randn(rows, ld, generator=g).to(dtype)
    xv = src.to(cuda)[:, :d]
    idx = torch.randperm(rows, generator=g)[:13].sort().values.int()
    sel = Guarded(13, d, dtype, cuda, ld=ld)
    idd = idx.to(cuda)
    L.check(lib.imt_gather_rows(O.dt(xv), O._p(xv), xv.stride(0), O._p(idd), O._p(sel.view), ld, 13, d, O._stream()), "imt_gather_rows")
    sel.check("gather_rows")
    assert _bits_equal(sel.view.cpu().contiguous(), src[idx.long(), :d].contiguous())
    assert _bits_equal(O.gather_rows(xv, idd).cpu(), src[idx.long(), :d].contiguous())
    old = torch.randn(rows, ld, generator=g).to(dtype)
    dst = Guarded(rows, d, dtype, cuda, ld=ld)
    dst.view.copy_(old[:, :d])
    O.scatter_rows(sel.view, idd, dst.view)
    dst.check("scatter_rows")
    want = old[:, :d].clone()
    want[idx.long()] = src[idx.long(), :d]
    assert _bits_equal(dst.view.cpu().contiguous(), want.contiguous()), "scatter_rows: wrong rows, or rows outside idx touched"


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_gated_mix_wrapping_columns(cuda, dtype):
    O, L, lib = _ops()
    g = torch.Generator().manual_seed(43)
    rows, d = 5, 260
    a, b = (torch.randn(rows, d, generator=g).to(dtype) for _ in range(2))
    gate = torch.randn(d, generator=g).to(dtype)
    out = Guarded(rows, d, dtype, cuda, ld=d)
    A, B, Gt = a.to(cuda), b.to(cuda), gate.to(cuda)
    L.check(lib.imt_gated_mix(O.dt(A), O._p(A), O._p(B), O._p(Gt), O._p(out.view), rows, d, O._stream()), "imt_gated_mix")
    out.check("gated_mix")
    s = torch.sigmoid(gate.double() + 1e-7)
    ref = s * a.double() + (1 - s) * b.double()
    _within(out.view, ref, (1e-5 if dtype == F32 else 1e-2) * _rowmax(ref), "gated_mix-%s" % _name(dtype))
