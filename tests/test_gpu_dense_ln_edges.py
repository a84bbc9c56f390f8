"""y = LayerNorm(dropout(x W^T + b) + resid) on its three launch paths against the fp64 restatement of tests/dense_ln_oracle.py:

  A  imt_gemm_bias_residual_ln (csrc/gemm_ln.hip): the four instances of gemm_ln_kernel where the LDS-DMA ring is shorter than
     its prologue, exactly full, first refilled and reused twice, where the K-order rotation wraps, and where the last row tile
     has one live row;
  B  imt_gemm(..., ln_out=...) (csrc/gemm.hip): splitk_epilogue_ln_kernel at every NCH with clamped lanes and M % 4 tails, and
     the LayerNorm launch behind the single launch, the ragged-K pair and the unfused split-K epilogue; check_ln_out's refusals;
  C  the three paths on one data set, and imt_layernorm_bwd fed with what each of them saved.

tests/test_gpu_ops.py compares path A with path B's kernels on Gaussian data by max|a-b| / max|b| and path B's output with
F.layer_norm of its own pre-LN rows.  Here, per case (the lists with a comment per case are in dense_ln_oracle.py):

  * operands are integers plus an asymmetric ramp, bias / residual integers, p = 0.5, alpha a power of two: the stored pre-LN
    value must equal the oracle BIT FOR BIT (bf16: the oracle rounded once) in whatever order K is summed;
  * y, mean, rstd are within the bounds of test_gpu_row_edges.py::test_layernorm_fwd_bwd (rowops_oracle.layernorm_bounds) of
    the fp64 LayerNorm of that rounded value;
  * the keep mask is imt_add_rows_dropout's on ones (the (seed, m * N + n) convention test_gpu_gemm_edges.py pins), never a
    restatement of the generator;
  * x, W, bias, residual, gamma, beta, pre_ln, out, mean and rstd are views inside buffers filled with a NaN bit pattern, every
    leading dimension of path A wider than its extent: inputs come back bit-unchanged, nothing outside the outputs is written,
    no NaN reaches a result, and a second launch into fresh outputs gives the same bits;
  * the profiler kinds are the ones the case is there for.

Each case prints ``DENSELN <id> <kinds> pre=<bit-equal | worst error / bound> y=<worst error / bound> mean=.. rstd=..`` before
it asserts (pytest -s; DESIGN.md, "Dense + LayerNorm edge tests", records the figures)."""
import ctypes

import pytest
import torch

from tests import dense_ln_oracle as DO
from tests import gemm_oracle as GO
from tests import rowops_oracle as RO

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def _ops():
    from imagetranslate_amd import hip_ops as O
    from imagetranslate_amd import _lib as L
    return O, L, L.load()


def _kinds_of(fn):
    """Kernel kinds (imt_prof_report rows) launched by fn(), as {kind: launches}."""
    _, L, lib = _ops()
    torch.cuda.synchronize()
    lib.imt_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        rows = (L.ProfRow * 64)()
        n = lib.imt_prof_report(rows, 64)
    finally:
        lib.imt_prof_enable(0)
    return {rows[i].kind.decode(): int(rows[i].launches) for i in range(n)}


def _want(kinds):
    want = {}
    for k in kinds:
        want[k] = want.get(k, 0) + 1
    return want


_KEEP = {}


def _keep(dev, M, N):
    """The keep mask [M, N] (bool, CPU) of p = 0.5 under DO.SEED: what imt_add_rows_dropout leaves of ones."""
    if (M, N) not in _KEEP:
        O, _, _ = _ops()
        rows = O.add_rows_dropout(torch.ones(M, N, device=dev, dtype=F32), None, dropout_p=DO.P_DROP, dropout_seed=DO.SEED)
        _KEEP[(M, N)] = (rows != 0).cpu()
    return _KEEP[(M, N)]


class _Inputs:
    """Guarded device copies of one data set (x, W, residual: leading dimensions wider than the extents)."""

    def __init__(self, d, dtype, M, N, K, dev):
        T = DO.DT[dtype]
        self.x = GO.Guard(M, K, T, dev).put(d["x"])
        self.W = GO.Guard(N, K, T, dev).put(d["W"])
        self.resid = GO.Guard(M, N, T, dev).put(d["resid"])
        self.bias = GO.GuardVec(N, T, dev).put(d["bias"])
        self.gamma = GO.GuardVec(N, T, dev).put(d["gamma"])
        self.beta = GO.GuardVec(N, T, dev).put(d["beta"])

    def check(self, what):
        for name in ("x", "W", "resid", "bias", "gamma", "beta"):
            getattr(self, name).check_all("%s: %s" % (what, name))


def _untouched(g):
    return bool((g.bits == g.pattern).all())


def _ratios(y, mean, rstd, pre_rows, ref, T):
    """Worst error / bound of (y, mean, rstd) against the oracle ``ref`` of the rows ``pre_rows``."""
    yb, mb, rb = DO.bounds(pre_rows, ref, T)
    return DO.worst_ratio(y, ref["y"], yb), DO.worst_ratio(mean, ref["mean"], mb), DO.worst_ratio(rstd, ref["rstd"], rb)


# ================================================================================================ A: imt_gemm_bias_residual_ln
class _FusedOut:
    def __init__(self, M, N, T, dev):
        self.pre, self.out = GO.Guard(M, N, T, dev), GO.Guard(M, N, T, dev)   # pre_ln and out share ldo
        assert self.pre.ld == self.out.ld and self.out.ld > N
        self.mean, self.rstd = GO.GuardVec(M, F32, dev), GO.GuardVec(M, F32, dev)

    def all(self):
        return (("pre_ln", self.pre), ("out", self.out), ("mean", self.mean), ("rstd", self.rstd))


def _fused_rc(inp, o, M, N, K, epi, eps, *, want_pre=True, want_stats=True, p=None, ldo=None, x_ptr=None):
    """The return code of one imt_gemm_bias_residual_ln call into the outputs ``o``."""
    O, _, lib = _ops()
    b, drop, r = DO.EPILOGUES[epi]
    x = ctypes.c_void_p(x_ptr) if x_ptr is not None else O._p(inp.x.view)
    return lib.imt_gemm_bias_residual_ln(O.dt(inp.x.full), x, inp.x.ld, O._p(inp.W.view), inp.W.ld, O._p(inp.bias.view) if b else None,
                                         O._p(inp.resid.view) if r else None, inp.resid.ld if r else 0, O._p(inp.gamma.view), O._p(inp.beta.view),
                                         O._p(o.pre.view) if want_pre else None, O._p(o.out.view), o.out.ld if ldo is None else ldo,
                                         O._p(o.mean.view) if want_stats else None, O._p(o.rstd.view) if want_stats else None, M, N, K, eps,
                                         (DO.P_DROP if drop else 0.0) if p is None else p, DO.SEED, O._stream())


def _fused_launch(inp, M, N, K, T, epi, eps, dev, with_kinds, **kw):
    _, L, _ = _ops()
    o = _FusedOut(M, N, T, dev)

    def call():
        L.check(_fused_rc(inp, o, M, N, K, epi, eps, **kw), "imt_gemm_bias_residual_ln")

    kinds = None
    if with_kinds:
        kinds = _kinds_of(call)
    else:
        call()
        torch.cuda.synchronize()
    return o, kinds


def _fused_check(cid, case, epi, dev, *, want_pre=True, want_stats=True):
    """One fused launch (and a second one) held to the oracle; returns (figures, errors)."""
    T = DO.DT[case.dtype]
    M, N, K = case.M, case.N, case.nt * DO.bk(case.dtype)
    d = DO.inputs(case.dtype, M, N, K, case.data)
    keep = _keep(dev, M, N) if DO.uses_dropout(epi) else None
    ref = DO.reference(d["x"], d["W"], T, d["gamma"], d["beta"], case.eps, **DO.epilogue_terms(epi, d, keep))
    inp = _Inputs(d, case.dtype, M, N, K, dev)
    o, kinds = _fused_launch(inp, M, N, K, T, epi, case.eps, dev, True, want_pre=want_pre, want_stats=want_stats)
    errors = []
    if kinds != {"gemm_ln_%s" % case.dtype: 1}:
        errors.append("%s: launched %s" % (cid, sorted(kinds.items())))
    pre_rows, pre_fig = ref["pre"], "not-stored"
    if want_pre:
        got = o.pre.view.cpu()
        if case.data == "gauss":
            r_pre = DO.worst_ratio(got, ref["pre64"], DO.pre_bound(ref, T))
            pre_fig = "%.3f" % r_pre
            if not r_pre <= 1.0:
                errors.append("%s: pre-LN worst |got - ref| / bound = %g" % (cid, r_pre))
            pre_rows, ref = got, DO.layernorm(got, d["gamma"], d["beta"], case.eps)   # the statistics are those of the STORED rows
        else:
            same = GO.bits_equal(got, ref["pre"])
            pre_fig = "bit-equal" if same else "DIFFERS"
            if not same:
                bad = got.double() != ref["pre"].double()
                errors.append("%s: pre-LN is not the oracle's bits: %d of %d elements, NaN %d" % (cid, int(bad.sum()), bad.numel(), int(got.isnan().sum())))
    elif not _untouched(o.pre):
        errors.append("%s: pre_ln = NULL, and its buffer was written" % cid)
    if case.data == "gauss" and not want_pre:
        raise AssertionError("a real-valued case needs the stored rows")
    mean = o.mean.view if want_stats else ref["mean"]
    rstd = o.rstd.view if want_stats else ref["rstd"]
    ry, rm, rr = _ratios(o.out.view, mean, rstd, pre_rows, ref, T)
    if not max(ry, rm, rr) <= 1.0:
        errors.append("%s: worst error / bound y %g mean %g rstd %g" % (cid, ry, rm, rr))
    if not want_stats and not (_untouched(o.mean) and _untouched(o.rstd)):
        errors.append("%s: mean / rstd = NULL, and their buffers were written" % cid)
    if case.data == "degenerate":
        yc = o.out.view.cpu()
        for r in DO.DEGENERATE_ROWS:
            if not GO.bits_equal(yc[r], d["beta"].to(T)):
                errors.append("%s: row %d has a constant pre-LN value, y must be beta exactly" % (cid, r))
    o2, _ = _fused_launch(inp, M, N, K, T, epi, case.eps, dev, False, want_pre=want_pre, want_stats=want_stats)
    for (name, g1), (_, g2) in zip(o.all(), o2.all()):
        try:
            g1.check("%s: %s" % (cid, name))
        except AssertionError as err:
            errors.append(str(err))
        if not torch.equal(g1.bits, g2.bits):
            errors.append("%s: %s differs between two launches" % (cid, name))
    try:
        inp.check(cid)
    except AssertionError as err:
        errors.append(str(err))
    fig = "pre=%s y=%.3f mean=%s rstd=%s" % (pre_fig, ry, "%.3f" % rm if want_stats else "null", "%.3f" % rr if want_stats else "null")
    return sorted(kinds.items()), fig, errors


@pytest.mark.parametrize("case", DO.FUSED_CASES, ids=[c.id for c in DO.FUSED_CASES])
def test_fused_kernel_edges(cuda, case):
    kinds, fig, errors = _fused_check(case.id, case, case.epi, cuda)
    print("DENSELN %s %s %s" % (case.id, kinds, fig))
    assert not errors, "\n".join(errors[:12])


@pytest.mark.parametrize("case", DO.SWEEP_CASES, ids=[c.id for c in DO.SWEEP_CASES])
def test_fused_kernel_epilogue_sweep(cuda, case):
    """{none, bias, resid, bias + resid, bias + drop + resid, drop} x pre_ln {wanted, NULL} x mean / rstd {given, NULL}."""
    errors = []
    for epi in DO.EPILOGUES:
        for want_pre in (True, False):
            for want_stats in (True, False):
                cid = "%s/%s/%s/%s" % (case.id, epi, "pre" if want_pre else "nopre", "stats" if want_stats else "nostats")
                kinds, fig, errs = _fused_check(cid, case, epi, cuda, want_pre=want_pre, want_stats=want_stats)
                print("DENSELN %s %s %s" % (cid, kinds, fig))
                errors += errs
    assert not errors, "\n".join(errors[:12])


@pytest.mark.parametrize("N", list(DO.INSTANCES))
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_fused_kernel_mask_is_the_row_kernels(cuda, dtype, N):
    """The mask of gemm_ln_kernel, recovered from a launch whose pre-dropout value cannot be zero (x W^T is 1 or 2, bias -4:
    kept <=> pre != resid, bit-wise), is imt_add_rows_dropout's -- over 10 workgroups and every wave's columns."""
    T = DO.DT[dtype]
    M, K = 289, 2 * DO.bk(dtype)
    d = dict(DO.inputs(dtype, M, N, K))
    d["x"], d["W"] = torch.zeros(M, K), torch.zeros(N, K)
    d["x"][:, 0] = 1.0
    d["W"][:, 0] = 1.0 + (torch.arange(N) % 2).float()
    d["bias"] = torch.full((N,), -4.0)
    plain = DO.reference(d["x"], d["W"], T, d["gamma"], d["beta"], 1e-12, bias=d["bias"])
    assert float(plain["pre64"].abs().min()) >= 2.0 and float(plain["pre64"].abs().max()) <= 3.0
    inp = _Inputs(d, dtype, M, N, K, cuda)
    o, kinds = _fused_launch(inp, M, N, K, T, DO.BDR, 1e-12, cuda, True)
    assert kinds == {"gemm_ln_%s" % dtype: 1}, kinds
    itype = GO.NAN_BITS[T][0]
    dropped = (o.pre.view.contiguous().view(itype) == inp.resid.view.contiguous().view(itype)).cpu()
    keep = _keep(cuda, M, N)
    frac = float(dropped.float().mean())
    sigma = (0.25 / (M * N)) ** 0.5
    print("DENSELN mask_N%d_%s %s dropped %.4f (5 sigma = %.4f)" % (N, dtype, sorted(kinds.items()), frac, 5 * sigma))
    assert abs(frac - DO.P_DROP) <= 5 * sigma
    for m0 in range(0, M, 32):
        blk = dropped[m0:m0 + 32]
        assert bool(blk.any()) and bool((~blk).any()), "row block %d: kept and dropped elements must both exist" % (m0 // 32)
    assert torch.equal(~dropped, keep), "%d decisions differ from imt_add_rows_dropout" % int((~dropped != keep).sum())
    ref = DO.reference(d["x"], d["W"], T, d["gamma"], d["beta"], 1e-12, bias=d["bias"], keep=keep, resid=d["resid"])
    assert GO.bits_equal(o.pre.view.cpu(), ref["pre"]), "kept values are not 2 v + resid"


FUSED_REFUSALS = ["N640", "K_not_whole_tiles", "ldo_not_x4", "x_misaligned", "dropout_p_1", "M0"]


@pytest.mark.parametrize("why", FUSED_REFUSALS)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_fused_kernel_refusals(cuda, dtype, why):
    """Each refusal raises ImtError before any launch and leaves the outputs unwritten; M = 0 returns without a launch.  (One
    row throughout: nothing here can reach past a buffer even if a refusal were missing.)"""
    _, L, _ = _ops()
    T = DO.DT[dtype]
    M, N, K = 1, (640 if why == "N640" else 128), 2 * DO.bk(dtype)
    if why == "K_not_whole_tiles":
        K = DO.bk(dtype) - DO.al(dtype)   # whole 16-byte chunks, so only the tile rule can refuse it
    d = DO.inputs(dtype, M, N, K)
    inp = _Inputs(d, dtype, M, N, K, cuda)
    o = _FusedOut(M, N, T, cuda)
    kw = {}
    if why == "ldo_not_x4":
        kw["ldo"] = o.out.ld + 2
    if why == "x_misaligned":
        kw["x_ptr"] = inp.x.full.data_ptr() + inp.x.full.element_size()   # the guard rows in front of the view: inside the buffer
    if why == "dropout_p_1":
        kw["p"] = 1.0
    rcs = []
    kinds = _kinds_of(lambda: rcs.append(_fused_rc(inp, o, 0 if why == "M0" else M, N, K, DO.BDR, 1e-12, **kw)))
    print("DENSELN refusal_%s_%s rc %d %s" % (why, dtype, rcs[0], sorted(kinds.items())))
    assert kinds == {}, kinds
    if why == "M0":
        assert rcs[0] == 0
    else:
        with pytest.raises(L.ImtError):
            L.check(rcs[0], "imt_gemm_bias_residual_ln")
    for name, g in o.all():
        assert _untouched(g), "%s was written by a refused call" % name
    inp.check(why)


# ================================================================================================ B: imt_gemm(..., ln=...)
class _GemmOut:
    """C and ln_out as contiguous [M, N] rows (what the LayerNorm launch needs) inside guarded vectors."""

    def __init__(self, M, N, T, dev):
        self.C, self.y = GO.GuardVec(M * N, T, dev), GO.GuardVec(M * N, T, dev)
        self.mean, self.rstd = GO.GuardVec(M, F32, dev), GO.GuardVec(M, F32, dev)
        self.Cv, self.yv = self.C.view.view(M, N), self.y.view.view(M, N)
        self.aux = None

    def all(self):
        return (("C", self.C), ("ln_out", self.y), ("mean", self.mean), ("rstd", self.rstd)) + ((("aux", self.aux),) if self.aux is not None else ())


def _gemm_kwargs(case, inp, o, dev, ln):
    O, _, _ = _ops()
    T = DO.DT[case.dtype]
    kw = dict(out=o.Cv)
    if case.epi == "alpha":
        kw.update(alpha=DO.ALPHA, alpha_dev=torch.tensor([DO.ALPHA_DEV], device=dev, dtype=F32))
    elif case.epi == "bias_gelu":
        o.aux = GO.Guard(case.M, case.N, T, dev)
        kw.update(bias=inp.bias.view, aux=o.aux.view, aux_mode=O.IMT_AUX_GELU_FWD)
    else:
        b, drop, r = DO.EPILOGUES[case.epi]
        if b:
            kw["bias"] = inp.bias.view
        if drop:
            kw.update(dropout_p=DO.P_DROP, dropout_seed=DO.SEED)
        if r:
            kw["resid"] = inp.resid.view
    if case.ws:
        kw["splitk_ws"] = O.splitk_workspace(dev)
    if ln:
        kw["ln"] = dict(gamma=inp.gamma.view, beta=inp.beta.view, out=o.yv, mean=o.mean.view, rstd=o.rstd.view, eps=1e-12)
    return kw


def _gemm_launch(case, inp, dev, ln, with_kinds):
    """(outputs, kinds | None, error message | None)"""
    O, L, _ = _ops()
    o = _GemmOut(case.M, case.N, DO.DT[case.dtype], dev)
    kw = _gemm_kwargs(case, inp, o, dev, ln)
    failed = []

    def call():
        try:
            O.gemm(inp.x.view, inp.W.view, O.IMT_NT, **kw)
        except L.ImtError as e:
            failed.append(str(e))

    kinds = None
    if with_kinds:
        kinds = _kinds_of(call)
    else:
        call()
        torch.cuda.synchronize()
    return o, kinds, (failed[0] if failed else None)


@pytest.mark.parametrize("case", DO.GEMM_CASES, ids=[c.id for c in DO.GEMM_CASES])
def test_gemm_ln_edges(cuda, case):
    O, _, _ = _ops()
    T = DO.DT[case.dtype]
    M, N, K = case.M, case.N, case.K
    d = DO.inputs(case.dtype, M, N, K)
    inp = _Inputs(d, case.dtype, M, N, K, cuda)
    errors = []
    o, kinds, failed = _gemm_launch(case, inp, cuda, True, True)
    if kinds != _want(case.kinds):
        errors.append("launched %s, the case is there for %s" % (sorted(kinds.items()), case.kinds))
    if (failed is None) != (case.refused is None) or (failed is not None and case.refused not in failed):
        errors.append("the call %s; expected %s" % ("failed: " + failed if failed else "succeeded", case.refused or "success"))
    got = o.Cv.cpu()
    if case.epi == "bias_gelu":   # real-valued through erf: C within gemm_oracle.bound, aux the rounded pre-activation, LayerNorm of the kernel's own C
        gref = GO.reference(GO.NT, d["x"], d["W"], T, bias=d["bias"], aux_mode=GO.AUX_GELU_FWD)
        r_pre = DO.worst_ratio(got, gref["out"], GO.bound(gref, GO.AUX_GELU_FWD, T))
        pre_fig = "%.3f" % r_pre
        if not r_pre <= 1.0:
            errors.append("C worst |got - ref| / bound = %g" % r_pre)
        if not GO.bits_equal(o.aux.view.cpu(), gref["aux"]):
            errors.append("aux is not the rounded pre-activation")
        pre_rows, ref = got, DO.layernorm(got, d["gamma"], d["beta"], 1e-12)
    else:
        keep = _keep(cuda, M, N) if DO.uses_dropout(case.epi) else None
        ref = DO.reference(d["x"], d["W"], T, d["gamma"], d["beta"], 1e-12, **DO.epilogue_terms(case.epi, d, keep))
        same = GO.bits_equal(got, ref["pre"])
        pre_fig, pre_rows = ("bit-equal" if same else "DIFFERS"), ref["pre"]
        if not same:
            bad = got.double() != ref["pre"].double()
            errors.append("C is not the oracle's bits: %d of %d elements, NaN %d" % (int(bad.sum()), bad.numel(), int(got.isnan().sum())))
    # the same call without ln=: the same C, bit for bit; and the LayerNorm launch on it: the same y, mean, rstd, bit for bit
    # (the promise in front of splitk_epilogue_ln_kernel; exact data makes the slab sums equal where the split count differs)
    o_plain, _, failed_plain = _gemm_launch(case, inp, cuda, False, False)
    if failed_plain is not None or not torch.equal(o.C.bits, o_plain.C.bits):
        errors.append("C differs from the same call without ln= (%s)" % failed_plain)
    if case.refused is None:
        ry, rm, rr = _ratios(o.yv, o.mean.view, o.rstd.view, pre_rows, ref, T)
        fig = "pre=%s y=%.3f mean=%.3f rstd=%.3f" % (pre_fig, ry, rm, rr)
        if not max(ry, rm, rr) <= 1.0:
            errors.append("worst error / bound y %g mean %g rstd %g" % (ry, rm, rr))
        y2, mean2, rstd2 = O.layernorm_fwd(o_plain.Cv.clone(), inp.gamma.view, inp.beta.view, eps=1e-12)
        for name, a, b in (("y", o.yv, y2), ("mean", o.mean.view, mean2), ("rstd", o.rstd.view, rstd2)):
            if not GO.bits_equal(a, b):
                errors.append("%s is not bit-identical to the epilogue launch + LayerNorm launch pair" % name)
    else:
        fig = "pre=%s refused: %s" % (pre_fig, failed)
        for name, g in (("ln_out", o.y), ("mean", o.mean), ("rstd", o.rstd)):
            if not _untouched(g):
                errors.append("%s was written although the LayerNorm launch refused" % name)
    o2, _, _ = _gemm_launch(case, inp, cuda, True, False)
    for (name, g1), (_, g2) in zip(o.all(), o2.all()):
        try:
            g1.check(name)
        except AssertionError as err:
            errors.append(str(err))
        if not torch.equal(g1.bits, g2.bits):
            errors.append("%s differs between two launches" % name)
    try:
        inp.check(case.id)
    except AssertionError as err:
        errors.append(str(err))
    print("DENSELN %s %s %s" % (case.id, sorted(kinds.items()), fig))
    assert not errors, case.id + ":\n" + "\n".join(errors[:12])


def test_fp32_never_reaches_the_fused_splitk_layernorm():
    """splitk_ws_ln_fused needs c_dtype != IMT_F32 and check_ln_out c_dtype == dtype: an fp32 product with ln_out is normalised by
    a LayerNorm launch ("Dense + LayerNorm edge tests").  The fp32 cases pin that through their kinds."""
    fp32 = [c for c in DO.GEMM_CASES if c.dtype == "f32"]
    assert len(fp32) >= 9 and all("gemm_splitk_epilogue_ln" not in c.kinds for c in fp32)
    assert all(DO.LN_KIND in c.kinds for c in fp32 if c.refused is None)


# ---- check_ln_out on its three call sites
# site -> (M, N, K in (tiles, chunks), a split-K workspace is passed)
LN_SITES = {"single": (61, 128, (3, 0), False), "ragged_k": (61, 128, (16, 1), False), "splitk_ws": (61, 128, (16, 0), True)}
LN_REASONS = ["ldc", "ld_ln", "c_f32", "accumulate", "split_k", "no_gamma", "no_beta"]


def _ln_refusals():
    out = []
    for site in LN_SITES:
        for why in LN_REASONS:
            for dtype in ("bf16", "f32"):
                if why == "c_f32" and dtype == "f32":
                    continue   # fp32 C IS the compute type there
                if why == "split_k" and dtype == "bf16":
                    continue   # atomic split-K needs fp32 C: with bf16 operands that is the c_f32 refusal
                out.append((site, why, dtype))
    return out


@pytest.mark.parametrize("site,why,dtype", _ln_refusals(), ids=["%s-%s-%s" % c for c in _ln_refusals()])
def test_check_ln_out_refusals(cuda, site, why, dtype):
    """Every precondition of ln_out, on the shape of every strategy that checks it: ImtError, no GEMM launched, C / ln_out /
    mean / rstd unwritten.  (split_k > 1 sends every shape to the single-launch strategy: its three cases all end at that site.)"""
    O, L, lib = _ops()
    T = DO.DT[dtype]
    M, N, (tiles, chunks), ws = LN_SITES[site]
    K = tiles * DO.bk(dtype) + chunks * DO.al(dtype)
    d = DO.inputs(dtype, M, N, K)
    inp = _Inputs(d, dtype, M, N, K, cuda)
    TC = F32 if why == "c_f32" else T
    C = GO.Guard(M, N, TC, cuda) if why == "ldc" else GO.GuardVec(M * N, TC, cuda)
    y = GO.Guard(M, N, T, cuda) if why == "ld_ln" else GO.GuardVec(M * N, T, cuda)
    mean, rstd = GO.GuardVec(M, F32, cuda), GO.GuardVec(M, F32, cuda)
    as_rows = lambda g: g.view if isinstance(g, GO.Guard) else g.view.view(M, N)  # noqa: E731
    kw = dict(out=as_rows(C), ln=dict(gamma=inp.gamma.view, beta=inp.beta.view, out=as_rows(y), mean=mean.view, rstd=rstd.view, eps=1e-12))
    if ws:
        kw["splitk_ws"] = O.splitk_workspace(cuda)
    if why == "accumulate":
        kw["accumulate"] = True
    if why == "split_k":
        kw["split_k"] = 2
    args = O.gemm(inp.x.view, inp.W.view, O.IMT_NT, _launch=False, **kw)
    if why == "no_gamma":
        args.ln_gamma = None
    if why == "no_beta":
        args.ln_beta = None
    rcs = []
    kinds = _kinds_of(lambda: rcs.append(lib.imt_gemm(ctypes.byref(args), O._stream())))
    msg = lib.imt_last_error().decode() if rcs[0] != 0 else ""
    print("DENSELN ln_refusal_%s_%s_%s rc %d %s '%s'" % (site, why, dtype, rcs[0], sorted(kinds.items()), msg))
    with pytest.raises(L.ImtError):
        L.check(rcs[0], "imt_gemm")
    assert "ln_out" in msg, msg
    assert kinds == {}, "launched %s before refusing" % sorted(kinds.items())
    for name, g in (("C", C), ("ln_out", y), ("mean", mean), ("rstd", rstd)):
        assert _untouched(g), "%s was written by a refused call" % name
    inp.check("%s %s" % (site, why))


# ================================================================================================ C: the contract between the paths
@pytest.mark.parametrize("case", DO.CONTRACT_CASES, ids=[c.id for c in DO.CONTRACT_CASES])
def test_three_paths_agree_and_feed_one_backward(cuda, case):
    """One exact data set through (1) imt_gemm_bias_residual_ln, (2) imt_gemm with ln_out and a split-K workspace, (3) imt_gemm with
    ln_out and none: pre-LN bit-identical, y / mean / rstd pairwise within the sum of their bounds, (2) and (3) bit-equal; and
    imt_layernorm_bwd, given what each path saved and the dropout seed, returns the oracle's dx and masks it with the mask
    the forward used (element index m * N + n)."""
    O, L, lib = _ops()
    T = DO.DT[case.dtype]
    M, N, K = case.M, case.N, case.K
    d = DO.inputs(case.dtype, M, N, K)
    keep = _keep(cuda, M, N)
    ref = DO.reference(d["x"], d["W"], T, d["gamma"], d["beta"], 1e-12, bias=d["bias"], keep=keep, resid=d["resid"])
    inp = _Inputs(d, case.dtype, M, N, K, cuda)
    o1, k1 = _fused_launch(inp, M, N, K, T, DO.BDR, 1e-12, cuda, True)
    one = "gemm_ws_%s_nt" % case.dtype
    split = [one, "gemm_splitk_epilogue_ln"] if case.dtype == "bf16" else [one, "gemm_splitk_epilogue", DO.LN_KIND]
    o2, k2, f2 = _gemm_launch(DO.GemmCase(case.id, case.dtype, M, N, K, DO.BDR, True, split, None), inp, cuda, True, True)
    o3, k3, f3 = _gemm_launch(DO.GemmCase(case.id, case.dtype, M, N, K, DO.BDR, False, [one, DO.LN_KIND], None), inp, cuda, True, True)
    assert f2 is None and f3 is None, (f2, f3)
    paths = [(o1.pre.view, o1.out.view, o1.mean.view, o1.rstd.view), (o2.Cv, o2.yv, o2.mean.view, o2.rstd.view),
             (o3.Cv, o3.yv, o3.mean.view, o3.rstd.view)]
    yb, mb, rb = DO.bounds(ref["pre"], ref, T)
    errors, figs = [], []
    if (k1, k2, k3) != ({"gemm_ln_%s" % case.dtype: 1}, _want(split), _want([one, DO.LN_KIND])):
        errors.append("kinds %s / %s / %s" % (sorted(k1.items()), sorted(k2.items()), sorted(k3.items())))
    for i, (pre, y, mean, rstd) in enumerate(paths):
        same = GO.bits_equal(pre.cpu(), ref["pre"])
        ry, rm, rr = DO.worst_ratio(y, ref["y"], yb), DO.worst_ratio(mean, ref["mean"], mb), DO.worst_ratio(rstd, ref["rstd"], rb)
        figs.append("path%d: pre=%s y=%.3f mean=%.3f rstd=%.3f" % (i + 1, "bit-equal" if same else "DIFFERS", ry, rm, rr))
        if not same or not max(ry, rm, rr) <= 1.0:
            errors.append(figs[-1])
    for i, j in ((0, 1), (0, 2), (1, 2)):
        for name, k, b in (("y", 1, yb), ("mean", 2, mb), ("rstd", 3, rb)):
            r = DO.worst_ratio(paths[i][k], paths[j][k].double().cpu(), 2 * b)
            if not r <= 1.0:
                errors.append("%s of path %d and path %d differ by %g of the sum of their bounds" % (name, i + 1, j + 1, r))
    for k, name in ((0, "pre"), (1, "y"), (2, "mean"), (3, "rstd")):
        if not GO.bits_equal(paths[1][k].contiguous(), paths[2][k].contiguous()):
            errors.append("%s of path 2 and path 3 differ in bits" % name)
    # backward
    dy = d["dy"].to(T).to(cuda)
    _, _, _, dx_ref, _, _ = RO.layernorm_fwd_bwd(ref["pre"], d["gamma"], d["beta"], d["dy"], float(torch.tensor(1e-12, dtype=F32)))
    dxb = RO.layernorm_dx_bound(dx_ref, T)
    for i, (pre, y, mean, rstd) in enumerate(paths):
        x_c, mean_c, rstd_c = pre.contiguous(), mean.contiguous(), rstd.contiguous()
        dx, dxd = GO.GuardVec(M * N, T, cuda), GO.GuardVec(M * N, T, cuda)
        grads = torch.zeros(2 * N, device=cuda)
        L.check(lib.imt_layernorm_bwd(O.dt(x_c), O._p(dy), O._p(x_c), O._p(inp.gamma.view), O._p(mean_c), O._p(rstd_c), O._p(dx.view),
                                      O._p(grads[:N]), O._p(grads[N:]), M, N, 0.0, 0, O._p(dxd.view), DO.P_DROP, DO.SEED, None, O._stream()),
                "imt_layernorm_bwd")
        dx.check("path %d dx" % (i + 1))
        dxd.check("path %d dx_drop" % (i + 1))
        got = dx.view.view(M, N).cpu()
        r = DO.worst_ratio(got, dx_ref, dxb)
        figs.append("path%d: dx=%.3f" % (i + 1, r))
        if not r <= 1.0:
            errors.append("path %d: dx at %g of its bound" % (i + 1, r))
        masked = torch.where(keep, (got.float() * DO.INV_KEEP).to(T), torch.zeros(M, N, dtype=T))
        if not torch.equal(dxd.view.view(M, N).cpu(), masked):
            errors.append("path %d: dx_drop is not dx under the forward's mask" % (i + 1))
    inp.check(case.id)
    print("DENSELN %s %s | %s | %s  %s" % (case.id, sorted(k1.items()), sorted(k2.items()), sorted(k3.items()), "  ".join(figs)))
    assert not errors, case.id + ":\n" + "\n".join(errors[:12])
