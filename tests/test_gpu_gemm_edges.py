"""imt_gemm (csrc/gemm.hip, csrc/gemm_xl.hpp) where its tiles end, its K loops take their first / last / odd trip, its leading
dimensions differ from the extents and its strategies change kernel, against the fp64 restatement of tests/gemm_oracle.py.
tests/test_gpu_ops.py compares one 200 x 264 x 136 NT product with a reference by max|a-b| / max|b| and otherwise kernel
variants with each other: a fault in the epilogue code they share agrees with itself.  Per case (CASES; the id names the kernel
the case is there for -- the one a forced variant falls back to when it cannot run the shape):

  * the launch reaches exactly the kernels the id names (imt_prof_report, as tests/test_gpu_gemm_dispatch.py reads it);
  * operands are small integers plus an asymmetric ramp, bias / residual / old C integers, p = 0.5 and alpha a power of two,
    so every fp32 sum is exact: fp32 C must equal the oracle BIT FOR BIT, bf16 C the oracle rounded to nearest even;
  * GELU / GELU' are real-valued: |got - ref| <= gemm_oracle.bound element by element (the erf approximation's stated error
    through the factor by which it enters, 4 fp32 roundings of the terms' magnitude, one output rounding);
  * A, B, bias, residual, the GELU' input, C, the GELU aux and a_colsum are views inside wider buffers filled with a NaN bit
    pattern, leading dimensions wider than the extents: everything outside C / aux / a_colsum comes back bit-unchanged, the
    inputs come back bit-unchanged entirely, and no NaN of a pad reaches a result;
  * a second launch into a fresh copy returns the same bits (atomic split-K included: the data is exact).

Under dropout the keep mask is RECOVERED from a launch whose pre-dropout value cannot be zero (|bias| = 4, |alpha A B| <= 2:
kept <=> C != resid), never restated from the generator; test_dropout_mask_* require that mask, flattened, to be one function
of (seed, m * N + n) on every variant, across full and edge tiles, across shapes that share their flat indices, in the split-K
epilogue launch and in imt_add_rows_dropout (the row-kernel convention imt_layernorm_bwd relies on).

Each case prints ``GEMMEDGE <id> <kinds> <epilogue>=<bit-equal | worst error / bound> ...`` before it asserts (pytest -s;
DESIGN.md, "GEMM edge tests", records the figures)."""
import collections

import pytest
import torch

from tests import gemm_oracle as GO

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF16, "f32": F32}
LAYOUT = {"NT": GO.NT, "NN": GO.NN, "TN": GO.TN}
FAMILY = {1: "dbuf", 3: "sbuf", 5: "ws", 6: "xl"}
SEED = 0x5DEECE66D
P_EXACT = 0.5   # inv_keep = 2: dropout keeps the sums exact


def _units(dtype):
    """(bk, al): K elements per tile (128 bytes), elements per 16-byte chunk."""
    return (64, 8) if dtype == "bf16" else (32, 4)


def _k_of(kspec, dtype):
    bk, al = _units(dtype)
    tiles, chunks, extra = kspec
    return tiles * bk + chunks * al + extra


def _k_name(kspec):
    tiles, chunks, extra = kspec
    parts = ([("%dbk" % tiles) if tiles > 1 else "bk"] if tiles else []) + (["al"] if chunks else []) + ([str(extra)] if extra else [])
    return "+".join(parts)


# every epilogue of a single launch: what it passes beside the operands
EPILOGUES = collections.OrderedDict([
    ("plain", {}), ("bias", {"bias": 1}), ("bias_gelu", {"bias": 1, "aux": "gelu"}), ("dgelu", {"aux": "dgelu"}), ("resid", {"resid": 1}),
    ("bias_drop_resid", {"bias": 1, "drop": 1, "resid": 1}), ("drop", {"drop": 1}), ("alpha", {"alpha": 1}), ("acc", {"acc": 1}),
    ("f32", {"f32": 1}), ("f32_acc", {"f32": 1, "acc": 1}), ("gelu_f32", {"bias": 1, "aux": "gelu", "f32": 1}),
    ("alpha_f32_acc", {"alpha": 1, "f32": 1, "acc": 1}), ("colsum_acc", {"f32": 1, "acc": 1, "colsum": 1})])
EP_SINGLE = ["plain", "bias", "bias_gelu", "dgelu", "resid", "bias_drop_resid", "drop", "alpha", "acc", "f32", "f32_acc", "gelu_f32"]
EP_SLABS = ["plain", "alpha", "acc", "f32", "f32_acc"]          # IMT_AUX_SPLITK_WS: plain epilogue only (alpha / alpha_dev)
EP_ATOMIC = ["f32_acc", "alpha_f32_acc", "colsum_acc"]          # split_k > 1: fp32 atomics onto the caller's C, no epilogue

Case = collections.namedtuple("Case", "id sid layout dtype M N K ld variant mode split_k kinds epilogues")
ALL4 = {1: "dbuf", 3: "sbuf", 5: "ws", 6: "xl"}
NO_DMA = {1: "dbuf", 3: "sbuf", 5: "sbuf", 6: "sbuf"}   # fewer than two whole K tiles (NT / NN: or a ragged K): the LDS-DMA loops cannot run it

# (id, layouts, M, N, K in (tiles, chunks, elements), leading dimensions that are stated rather than derived, variant -> kernel family)
SHAPES = [
    ("tiny", ("NT", "NN", "TN"), 5, 8, (0, 1, 0), {}, NO_DMA),
    ("tiny", ("NT", "NN", "TN"), 5, 8, (1, 1, 0), {}, NO_DMA),
    ("tiny", ("NT",), 5, 6, (0, 1, 0), {}, NO_DMA),
    ("tiny", ("NT",), 5, 6, (1, 1, 0), {}, NO_DMA),
    ("full", ("NT", "NN", "TN"), 256, 256, (2, 0, 0), {}, ALL4),
    ("full", ("NT", "NN", "TN"), 256, 256, (7, 0, 0), {}, ALL4),
    ("edges", ("NT", "NN", "TN"), 300, 392, (3, 0, 0), {}, ALL4),
    ("edges", ("NT",), 300, 390, (3, 0, 0), {"ldc": 392}, ALL4),
    ("edges", ("TN",), 300, 392, (3, 0, 1), {}, ALL4),
    ("edges", ("TN",), 300, 392, (2, 0, 1), {}, ALL4),
    ("overhang", ("NN",), 200, 136, (0, 0, 193), {"lda": 200}, NO_DMA),
    ("overhang", ("NN", "TN"), 200, 133, (2, 0, 0), {"ldb": 136}, ALL4),
    # the weight gradient over a vocabulary of 193 entries: the M extent of the K-strided A ends on an odd element
    ("overhang", ("TN",), 193, 136, (2, 0, 0), {"lda": 200}, ALL4),
    ("splitk_ws", ("NT", "NN"), 200, 136, (16, 0, 0), {}, ALL4),   # the same shape as single launches of every variant
]


def _kind(family, dtype, layout):
    return "gemm_%s_%s_%s" % (family, dtype, layout.lower())


def _cases():
    out = []

    def add(sid, layout, dtype, M, N, kspec, ld, variant, mode, split_k, kinds, eps):
        K = _k_of(kspec, dtype)
        cid = "%s_%s_%dx%dx%s_%s_v%d%s_%s" % (sid, layout, M, N, _k_name(kspec), dtype, variant, ("_s%d" % split_k) if split_k > 1 else "", "+".join(kinds))
        out.append(Case(cid, sid, layout, dtype, M, N, K, dict(ld), variant, mode, split_k, list(kinds), list(eps)))

    for dtype in ("bf16", "f32"):
        for (sid, layouts, M, N, kspec, ld, runs) in SHAPES:
            for layout in layouts:
                for variant in (1, 3, 5, 6):
                    eps = EP_SINGLE + (["colsum_acc"] if layout == "TN" else [])
                    add(sid, layout, dtype, M, N, kspec, ld, variant, "single", 1, [_kind(runs[variant], dtype, layout)], eps)
        # 272 tiles on 256 workgroups of the persistent kernel: sixteen run a non-last tile (256 threads in the epilogue) and then a
        # last tile (512: the producer waves join without accumulators); the last tile row is ragged; TN: the extra barriers of
        # the fused column sums
        add("walk", "NT", dtype, 2136, 2048, (2, 0, 0), {}, 5, "single", 1, [_kind("ws", dtype, "NT")], ["plain", "resid", "f32_acc"])
        add("walk", "TN", dtype, 2136, 2048, (2, 0, 0), {}, 5, "single", 1, [_kind("ws", dtype, "TN")], ["colsum_acc"])
        for layout in ("NT", "NN"):
            # K ranges on the persistent kernel into fp32 slabs + the epilogue launch (imt_gemm_args.splitk_ws; the policy's own choice)
            add("splitk_ws", layout, dtype, 200, 136, (16, 0, 0), {}, 0, "ws", 1, [_kind("ws", dtype, layout), "gemm_splitk_epilogue"], EP_SINGLE)
            # IMT_AUX_SPLITK_WS: ragged tail first (its own small product); uneven ranges; 11 tiles over 5 splits = ranges of 3, the
            # last one EMPTY, which must still write a zero slab
            add("slabs", layout, dtype, 300, 392, (4, 1, 0), {}, 0, "slabs", 2, [_kind("sbuf", dtype, layout), _kind("xl", dtype, layout), "gemm_splitk_reduce"], EP_SLABS)
            add("slabs", layout, dtype, 300, 392, (7, 0, 0), {}, 0, "slabs", 3, [_kind("xl", dtype, layout), "gemm_splitk_reduce"], EP_SLABS)
            add("slabs", layout, dtype, 300, 392, (11, 0, 0), {}, 0, "slabs", 5, [_kind("xl", dtype, layout), "gemm_splitk_reduce"], EP_SLABS)
        for split_k in (2, 4):
            for variant in (1, 3):
                add("atomic", "TN", dtype, 300, 392, (5, 0, 0), {}, variant, "atomic", split_k, [_kind(FAMILY[variant], dtype, "TN")], EP_ATOMIC)
    return out


CASES = _cases()


# ------------------------------------------------------------------------------------------------ shared data (computed once, never modified)
_PRODUCTS, _EPI_DATA, _KEEP = {}, {}, {}


def _ops():
    from imagetranslate_amd import hip_ops as O
    return O


def _kinds_of(fn):
    """Kernel kinds (imt_prof_report rows) launched by fn(), as {kind: launches}."""
    from imagetranslate_amd import _lib as L
    lib = L.load()
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


def _product(layout, M, N, K):
    key = (layout, M, N, K)
    if key not in _PRODUCTS:
        A, B = GO.integer_operands(LAYOUT[layout], M, N, K, 1)
        _PRODUCTS[key] = (A, B, GO.product(LAYOUT[layout], A, B))
    return _PRODUCTS[key]


def _epi_data(M, N):
    """Integer bias / residual / old C / old column sums and a real-valued GELU' input for an [M, N] output (fp32, CPU)."""
    if (M, N) not in _EPI_DATA:
        g = torch.Generator().manual_seed(1000 * M + N)
        _EPI_DATA[(M, N)] = dict(bias=torch.randint(-4, 5, (N,), generator=g).float(), resid=torch.randint(-3, 4, (M, N), generator=g).float(),
                                 C0=torch.randint(-3, 4, (M, N), generator=g).float(), colsum0=torch.randint(-3, 4, (M,), generator=g).float(),
                                 auxin=torch.randn(M, N, generator=g) * 1.5)
    return _EPI_DATA[(M, N)]


def _int_bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _recover_mask(dev, M, N, p, *, dtype=F32, variant=1, k_tiles=0, splitk_ws=False, kinds=None):
    """The keep mask [M, N] (bool, CPU) of one bias + dropout + residual launch (NT) whose pre-dropout value is provably
    non-zero: A B is 1 or 2 (one non-zero column of A and B), bias is -4, so v is -3 or -2 and kept <=> C != resid, bit-wise."""
    O = _ops()
    bk, al = (64, 8) if dtype == BF16 else (32, 4)
    K = k_tiles * bk if k_tiles else al
    A = torch.zeros(M, K)
    A[:, 0] = 1.0
    B = torch.zeros(N, K)
    B[:, 0] = 1.0 + (torch.arange(N) % 2).float()
    bias = torch.full((N,), -4.0)
    resid = _epi_data(M, N)["resid"]
    pre = GO.reference(GO.NT, A, B, dtype, bias=bias)
    assert float(pre["accmag"].max()) <= 6.0 and float((pre["pre"] - bias.double()).abs().max()) <= 2.0 and float(pre["pre"].abs().min()) >= 2.0
    gC = GO.Guard(M, N, dtype, dev)
    gR = GO.Guard(M, N, dtype, dev).put(resid)
    kw = dict(out=gC.view, bias=bias.to(dtype).to(dev), resid=gR.view, dropout_p=p, dropout_seed=SEED, force_general=variant)
    if splitk_ws:
        kw["splitk_ws"] = O.splitk_workspace(dev)
    got = _kinds_of(lambda: O.gemm(A.to(dtype).to(dev), B.to(dtype).to(dev), O.IMT_NT, **kw))
    if kinds is not None:
        assert got == _want(kinds), (got, kinds)
    gC.check("mask launch C")
    gR.check_all("mask launch resid")
    keep = (_int_bits(gC.view) != _int_bits(gR.view)).cpu()
    # what the launch wrote is what the oracle gives UNDER that mask (so a kept element is the scaled value, not just "different")
    if p == P_EXACT:
        ref = GO.reference(GO.NT, A, B, dtype, bias=bias, keep=keep, dropout_p=p, resid=resid)
        assert GO.bits_equal(gC.view.cpu(), ref["out"].to(dtype)), "mask launch: kept values are not 2 v + resid"
    return keep


def _keep_for_cases(dev, M, N):
    """The mask the exact cases hold every kernel to: recovered ONCE per shape from the register-staged fp32 kernel (that all
    other paths make the same mask is what they are then held to, and what test_dropout_mask_* check directly)."""
    if (M, N) not in _KEEP:
        _KEEP[(M, N)] = _recover_mask(dev, M, N, P_EXACT)
    return _KEEP[(M, N)]


# ------------------------------------------------------------------------------------------------ one case
class _Inputs:
    def __init__(self, case, dev):
        T = DT[case.dtype]
        A, B, self.prod = _product(case.layout, case.M, case.N, case.K)
        self.A_cpu, self.B_cpu = A, B
        d = _epi_data(case.M, case.N)
        self.d = d
        self.A = GO.Guard(A.shape[0], A.shape[1], T, dev, ld=case.ld.get("lda")).put(A)
        self.B = GO.Guard(B.shape[0], B.shape[1], T, dev, ld=case.ld.get("ldb")).put(B)
        self.bias = GO.GuardVec(case.N, T, dev).put(d["bias"])
        self.resid = GO.Guard(case.M, case.N, T, dev).put(d["resid"])
        self.auxin_cpu = d["auxin"].to(T)   # rounded to the compute type: what the kernel reads
        self.auxin = GO.Guard(case.M, case.N, T, dev).put(self.auxin_cpu)
        self.alpha_dev = torch.tensor([0.5], device=dev, dtype=F32)

    def check(self, what):
        for name in ("A", "B", "bias", "resid", "auxin"):
            getattr(self, name).check_all("%s: %s" % (what, name))


def _launch(case, epn, inp, dev, with_kinds):
    """One launch of epilogue ``epn`` into fresh guarded outputs: (C guard, aux guard | None, colsum guard | None, slab guard | None, kinds | None)."""
    O = _ops()
    T = DT[case.dtype]
    e = EPILOGUES[epn]
    d = inp.d
    out_dtype = F32 if e.get("f32") else T
    C = GO.Guard(case.M, case.N, out_dtype, dev, ld=case.ld.get("ldc"))
    if e.get("acc"):
        C.put(d["C0"])
    kw = dict(out=C.view, accumulate=bool(e.get("acc")), force_general=case.variant)
    aux = colsum = slabs = None
    if e.get("bias"):
        kw["bias"] = inp.bias.view
    if e.get("resid"):
        kw["resid"] = inp.resid.view
    if e.get("aux") == "gelu":
        aux = GO.Guard(case.M, case.N, T, dev)
        kw.update(aux=aux.view, aux_mode=O.IMT_AUX_GELU_FWD)
    elif e.get("aux") == "dgelu":
        kw.update(aux=inp.auxin.view, aux_mode=O.IMT_AUX_DGELU)
    if e.get("drop"):
        kw.update(dropout_p=P_EXACT, dropout_seed=SEED)
    if e.get("alpha"):
        kw.update(alpha=0.25, alpha_dev=inp.alpha_dev)
    if e.get("colsum"):
        colsum = GO.GuardVec(case.M, F32, dev).put(d["colsum0"])
        kw["a_colsum"] = colsum.view
    if case.mode == "ws":
        kw["splitk_ws"] = O.splitk_workspace(dev)
    elif case.mode == "slabs":
        slabs = GO.GuardVec(case.split_k * case.M * case.N, F32, dev)
        kw.update(aux=slabs.view.view(case.split_k * case.M, case.N), aux_mode=O.IMT_AUX_SPLITK_WS, split_k=case.split_k)
    elif case.mode == "atomic":
        kw["split_k"] = case.split_k

    def call():
        O.gemm(inp.A.view, inp.B.view, LAYOUT[case.layout], **kw)

    kinds = None
    if with_kinds:
        kinds = _kinds_of(call)
    else:
        call()
        torch.cuda.synchronize()
    return C, aux, colsum, slabs, kinds


def _reference(case, epn, inp, keep):
    e = EPILOGUES[epn]
    d = inp.d
    T = DT[case.dtype]
    return GO.reference(LAYOUT[case.layout], inp.A_cpu, inp.B_cpu, T, prod=inp.prod,
                        alpha=0.25 if e.get("alpha") else 1.0, alpha_dev=0.5 if e.get("alpha") else None,
                        bias=d["bias"] if e.get("bias") else None,
                        aux_mode={"gelu": GO.AUX_GELU_FWD, "dgelu": GO.AUX_DGELU}.get(e.get("aux"), GO.AUX_NONE), aux=inp.auxin_cpu,
                        keep=keep if e.get("drop") else None, dropout_p=P_EXACT if e.get("drop") else 0.0,
                        resid=d["resid"] if e.get("resid") else None, C0=d["C0"] if e.get("acc") else None,
                        colsum0=d["colsum0"] if e.get("colsum") else None)


def _exact_report(got, want):
    """None when bit-equal, else how many elements differ and by how much."""
    if GO.bits_equal(got, want):
        return None
    bad = (_int_bits(got) != _int_bits(want))
    diff = (got.double() - want.double()).abs()
    return "%d of %d elements differ (max |diff| %g, NaN %d)" % (int(bad.sum()), bad.numel(), float(diff[~diff.isnan()].max()) if bool((~diff.isnan()).any()) else float("nan"),
                                                                int(got.isnan().sum()))


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gemm_edges(cuda, case):
    T = DT[case.dtype]
    inp = _Inputs(case, cuda)
    keep = _keep_for_cases(cuda, case.M, case.N) if any(EPILOGUES[e].get("drop") for e in case.epilogues) else None
    if case.mode == "slabs" and case.K % _units(case.dtype)[0]:
        # the ragged tail goes into C first and the whole-tile body is added on top: one rounding only as long as C holds the tail
        # exactly -- true of this data (asserted), so bf16 C is still the oracle rounded once
        bk = _units(case.dtype)[0]
        kb = case.K // bk * bk
        tail = (inp.A_cpu[:, kb:].double() @ (inp.B_cpu[:, kb:].double().t() if case.layout == "NT" else inp.B_cpu[kb:].double()))
        for s in (1.0, 0.125):
            for c0 in (0.0, inp.d["C0"].double()):
                assert torch.equal((s * tail + c0).to(T).double(), s * tail + c0)
    figures, errors, kinds_seen = [], [], None
    for epn in case.epilogues:
        e = EPILOGUES[epn]
        what = "%s / %s" % (case.id, epn)
        C, aux, colsum, slabs, kinds = _launch(case, epn, inp, cuda, True)
        kinds_seen = kinds
        if kinds != _want(case.kinds):
            errors.append("%s: launched %s, the case is there for %s" % (what, sorted(kinds.items()), case.kinds))
        ref = _reference(case, epn, inp, keep)
        got = C.view.cpu()
        real = e.get("aux") is not None
        if real:
            b = GO.bound(ref, {"gelu": GO.AUX_GELU_FWD, "dgelu": GO.AUX_DGELU}[e["aux"]], got.dtype)
            err = (got.double() - ref["out"]).abs()
            ratio = float(torch.where(err == 0, torch.zeros_like(err), err / b).nan_to_num(nan=float("inf")).max())  # (NaN in got: inf)
            figures.append("%s=%.3f" % (epn, ratio))
            if not ratio <= 1.0:
                errors.append("%s: worst |got - ref| / bound = %g" % (what, ratio))
        else:
            rep = _exact_report(got, ref["out"].to(got.dtype))
            figures.append("%s=%s" % (epn, "bit-equal" if rep is None else "DIFFERS"))
            if rep is not None:
                errors.append("%s: C is not the oracle's bits: %s" % (what, rep))
        if aux is not None:   # what GELU stores for the backward: the pre-activation rounded to T, exact data -> exact bits
            rep = _exact_report(aux.view.cpu(), ref["aux"])
            if rep is not None:
                errors.append("%s: aux is not the rounded pre-activation: %s" % (what, rep))
        if colsum is not None:
            rep = _exact_report(colsum.view.cpu(), ref["colsum"].to(F32))
            if rep is not None:
                errors.append("%s: a_colsum: %s" % (what, rep))
        # guards, and a second launch into fresh copies: same bits everywhere
        C2, aux2, colsum2, slabs2, _ = _launch(case, epn, inp, cuda, False)
        for (name, g1, g2) in (("C", C, C2), ("aux", aux, aux2), ("a_colsum", colsum, colsum2), ("slab workspace", slabs, slabs2)):
            if g1 is None:
                continue
            try:
                g1.check("%s: %s" % (what, name))
            except AssertionError as err:
                errors.append(str(err))
            if name != "slab workspace" and not torch.equal(g1.bits, g2.bits):
                errors.append("%s: %s differs between two launches" % (what, name))
        try:
            inp.check(what)
        except AssertionError as err:
            errors.append(str(err))
    print("GEMMEDGE %s %s %s" % (case.id, sorted((kinds_seen or {}).items()), " ".join(figures)))
    assert not errors, "\n".join(errors[:12])


# ------------------------------------------------------------------------------------------------ the dropout mask
MASK_P = (0.1, 0.5)


@pytest.mark.parametrize("p", MASK_P)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_dropout_mask_same_flat_indices(cuda, dtype, p):
    """(256, 390) and (195, 512) share their 99 840 flat indices m * N + n.  The first takes the per-element branch of the fast
    epilogue (full tiles, N % 4 != 0), edge tiles and the scalar tail; the second dropout_apply4 on full and ragged-M tiles."""
    T = DT[dtype]
    a = _recover_mask(cuda, 256, 390, p, dtype=T, variant=3, kinds=[_kind("sbuf", dtype, "NT")])
    b = _recover_mask(cuda, 195, 512, p, dtype=T, variant=3, kinds=[_kind("sbuf", dtype, "NT")])
    frac = float(a.float().mean())
    print("GEMMEDGE mask_flat_%s_p%g kept %.4f" % (dtype, p, frac))
    assert abs(frac - (1.0 - p)) < 0.01   # 99 840 draws: sigma < 0.0016
    assert torch.equal(a.reshape(-1), b.reshape(-1)), "%d decisions differ" % int((a.reshape(-1) != b.reshape(-1)).sum())
    rows = _ops().add_rows_dropout(torch.ones(195, 512, device=cuda, dtype=T), dropout_p=p, dropout_seed=SEED)
    assert torch.equal((rows != 0).cpu(), b), "imt_add_rows_dropout makes another mask than the GEMM epilogue"


@pytest.mark.parametrize("p", MASK_P)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_dropout_mask_every_variant(cuda, dtype, p):
    """(300, 392): a mask row crosses full and edge tiles of 128 and of 256; every variant must make the mask of the row kernels."""
    T = DT[dtype]
    rows = (_ops().add_rows_dropout(torch.ones(300, 392, device=cuda, dtype=T), dropout_p=p, dropout_seed=SEED) != 0).cpu()
    for variant in (1, 3, 5, 6):
        m = _recover_mask(cuda, 300, 392, p, dtype=T, variant=variant, k_tiles=2, kinds=[_kind(FAMILY[variant], dtype, "NT")])
        assert torch.equal(m, rows), "variant %d: %d decisions differ from imt_add_rows_dropout" % (variant, int((m != rows).sum()))


@pytest.mark.parametrize("p", MASK_P)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_dropout_mask_splitk_epilogue(cuda, dtype, p):
    """(200, 136), K = 16 tiles with a split-K workspace: the mask is made by splitk_epilogue_kernel."""
    T = DT[dtype]
    rows = (_ops().add_rows_dropout(torch.ones(200, 136, device=cuda, dtype=T), dropout_p=p, dropout_seed=SEED) != 0).cpu()
    m = _recover_mask(cuda, 200, 136, p, dtype=T, variant=0, k_tiles=16, splitk_ws=True, kinds=[_kind("ws", dtype, "NT"), "gemm_splitk_epilogue"])
    one = _recover_mask(cuda, 200, 136, p, dtype=T, variant=3, k_tiles=16, kinds=[_kind("sbuf", dtype, "NT")])
    assert torch.equal(m, rows) and torch.equal(one, rows)
