"""imt_gemm_grouped_tn (csrc/gemm.hip: gemm_grouped_tn_kernel<T, 128>, grouped_tall_tile, SlabDma, grouped_tile) element by
element against the fp64 restatement of tests/gemm_oracle.py: every weight and bias gradient of a training step comes out of
this kernel.  tests/test_gpu_ops.py compares it norm-wise on dense operands and tests/test_gpu_grouped_dw_tiles.py its two
instances with each other; the instances share the epilogue, the DMA descriptors, the column-sum scheme and the tile map, so a
fault in any of those agrees with itself.  Per case (CASES; tests/test_grouped_oracle.py checks the table on the CPU) and per
problem of its list:

  * operands are GO.integer_operands (integers in -3..3 plus the asymmetric ramps), old C and old a_colsum integers in -4..4,
    alpha 1 or 0.5: every fp32 partial sum is exact in any order, the atomic column sums included, so dW must equal the oracle
    rounded to fp32 BIT FOR BIT and db the oracle's column sums bit for bit;
  * A [K, M], B [K, N], C [M, N] and a_colsum [M] are views inside wider buffers filled with a NaN bit pattern (leading
    dimensions wider than the extents, NaN rows just past K: a DMA descriptor sized by anything but the view extent lets them
    in): the inputs come back bit-unchanged, everything outside C / a_colsum comes back bit-unchanged, every result is finite;
  * a second launch into fresh copies returns the same bits;
  * a groupable list is exactly one gemm_<dt>_tn_grouped launch (imt_prof_report), a list that imt_gemm_grouped_tn refuses
    shows no such kind and at least one launch per product -- and is held to the same bits;
  * groupable lists run on the 128 x 128 instance and, where grouped_tall's preconditions hold (_tall_ok), on the 256 x 128
    one; each instance against the oracle, never only against the other.

The Gaussian cases (real-valued data: the integers hide dropped mantissa bits) are held element by element to the textbook
bound of a K-term fp32 sum in any order over exact products, |got - ref| <= (K + 2) 2^-24 mag, mag the sum of the terms'
magnitudes (GO.reference; for db: sum_k |a| + |db0|).

Each case prints ``GROUPEDGE <id> <instance> <kind> dW=bit-equal db=bit-equal`` (Gaussian: the worst error / bound) before it
asserts (pytest -s; DESIGN.md, "Grouped weight-gradient edge tests", records them)."""
import collections

import pytest
import torch

from tests import gemm_oracle as GO
from tests.test_gpu_gemm_edges import _exact_report, _k_of, _kinds_of, _units

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF16, "f32": F32}
MAX_GROUP = 16          # csrc/gemm.hip
GROUP_MAX_TILES = 640   # counted in 128 x 128 tiles
AL = "al"               # a row / column count of one 16-byte chunk of the compute type

# M, N: extents or AL; kspec: K in (K tiles, chunks, elements) as _k_of; colsum: the problem carries a bias gradient;
# ld: leading dimensions that are stated rather than the guards' defaults (multiples of al / of 4 for ldc)
Prob = collections.namedtuple("Prob", "M N kspec colsum alpha ld")
# refused: None = groupable, else the one condition of imt_gemm_grouped_tn the list is there to violate (refusals())
Case = collections.namedtuple("Case", "id dtype probs refused")


def P(M, N, kspec, colsum=True, alpha=1.0, **ld):
    return Prob(M, N, kspec, colsum, alpha, ld)


def _k_name(kspec):
    tiles, chunks, extra = kspec
    return "%dbk" % tiles + ("+%dal" % chunks if chunks else "") + ("%+d" % extra if extra else "")


K2, K2P, K3M, K3, K3P, K5P, K9P = (2, 0, 0), (2, 0, 1), (3, 0, -1), (3, 0, 0), (3, 0, 1), (5, 0, 1), (9, 0, 1)
# 1. ring depth: K -> (trips of the K-tile loop, trips of the K-slab loop).  The 128 instance's ring holds four K tiles (three in
# flight), the 256 instance's six K slabs of half a tile (five in flight).
RING = collections.OrderedDict([
    (K2, (2, 4)),     # prologue shorter than both rings
    (K2P, (3, 5)),    # a last tile / slab with a single valid row
    (K3M, (3, 6)),    # last tile one row short
    (K3, (3, 6)),
    (K3P, (4, 7)),    # first in-loop issue of the square ring; the tall ring wraps
    (K5P, (6, 11)),   # the square ring wraps
    (K9P, (10, 19)),  # several wraps, ragged
])
# 2. tile edges: every M of {al, 128, 136, 200, 264} and every N of {al, 128, 136, 392}, the corner (200, 136) among them
TILE_EDGES = [[(AL, AL), (128, 128), (136, 392), (200, 136)], [(264, AL), (AL, 136), (200, 392), (264, 128), (128, 136)]]
# 3. the tall instance where N ends: every M of {256, 512, 768} with every N of {al, 136, 392} at least once
TALL_EDGES = [(256, AL), (512, 136), (768, 392), (256, 392), (768, AL), (512, 392), (256, 136)]
# 4. six problems with their own K and leading dimensions, bias gradient on 1, 3 and 4, alpha = 0.5: 34 square tiles (17 tall)
MIXED = [P(256, 136, K2, False, 0.5, lda=264, ldb=152, ldc=140), P(512, 128, K2P, True, 0.5, lda=528, ldb=136, ldc=132),
         P(256, 392, K9P, False, 0.5, lda=288, ldb=408, ldc=396), P(512, 136, K3, True, 0.5, lda=520, ldb=160, ldc=144),
         P(256, 264, K3M, True, 0.5, lda=272, ldb=280, ldc=268), P(512, AL, K5P, False, 0.5, lda=536, ldb=16, ldc=12)]
MIXED_FEW = [P(128, 136, K2P, True, 0.5), P(200, AL, K3, False, 0.5, lda=208), P(AL, 128, K9P, True, 0.5, ldb=136)]   # 5 tiles
# 5. 1024 x 2048 is 8 x 16 square tiles: five of them are the 640 a group may hold (320 tall ones: 2 * 320 <= 640)
FULL640 = [P(1024, 2048, K2, i % 2 == 0) for i in range(5)]


def _cases():
    out = []
    for dtype in ("bf16", "f32"):
        def add(cid, probs, refused=None):
            out.append(Case("%s_%s" % (cid, dtype), dtype, list(probs), refused))

        for kspec in RING:
            add("ring_" + _k_name(kspec), [P(256, 128, kspec, False), P(256, 136, kspec, True)])
        for i, shapes in enumerate(TILE_EDGES):
            add("tile_edges_%s" % "ab"[i], [P(M, N, K3P) for (M, N) in shapes])
        add("tall_n_edges", [P(M, N, K3P) for (M, N) in TALL_EDGES])
        add("mixed_34_tiles", MIXED)
        add("mixed_5_tiles", MIXED_FEW)
        add("limit_16_problems", [P(128, 128, K2P, i % 3 != 1) for i in range(MAX_GROUP)])
        add("limit_640_tiles", FULL640)
        add("refused_17_problems", [P(128, 128, K2P, i % 3 != 1) for i in range(MAX_GROUP + 1)], "count")
        add("refused_641_tiles", FULL640 + [P(128, 128, K2)], "tiles")
        add("refused_m_193", [P(256, 136, K3P), P(193, 136, K3P), P(128, 128, K3P, False)], "m_align")
        add("refused_one_k_tile", [P(256, 128, K2), P(256, 136, (1, 0, 0))], "k_tiles")
        add("refused_alpha_differs", [P(256, 128, K2P), P(256, 136, K2P, True, 0.5)], "alpha")
    return out


CASES = _cases()
# 7. real-valued data, per dtype and instance
GAUSS = [(512, 392), (256, 136)]
GAUSS_K = K9P


# ------------------------------------------------------------------------------------------------ the table, resolved (CPU)
def _al(dtype):
    return _units(dtype)[1]


def extents(p, dtype):
    """(M, N, K) of a problem in elements."""
    al = _al(dtype)
    return (al if p.M == AL else p.M, al if p.N == AL else p.N, _k_of(p.kspec, dtype))


def lds(p, dtype):
    """(lda, ldb, ldc) in elements: stated, or GO.Guard's default (the extent rounded up to a chunk, plus one chunk)."""
    M, N, _ = extents(p, dtype)
    al = _al(dtype)
    return (p.ld.get("lda", (M + al - 1) // al * al + al), p.ld.get("ldb", (N + al - 1) // al * al + al), p.ld.get("ldc", (N + 3) // 4 * 4 + 4))


def loop_trips(K, dtype):
    """(K tiles of the 128 x 128 instance, K slabs of the 256 x 128 instance): the trip counts of the two K loops."""
    bk = _units(dtype)[0]
    return (K + bk - 1) // bk, (K + bk // 2 - 1) // (bk // 2)


def square_tiles(case):
    return sum(((M + 127) // 128) * ((N + 127) // 128) for (M, N, _) in (extents(p, case.dtype) for p in case.probs))


def refusals(case):
    """The conditions of imt_gemm_grouped_tn (csrc/gemm.hip) that the list fails, by name; empty = one grouped launch.  (Same
    dtype, TN, fp32 C, no other epilogue and 16-byte aligned bases hold for every list this file builds.)"""
    bk, al = _units(case.dtype)
    es = 2 if case.dtype == "bf16" else 4
    bad = set()
    if len(case.probs) > MAX_GROUP:
        bad.add("count")
    if square_tiles(case) > GROUP_MAX_TILES:
        bad.add("tiles")
    for p in case.probs:
        (M, N, K), (lda, ldb, ldc) = extents(p, case.dtype), lds(p, case.dtype)
        if M % al:
            bad.add("m_align")
        if N % al:
            bad.add("n_align")
        if K // bk < 2:
            bad.add("k_tiles")
        if p.alpha != case.probs[0].alpha:
            bad.add("alpha")
        if lda % al or ldb % al or ldc % 4:
            bad.add("ld_align")
        if K * lda * es >= 1 << 31 or K * ldb * es >= 1 << 31:
            bad.add("bytes")
    return bad


def _tall_ok(shapes):
    """grouped_tall's preconditions (csrc/gemm.hip): every row count a multiple of 256, and the 256 x 128 tiles, counted as two
    128 x 128 ones each, within the 640 a group may hold."""
    if any(M % 256 for (M, N) in shapes):
        return False
    return 2 * sum((M // 256) * ((N + 127) // 128) for (M, N) in shapes) <= GROUP_MAX_TILES


def instances(case):
    """tile_rows settings a case runs with: both instances where it is groupable and grouped_tall allows, 0 = the policy for
    the lists that are refused anyway."""
    if case.refused is not None:
        return [0]
    return [128] + ([256] if _tall_ok([extents(p, case.dtype)[:2] for p in case.probs]) else [])


RUNS = [(c, t) for c in CASES for t in instances(c)]


# ------------------------------------------------------------------------------------------------ shared data (computed once, never modified)
_DATA = {}


def problem_data(dtype, p, seed):
    """Operands, old C / a_colsum and the oracle's dW / db rounded to fp32 (CPU tensors) of one problem, shared by every case
    that holds it; mag / csmag: the largest sum of the terms' magnitudes of a dW / db element."""
    M, N, K = extents(p, dtype)
    key = (M, N, K, seed, p.colsum, p.alpha)
    if key not in _DATA:
        A, B = GO.integer_operands(GO.TN, M, N, K, seed)
        g = torch.Generator().manual_seed(7919 * seed + 1000 * M + N)
        C0 = torch.randint(-4, 5, (M, N), generator=g).float()
        cs0 = torch.randint(-4, 5, (M,), generator=g).float() if p.colsum else None
        ref = GO.reference(GO.TN, A, B, DT[dtype], alpha=p.alpha, C0=C0, colsum0=cs0)
        csmag = p.alpha * A.double().abs().sum(0) + cs0.double().abs() if p.colsum else None
        # (only what the checks need is kept: the 640-tile lists are 8 MB per tensor and problem)
        _DATA[key] = dict(A=A, B=B, C0=C0, cs0=cs0, want_dw=ref["out"].to(F32), want_db=ref["colsum"].to(F32) if p.colsum else None,
                          mag=float(ref["mag"].max()), csmag=float(csmag.max()) if p.colsum else 0.0,
                          exact=bool((ref["out"].to(F32).double() == ref["out"]).all()))
    return _DATA[key]


def case_data(case):
    return [problem_data(case.dtype, p, 1 + i) for i, p in enumerate(case.probs)]


# ------------------------------------------------------------------------------------------------ one launch
class _Group:
    """The guarded inputs of a list (uploaded once) and launches of it into fresh guarded outputs."""

    def __init__(self, dtype, probs, data, dev):
        self.dtype, self.probs, self.data, self.dev = dtype, probs, data, dev
        T = DT[dtype]
        self.A, self.B = [], []
        for p, d in zip(probs, data):
            (M, N, K), (lda, ldb, _) = extents(p, dtype), lds(p, dtype)
            self.A.append(GO.Guard(K, M, T, dev, ld=lda).put(d["A"]))
            self.B.append(GO.Guard(K, N, T, dev, ld=ldb).put(d["B"]))

    def launch(self, tile_rows, with_kinds):
        """-> ([(C guard, a_colsum guard | None)], kinds | None)"""
        from imagetranslate_amd import hip_ops as O
        outs, problems = [], []
        for p, d, gA, gB in zip(self.probs, self.data, self.A, self.B):
            M, N, _ = extents(p, self.dtype)
            C = GO.Guard(M, N, F32, self.dev, ld=lds(p, self.dtype)[2]).put(d["C0"])
            cs = GO.GuardVec(M, F32, self.dev).put(d["cs0"]) if p.colsum else None
            outs.append((C, cs))
            problems.append(dict(A=gA.view, B=gB.view, out=C.view, a_colsum=None if cs is None else cs.view, alpha=p.alpha))

        def call():
            O.gemm_grouped_tn(problems, tile_rows=tile_rows)

        kinds = None
        if with_kinds:
            kinds = _kinds_of(call)
        else:
            call()
            torch.cuda.synchronize()
        return outs, kinds

    def check_inputs(self, what, errors):
        for i, (gA, gB) in enumerate(zip(self.A, self.B)):
            for name, g in (("A", gA), ("B", gB)):
                try:
                    g.check_all("%s: %s of problem %d" % (what, name, i))
                except AssertionError as err:
                    errors.append(str(err))


def _check_guards_and_repeat(what, outs, outs2, errors):
    for i, ((C, cs), (C2, cs2)) in enumerate(zip(outs, outs2)):
        for name, g1, g2 in (("C", C, C2), ("a_colsum", cs, cs2)):
            if g1 is None:
                continue
            try:
                g1.check("%s: %s of problem %d" % (what, name, i))
            except AssertionError as err:
                errors.append(str(err))
            if not torch.equal(g1.bits, g2.bits):
                errors.append("%s: %s of problem %d differs between two launches" % (what, name, i))


def _check_dispatch(what, case_refused, count, dtype, kinds, errors):
    grouped = "gemm_%s_tn_grouped" % dtype
    if case_refused is None:
        if kinds != {grouped: 1}:
            errors.append("%s: launched %s, a groupable list is exactly one %s" % (what, sorted(kinds.items()), grouped))
    elif any("tn_grouped" in k for k in kinds) or sum(kinds.values()) < count:
        errors.append("%s: launched %s, the list must fall back to one imt_gemm per product (%d)" % (what, sorted(kinds.items()), count))


def _instance_name(tile_rows):
    return {0: "policy", 128: "128x128", 256: "256x128"}[tile_rows]


def _xcd_shares_ending_inside(grids):
    """How many of the eight XCDs' runs of the tile list end inside a problem (grouped_tile: workgroup w runs on XCD w % 8)."""
    from imagetranslate_amd import hip_ops as O
    order = O.grouped_tile_order(grids)
    assert sorted(order) == sorted((i, r, c) for i, (R, Cc) in enumerate(grids) for r in range(R) for c in range(Cc))
    inside = 0
    for x in range(min(8, len(order))):
        i, r, c = order[max(w for w in range(len(order)) if w % 8 == x)]
        inside += (r, c) != (grids[i][0] - 1, grids[i][1] - 1)
    return inside


@pytest.mark.parametrize("case,tile_rows", RUNS, ids=["%s-%s" % (c.id, _instance_name(t)) for (c, t) in RUNS])
def test_grouped_edges(cuda, case, tile_rows):
    assert refusals(case) == (set() if case.refused is None else {case.refused})
    what = "%s / %s" % (case.id, _instance_name(tile_rows))
    if case.id.startswith("mixed_34"):
        shapes = [extents(p, case.dtype)[:2] for p in case.probs]
        tm = tile_rows
        grids = [((M + tm - 1) // tm, (N + 127) // 128) for (M, N) in shapes]
        total = sum(r * c for r, c in grids)
        assert total == {128: 34, 256: 17}[tm] and total % 8 != 0
        assert _xcd_shares_ending_inside(grids) >= 2
    data = case_data(case)
    grp = _Group(case.dtype, case.probs, data, cuda)
    errors = []
    outs, kinds = grp.launch(tile_rows, True)
    _check_dispatch(what, case.refused, len(case.probs), case.dtype, kinds, errors)
    dw_ok = db_ok = True
    for i, (p, d, (C, cs)) in enumerate(zip(case.probs, data, outs)):
        got = C.view.cpu()
        rep = _exact_report(got, d["want_dw"])
        if rep is not None or not bool(got.isfinite().all()):
            dw_ok = False
            errors.append("%s: dW of problem %d %s is not the oracle's bits: %s" % (what, i, extents(p, case.dtype), rep))
        if cs is not None:
            got = cs.view.cpu()
            rep = _exact_report(got, d["want_db"])
            if rep is not None or not bool(got.isfinite().all()):
                db_ok = False
                errors.append("%s: db of problem %d %s is not the oracle's bits: %s" % (what, i, extents(p, case.dtype), rep))
    outs2, _ = grp.launch(tile_rows, False)
    _check_guards_and_repeat(what, outs, outs2, errors)
    grp.check_inputs(what, errors)
    print("GROUPEDGE %s %s %s dW=%s db=%s" % (case.id, _instance_name(tile_rows), "+".join("%s:%d" % kv for kv in sorted(kinds.items())),
                                              "bit-equal" if dw_ok else "DIFFERS", "bit-equal" if db_ok else "DIFFERS"))
    assert not errors, "\n".join(errors[:12])


# ------------------------------------------------------------------------------------------------ real-valued data
def _ratio(got, ref, bound):
    err = (got.double() - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).nan_to_num(nan=float("inf")).max())   # (NaN in got: inf)


@pytest.mark.parametrize("tile_rows", [128, 256])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_grouped_gaussian(cuda, dtype, tile_rows):
    assert _tall_ok(GAUSS)
    T = DT[dtype]
    K = _k_of(GAUSS_K, dtype)
    probs = [P(M, N, GAUSS_K) for (M, N) in GAUSS]
    g = torch.Generator().manual_seed(20 + K)
    data = []
    for (M, N) in GAUSS:
        A, B = torch.randn(K, M, generator=g).to(T).float(), torch.randn(K, N, generator=g).to(T).float()   # what the kernel reads
        C0, cs0 = torch.randn(M, N, generator=g), torch.randn(M, generator=g)
        data.append(dict(A=A, B=B, C0=C0, cs0=cs0, ref=GO.reference(GO.TN, A, B, T, C0=C0, colsum0=cs0),
                         csmag=A.double().abs().sum(0) + cs0.double().abs()))
    what = "gauss_%s / %s" % (dtype, _instance_name(tile_rows))
    grp = _Group(dtype, probs, data, cuda)
    errors = []
    outs, kinds = grp.launch(tile_rows, True)
    _check_dispatch(what, None, len(probs), dtype, kinds, errors)
    u = (K + 2) * GO.U32
    worst_dw = max(_ratio(C.view.cpu(), d["ref"]["out"], u * d["ref"]["mag"]) for d, (C, cs) in zip(data, outs))
    worst_db = max(_ratio(cs.view.cpu(), d["ref"]["colsum"], u * d["csmag"]) for d, (C, cs) in zip(data, outs))
    outs2, _ = grp.launch(tile_rows, False)
    _check_guards_and_repeat(what, outs, outs2, errors)
    grp.check_inputs(what, errors)
    print("GROUPEDGE gauss_%s %s %s dW=%.4f db=%.4f" % (dtype, _instance_name(tile_rows), "+".join("%s:%d" % kv for kv in sorted(kinds.items())),
                                                       worst_dw, worst_db))
    if not worst_dw <= 1.0:
        errors.append("%s: dW: worst |got - ref| / bound = %g" % (what, worst_dw))
    if not worst_db <= 1.0:
        errors.append("%s: db: worst |got - ref| / bound = %g" % (what, worst_db))
    assert not errors, "\n".join(errors[:12])
