"""The case table of tests/test_gpu_grouped_edges.py, checked without a GPU: its integer data is exact in fp32, its ring-depth
cases take the K-loop trips they are there for, each refused list fails exactly one condition of imt_gemm_grouped_tn, and the
mixed groups have the tile totals their XCD shares need."""
import pytest
import torch

from tests import gemm_oracle as GO
from tests import test_gpu_grouped_edges as GE

CASES = GE.CASES
IDS = [c.id for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_integer_cases_are_exact_in_fp32(case):
    """|alpha| sum_k |a||b| + |C0| < 2^24 for every dW element (and the same for db): every partial sum, in any order, is a
    multiple of 1/2 below 2^23 in magnitude -- an fp32 number; the operands themselves are bf16 numbers."""
    for p, d in zip(case.probs, GE.case_data(case)):
        M, N, K = GE.extents(p, case.dtype)
        assert tuple(d["A"].shape) == (K, M) and tuple(d["B"].shape) == (K, N) and p.alpha in (1.0, 0.5)
        assert torch.equal(d["A"].to(GE.DT[case.dtype]).float(), d["A"]) and torch.equal(d["B"].to(GE.DT[case.dtype]).float(), d["B"])
        assert d["mag"] < 2 ** 24 and d["csmag"] < 2 ** 24 and d["exact"]
        assert float(d["C0"].abs().max()) <= 4 and torch.equal(d["C0"], d["C0"].round())
        assert (d["cs0"] is not None) == p.colsum == (d["want_db"] is not None)
        assert d["want_dw"].dtype == torch.float32 and bool(d["want_dw"].isfinite().all())


def test_problem_data_is_the_oracle():
    """problem_data keeps only the rounded oracle: restate one problem by hand (alpha = 0.5, bias gradient on)."""
    p = GE.P(16, 8, GE.K2P, True, 0.5)
    d = GE.problem_data("bf16", p, 3)
    want = 0.5 * d["A"].double().t() @ d["B"].double() + d["C0"].double()
    assert torch.equal(d["want_dw"].double(), want)
    assert torch.equal(d["want_db"].double(), 0.5 * d["A"].double().sum(0) + d["cs0"].double())
    assert d["mag"] == float((0.5 * d["A"].double().abs().t() @ d["B"].double().abs() + d["C0"].double().abs()).max())


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_ring_depth_cases_take_the_trips_the_table_claims(dtype):
    bk = GE._units(dtype)[0]
    slab = bk // 2
    assert (bk, slab) == {"bf16": (64, 32), "f32": (32, 16)}[dtype]
    # the table of the issue: K in tiles and tokens -> K slabs, and what the case reaches
    assert [(GE._k_of(k, dtype), GE.RING[k]) for k in GE.RING] == [
        (2 * bk, (2, 4)), (2 * bk + 1, (3, 5)), (3 * bk - 1, (3, 6)), (3 * bk, (3, 6)), (3 * bk + 1, (4, 7)), (5 * bk + 1, (6, 11)), (9 * bk + 1, (10, 19))]
    ring = {c.id: c for c in CASES if c.id.startswith("ring_") and c.dtype == dtype}
    assert len(ring) == len(GE.RING)
    for kspec, (tiles, slabs) in GE.RING.items():
        case = ring["ring_%s_%s" % (GE._k_name(kspec), dtype)]
        assert case.refused is None and GE.instances(case) == [128, 256]
        assert [GE.extents(p, dtype)[:2] for p in case.probs] == [(256, 128), (256, 136)] and [p.colsum for p in case.probs] == [False, True]
        for p in case.probs:
            K = GE.extents(p, dtype)[2]
            assert GE.loop_trips(K, dtype) == (tiles, slabs), (case.id, K)
            # restated: whole trips plus one for a ragged rest; rows valid in the last trip
            assert tiles == K // bk + (K % bk != 0) and slabs == K // slab + (K % slab != 0)
    K = {k: GE._k_of(k, dtype) for k in GE.RING}
    assert K[GE.K2] // bk < 3 and GE.RING[GE.K2][1] < 5            # the prologue of neither ring (3 tiles, 5 slabs) fills
    assert K[GE.K2P] % bk == 1 and K[GE.K2P] % slab == 1           # a single valid row in the last tile and slab
    assert K[GE.K3M] % bk == bk - 1                                # one row short
    assert GE.RING[GE.K3P] == (4, 7)                               # trip 0 issues tile 3 in the loop; slab 6 reuses slot 0
    assert GE.RING[GE.K5P][0] > 4 and GE.RING[GE.K9P][0] > 8 and GE.RING[GE.K9P][1] > 12   # slots taken a second and third time


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_each_refused_list_fails_exactly_one_condition(case):
    bad = GE.refusals(case)
    if case.refused is None:
        assert bad == set() and GE.instances(case)[0] == 128
        return
    assert bad == {case.refused} and GE.instances(case) == [0]
    # the condition restated on its own, and the list without the offending problem is groupable
    bk, al = GE._units(case.dtype)
    ext = [GE.extents(p, case.dtype) for p in case.probs]
    if case.refused == "count":
        assert len(case.probs) == GE.MAX_GROUP + 1
        rest = case.probs[:-1]
    elif case.refused == "tiles":
        assert GE.square_tiles(case) == GE.GROUP_MAX_TILES + 1
        rest = case.probs[:-1]
    elif case.refused == "m_align":
        assert [M % al != 0 for (M, N, K) in ext] == [False, True, False] and ext[1][0] == 193
        rest = [case.probs[0], case.probs[2]]
    elif case.refused == "k_tiles":
        assert [K // bk for (M, N, K) in ext] == [2, 1]
        rest = case.probs[:1]
    else:
        assert case.refused == "alpha" and [p.alpha for p in case.probs] == [1.0, 0.5]
        rest = case.probs[:1]
    assert GE.refusals(GE.Case("rest", case.dtype, rest, None)) == set()


def test_refusals_cover_the_issue():
    for dtype in ("bf16", "f32"):
        assert sorted(c.refused for c in CASES if c.dtype == dtype and c.refused) == ["alpha", "count", "k_tiles", "m_align", "tiles"]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_mixed_groups_and_limits(dtype):
    by_id = {c.id: c for c in CASES if c.dtype == dtype}
    mixed = by_id["mixed_34_tiles_" + dtype]
    assert len(mixed.probs) == 6 and GE.square_tiles(mixed) == 34 and GE.square_tiles(mixed) % 8 != 0
    assert [i for i, p in enumerate(mixed.probs) if p.colsum] == [1, 3, 4] and all(p.alpha == 0.5 for p in mixed.probs)
    ks = [p.kspec for p in mixed.probs]
    assert len(set(ks)) == 6 and {GE.K2, GE.K2P, GE.K9P} <= set(ks)
    shapes = [GE.extents(p, dtype)[:2] for p in mixed.probs]
    assert GE.instances(mixed) == [128, 256] and sum((M // 256) * ((N + 127) // 128) for (M, N) in shapes) == 17
    # every leading dimension is wider than its extent and no two problems share one
    l3 = [GE.lds(p, dtype) for p in mixed.probs]
    assert all(la > M and lb > N and lc > N for (la, lb, lc), (M, N) in zip(l3, shapes))
    assert len({l[0] for l in l3}) == 6 and len({l[1] for l in l3}) == 6 and len({l[2] for l in l3}) == 6
    few = by_id["mixed_5_tiles_" + dtype]
    assert GE.square_tiles(few) == 5 and GE.instances(few) == [128]
    assert len(by_id["limit_16_problems_" + dtype].probs) == GE.MAX_GROUP
    full = by_id["limit_640_tiles_" + dtype]
    assert GE.square_tiles(full) == GE.GROUP_MAX_TILES and GE.instances(full) == [128, 256]
    assert [GE.extents(p, dtype) for p in full.probs] == [(1024, 2048, 2 * GE._units(dtype)[0])] * 5
    # the axes of the tile-edge lists
    al = GE._units(dtype)[1]
    edge = [GE.extents(p, dtype)[:2] for cid in ("tile_edges_a_", "tile_edges_b_") for p in by_id[cid + dtype].probs]
    assert {M for (M, N) in edge} == {al, 128, 136, 200, 264} and {N for (M, N) in edge} == {al, 128, 136, 392} and (200, 136) in edge
    tall = by_id["tall_n_edges_" + dtype]
    assert GE.instances(tall) == [128, 256]
    tall = [GE.extents(p, dtype)[:2] for p in tall.probs]
    assert {M for (M, N) in tall} == {256, 512, 768} and {N for (M, N) in tall} == {al, 136, 392}


def test_tall_preconditions():
    assert GE._tall_ok([(256, 8), (768, 392)]) and not GE._tall_ok([(256, 128), (384, 128)])
    assert GE._tall_ok([(1024, 2048)] * 5) and not GE._tall_ok([(1024, 2048)] * 5 + [(256, 8)])
    assert GE._tall_ok(GE.GAUSS)


def test_every_view_has_nan_pads():
    """GO.Guard's default leading dimension is what lds() restates, and it is wider than the extent."""
    for dtype in ("bf16", "f32"):
        for p in (GE.P(GE.AL, 392, GE.K2), GE.P(193, 136, GE.K2), GE.P(200, GE.AL, GE.K2)):
            M, N, K = GE.extents(p, dtype)
            lda, ldb, ldc = GE.lds(p, dtype)
            dev = torch.device("cpu")
            assert GO.Guard(K, M, GE.DT[dtype], dev).ld == lda > M and GO.Guard(K, N, GE.DT[dtype], dev).ld == ldb > N
            assert GO.Guard(M, N, torch.float32, dev).ld == ldc > N
