"""imt_knn_rows on the GPU against the fp64 oracle (tests/mine_oracle.py): exact indices where the data decides them (planted
neighbours, ties), tolerance-aware parity elsewhere, at the kernel's edges: 256-row / 256-column tiles, 32 (fp32) / 64 (bf16)
element K tiles, ragged last tiles, more lists than keys, column ranges (splits), strided views, guards around every output.

Tolerance: the project's fp32 bar of 1e-4 on values with |cos| <= 1 (fp32 accumulation of at most 768 products of unit-vector
components is orders below it).  For bf16 the oracle reads the bf16-rounded inputs: the products of two bf16 numbers are exact in
fp32, so the same bar holds."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import mine_oracle as MO

pytestmark = pytest.mark.gpu
TOL = 1e-4
DTYPES = [torch.float32, torch.bfloat16]
COSINES = [0.95 - 0.03 * j for j in range(8)]   # 0.95, 0.92, ..., 0.74
GAP = 0.05


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def planted(N, M, dtype, d=64, seed=0):
    """Queries in groups around a centre (cosine 0.9995 to it), every group with 8 planted keys at COSINES to the centre, scattered
    over the columns by a random permutation; all other keys are unit Gaussian.  With fewer than 8 keys per query to spare the
    groups share: G = min(16, M // 9, N) groups.  Returns (x, y) rounded to ``dtype`` as fp32 tensors, the fp64 similarities of
    the rounded values, and the oracle's lists for k = 8."""
    rng = np.random.RandomState(seed + 131 * N + M)
    G = max(1, min(16, M // 9, N))
    centres = _unit(rng.randn(G, d))
    y = _unit(rng.randn(M, d))
    cols = rng.permutation(M)[:8 * G].reshape(G, 8)
    for g in range(G):
        for j, c in enumerate(COSINES):
            n = rng.randn(d)
            n = _unit(n - n.dot(centres[g]) * centres[g])
            y[cols[g, j]] = c * centres[g] + np.sqrt(1 - c * c) * n
    group = np.arange(N) % G
    p = rng.randn(N, d)
    p = _unit(p - (p * centres[group]).sum(-1, keepdims=True) * centres[group])
    x = 0.9995 * centres[group] + np.sqrt(1 - 0.9995 ** 2) * p
    xt, yt = (torch.from_numpy(a).to(dtype).float() for a in (x, y))
    sim = MO.similarities(xt.numpy(), yt.numpy())
    val, idx = MO.knn_from_sim(sim, 8)
    # the data decides the indices: the planted keys are the 8 best of every query, in the planted order, and the smallest
    # planted cosine leads the largest unplanted one by GAP; neighbouring planted cosines are 0.03 apart (checked: > 0.015)
    assert (idx[:, :min(8, M)] == cols[group][:, :min(8, M)]).all(), "the planted keys are not the oracle's best, in order"
    if M > 8:
        lead = val[:, 7] - np.sort(sim, axis=1)[:, -9]
        assert lead.min() >= GAP, "planted lead %.3f" % lead.min()
    assert (val[:, :-1] - val[:, 1:]).min() > 0.015
    return xt, yt, sim, val, idx


def raw_knn(x, y, k, *, splits=0, index_base=0, guard_rows=0, ws_guard=0):
    """imt_knn_rows through the C ABI on 2-D views as they are (no copies).  Returns (val, idx int32) with ``guard_rows`` extra
    rows filled with canaries, and the workspace (uint8) with ``ws_guard`` canary bytes behind its stated size."""
    from imagetranslate_amd import _lib as L
    from imagetranslate_amd import hip_ops as O
    lib = L.load()
    N, K = x.shape
    M = y.shape[0]
    val = torch.full((N + guard_rows, k), 777.0, device="cuda", dtype=torch.float32)
    idx = torch.full((N + guard_rows, k), -777, device="cuda", dtype=torch.int32)
    nbytes = int(lib.imt_knn_ws_bytes(N, M, k, splits))
    assert nbytes > 0
    ws = torch.full((nbytes + ws_guard,), 0x5A, device="cuda", dtype=torch.uint8)
    a = L.KnnArgs()
    a.dtype, a.N, a.M, a.K, a.k = O.dt(x), N, M, K, k
    a.x, a.ldx = x.data_ptr(), max(K, x.stride(0))
    a.y, a.ldy = y.data_ptr(), max(K, y.stride(0))
    a.index_base, a.splits = index_base, splits
    a.val, a.idx = val.data_ptr(), idx.data_ptr()
    a.ws, a.ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.imt_knn_rows(ctypes.byref(a), O._stream()), "imt_knn_rows")
    torch.cuda.synchronize()
    return val, idx, ws, nbytes


def check_tolerant(val, idx, sim, k):
    """For every row and rank j: indices distinct and in range; the returned value within TOL of the fp64 similarity of the
    returned index; that similarity within TOL of the oracle's j-th best."""
    N, M = sim.shape
    val, idx = val.cpu().numpy().astype(np.float64), idx.cpu().numpy().astype(np.int64)
    n = min(k, M)
    assert val.shape == idx.shape == (N, k)
    assert (idx[:, :n] >= 0).all() and (idx[:, :n] < M).all(), "index out of range"
    srt = np.sort(idx[:, :n], axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "an index twice in one row"
    at = np.take_along_axis(sim, idx[:, :n], axis=1)
    want, _ = MO.knn_from_sim(sim, k)
    e1, e2 = np.abs(val[:, :n] - at).max(), np.abs(at - want[:, :n]).max()
    print("\n[knn %dx%d k=%d] value vs fp64 of its index %.2e | that vs the oracle's j-th best %.2e" % (N, M, k, e1, e2))
    assert e1 <= TOL and e2 <= TOL
    assert (val[:, :-1] >= val[:, 1:]).all(), "values are not descending"
    assert np.isneginf(val[:, n:]).all() and (idx[:, n:] == -1).all()


SHAPES = [(1, 9), (255, 255), (256, 256), (257, 257), (513, 700)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("N,M", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("k", [1, 4, 8])
def test_planted_neighbours_come_back_with_exact_indices(cuda, N, M, k, dtype):
    from imagetranslate_amd import hip_ops as O
    x, y, sim, wval, widx = planted(N, M, dtype)
    val, idx = O.knn_rows(x.cuda().to(dtype), y.cuda().to(dtype), k)
    assert val.dtype == torch.float32 and idx.dtype == torch.int64 and tuple(val.shape) == tuple(idx.shape) == (N, k)
    assert np.array_equal(idx.cpu().numpy(), widx[:, :k])
    err = np.abs(val.cpu().numpy().astype(np.float64) - wval[:, :k]).max()
    print("\n[knn planted %dx%d k=%d %s] max value error %.2e" % (N, M, k, dtype, err))
    assert err <= TOL


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("N,M,d", [(513, 700, 64), (300, 1000, 768)])
def test_unplanted_data_within_tolerance_for_every_row_and_rank(cuda, N, M, d, dtype):
    from imagetranslate_amd import hip_ops as O
    rng = np.random.RandomState(N + d)
    x, y = (torch.from_numpy(_unit(rng.randn(n, d))).to(dtype).float() for n in (N, M))
    sim = MO.similarities(x.numpy(), y.numpy())
    val, idx = O.knn_rows(x.cuda().to(dtype), y.cuda().to(dtype), 8)
    check_tolerant(val, idx, sim, 8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("splits", [0, 1, 3])
def test_equal_keys_come_back_in_index_order(cuda, dtype, splits):
    """Identical key rows at 3, 255 (one tile, two waves), 256 (the next tile) and 600 that are every query's best."""
    rng = np.random.RandomState(5)
    N, M, d = 257, 700, 64
    g = _unit(rng.randn(d))
    x = torch.from_numpy(_unit(g + 0.04 * rng.randn(N, d))).to(dtype)
    y = _unit(rng.randn(M, d))
    tied = [3, 255, 256, 600]
    y[tied] = g
    y = torch.from_numpy(y).to(dtype)
    sim = MO.similarities(x.float().numpy(), y.float().numpy())
    rest = np.delete(sim, tied, axis=1).max()
    assert sim[:, 3].min() - rest > GAP and (sim[:, tied] == sim[:, 3:4]).all()
    for k, want in ((4, tied), (2, tied[:2]), (8, tied)):
        val, idx, _, _ = raw_knn(x.cuda(), y.cuda(), k, splits=splits)
        got = idx.cpu().numpy()
        assert (got[:, :len(want)] == np.array(want)).all(), (k, got[:3])
        v = val.cpu().numpy()
        assert (v[:, :len(want)] == v[:, :1]).all(), "the same key gives the same product wherever its tile runs"
        if k == 8:
            check_tolerant(val, idx, sim, 8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("M", [257, 300])
def test_zero_filled_columns_of_a_ragged_tile_are_no_candidates(cuda, M, dtype):
    """All similarities negative: the zeros the DMA fills columns >= M with would beat every real key."""
    from imagetranslate_amd import hip_ops as O
    rng = np.random.RandomState(M)
    N, d = 100, 64
    g = _unit(rng.randn(d))
    x = torch.from_numpy(_unit(g + 0.04 * rng.randn(N, d))).to(dtype)
    y = torch.from_numpy(_unit(-g + 0.04 * rng.randn(M, d))).to(dtype)
    sim = MO.similarities(x.float().numpy(), y.float().numpy())
    assert sim.max() < -0.5
    val, idx = O.knn_rows(x.cuda(), y.cuda(), 8)
    assert int(idx.max()) < M and int(idx.min()) >= 0, "an index past the keys"
    assert float(val.max()) < -0.5, "a zero of the ragged tile's fill is among the values"
    check_tolerant(val, idx, sim, 8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_more_places_than_keys_end_in_minus_infinity(cuda, dtype):
    from imagetranslate_amd import hip_ops as O
    rng = np.random.RandomState(3)
    x, y = (torch.from_numpy(_unit(rng.randn(n, 64))).to(dtype) for n in (40, 3))
    sim = MO.similarities(x.float().numpy(), y.float().numpy())
    val, idx = O.knn_rows(x.cuda(), y.cuda(), 8)
    assert torch.isneginf(val[:, 3:]).all() and (idx[:, 3:] == -1).all()
    assert np.array_equal(idx[:, :3].cpu().numpy(), MO.knn_from_sim(sim, 8)[1][:, :3])
    check_tolerant(val, idx, sim, 8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_every_number_of_splits_gives_the_same_bits(cuda, dtype):
    x, y, sim, wval, widx = planted(256, 5000, dtype)
    xc, yc = x.cuda().to(dtype), y.cuda().to(dtype)
    first = None
    for splits in (1, 2, 3, 7, 0):
        val, idx, _, _ = raw_knn(xc, yc, 8, splits=splits)
        if first is None:
            first = (val, idx)
            assert np.array_equal(idx.cpu().numpy(), widx)
            assert np.abs(val.cpu().numpy().astype(np.float64) - wval).max() <= TOL
        assert torch.equal(val, first[0]) and torch.equal(idx, first[1]), "splits = %d changes the result" % splits


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_strided_views_guards_and_index_base(cuda, dtype):
    """Rows of wider buffers (ldx, ldy > K); nothing is written behind val, idx or the workspace's stated size; index_base
    shifts every index."""
    N, M, k = 257, 300, 4
    x, y, sim, wval, widx = planted(N, M, dtype)
    xw = torch.full((N, 96), 9.0, device="cuda", dtype=dtype)
    yw = torch.full((M, 160), -9.0, device="cuda", dtype=dtype)
    xw[:, :64], yw[:, :64] = x.cuda().to(dtype), y.cuda().to(dtype)
    val, idx, ws, nbytes = raw_knn(xw[:, :64], yw[:, :64], k, splits=2, index_base=1000, guard_rows=3, ws_guard=4096)
    assert np.array_equal(idx[:N].cpu().numpy(), widx[:, :k] + 1000)
    assert np.abs(val[:N].cpu().numpy().astype(np.float64) - wval[:, :k]).max() <= TOL
    assert (val[N:] == 777.0).all() and (idx[N:] == -777).all(), "rows past N were written"
    assert (ws[nbytes:] == 0x5A).all(), "the workspace is written beyond imt_knn_ws_bytes"
    # past the keys there is no index to shift
    val, idx, _, _ = raw_knn(xw[:, :64], yw[:3, :64], 8, index_base=1000)
    assert (idx[:, 3:] == -1).all() and int(idx[:, :3].min()) >= 1000 and int(idx[:, :3].max()) < 1003


def test_two_calls_give_the_same_bits(cuda):
    from imagetranslate_amd import hip_ops as O
    rng = np.random.RandomState(11)
    x, y = (torch.from_numpy(_unit(rng.randn(n, 768))).float().cuda() for n in (300, 1000))
    for a, b in ((x, y), (x.bfloat16(), y.bfloat16())):
        one, two = O.knn_rows(a, b, 8), O.knn_rows(a, b, 8)
        assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_key_chunks_merge_to_the_bits_of_one_call(cuda, dtype):
    from imagetranslate_amd import hip_ops as O
    x, y, sim, wval, widx = planted(513, 700, dtype)
    xc, yc = x.cuda().to(dtype), y.cuda().to(dtype)
    for k in (1, 8):
        one = O.knn_rows(xc, yc, k)
        three = O.knn_rows(xc, yc, k, _key_chunk=234)
        assert torch.equal(one[0], three[0]) and torch.equal(one[1], three[1])
        both = O.knn_rows(xc, yc, k, _key_chunk=234, _query_chunk=200)   # query chunks too: 200 + 200 + 113 rows
        assert torch.equal(one[0], both[0]) and torch.equal(one[1], both[1])
        assert np.array_equal(three[1].cpu().numpy(), widx[:, :k])
    # equal keys in different chunks keep index order through the merge
    yc2 = yc.clone()
    yc2[[5, 300, 650]] = yc[int(widx[0, 0])]
    one, three = O.knn_rows(xc, yc2, 4), O.knn_rows(xc, yc2, 4, _key_chunk=234)
    assert torch.equal(one[0], three[0]) and torch.equal(one[1], three[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_a_vector_length_that_is_no_whole_tile_is_zero_padded(cuda, dtype):
    from imagetranslate_amd import hip_ops as O
    rng = np.random.RandomState(100)
    x, y = (torch.from_numpy(_unit(rng.randn(n, 100))).to(dtype) for n in (130, 300))
    sim = MO.similarities(x.float().numpy(), y.float().numpy())
    val, idx = O.knn_rows(x.cuda(), y.cuda(), 4)
    check_tolerant(val, idx, sim, 4)


def test_wrapper_refuses_what_the_kernel_does_not_take(cuda):
    from imagetranslate_amd import hip_ops as O
    x = torch.zeros(4, 64, device="cuda")
    with pytest.raises(ValueError):
        O.knn_rows(x, x, 9)
    with pytest.raises(ValueError):
        O.knn_rows(x, x.bfloat16(), 4)
    val, idx = O.knn_rows(x, x[:0], 4)
    assert torch.isneginf(val).all() and (idx == -1).all()


def test_keys_past_the_two_gib_operand_limit_are_chunked_with_global_indices(cuda):
    """4.2 million fp32 keys of 128 elements are 2 GiB + 500 KB: one call cannot address them (32-bit DMA offsets), so
    ``knn_rows`` makes two and ``index_base`` carries the second chunk's offset.  A key equal to query 1 sits at the first
    index, on either side of the chunk boundary and at the last index: exactly these come back, in index order, at cosine 1.
    The other queries are compared with an fp64 product on the device (sliced: the keys in fp64 would be 4 GiB)."""
    from imagetranslate_amd import hip_ops as O
    K = 128
    M = (1 << 31) // (K * 4) + 1000
    g = torch.Generator(device="cuda").manual_seed(0)
    y = torch.nn.functional.normalize(torch.randn(M, K, device="cuda", generator=g), dim=-1)
    x = torch.nn.functional.normalize(torch.randn(3, K, device="cuda", generator=g), dim=-1)
    limit = O._knn_max_rows(y)
    assert limit < M < 2 * limit, "two chunks"
    plant = [0, limit - 1, limit, M - 1]
    y[plant] = x[1]
    val, idx = O.knn_rows(x, y, 4)
    assert idx[1].tolist() == plant, idx[1].tolist()
    assert float((val[1] - 1.0).abs().max()) <= TOL
    sim = torch.cat([y[c0:c0 + (1 << 20)].double() @ x.double().t() for c0 in range(0, M, 1 << 20)]).t().contiguous()
    want, _ = torch.topk(sim, 4, dim=1)
    at = sim.gather(1, idx)
    e1, e2 = float((val.double() - at).abs().max()), float((at - want).abs().max())
    print("\n[knn 3x%d two chunks] value vs fp64 of its index %.2e | that vs the j-th best %.2e" % (M, e1, e2))
    assert e1 <= TOL and e2 <= TOL
    assert int(idx.min()) >= 0 and int(idx.max()) < M and float(sim[0].max()) < 0.6
