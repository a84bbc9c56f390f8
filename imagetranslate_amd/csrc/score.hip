// Scoring of given target tokens (see include/imt_hip.h, imt_score_rows): logprob[r] = logit[r, target[r]] - logsumexp(logit[r, :])
// with logit = x W^T + bias, WITHOUT ever storing the [N, V] logits.
//
// score_xl_kernel is gemm_xl_kernel's NT main loop (gemm_xl.hpp: 256 x 256 tile, two 64-KiB LDS-DMA stages, 8 waves as
// 2 (m) x 4 (n), acc[8][4] per wave) with an epilogue that REDUCES the tile.  A lane holds, per 16-row group i = 0..7, four
// quads j of consecutive columns of one row (XlOwn, gemm_xl.hpp).  Per group i:
//   1. v = acc + bias (columns >= V of the ragged last tile -> -inf: the DMA zero-filled them, they must not count);
//      (max, sum exp(v - max)) over the lane's 16 values;
//   2. the 4 lanes lg of a row combine with two xor-shuffles (16, 32) -> the wave's 64 columns;
//   3. lane lg == 0 parks the pair in LDS (free after the K loop), [256 rows][4 waves wni].
// After one barrier thread t combines the 4 pairs of row t in wave order and stores ONE float2 per (row, column tile).
// The single lane of the grid whose column equals target[row] stores that logit (plain vector store).  Rows >= N store
// nothing.  score_combine_kernel then merges the column tiles of a row in tile order and, with segments, sums the rows of
// a sentence in a fixed order: no atomics anywhere, two runs are bit-identical.
#include <math.h>
#include "gemm_xl.hpp"

namespace {

// (m, s) <- (m, s) (+) (m2, s2) for partial log-sum-exps: max m, s = sum exp(v - m).  An empty part is (-inf, 0).
IMT_DEVICE void lse_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  const float b = mn == -INFINITY ? 0.f : mn;
  s = s * __expf(m - b) + s2 * __expf(m2 - b);
  m = mn;
}

constexpr int SCORE_ROWS = 256;  // rows per workgroup of both kernels

template <typename T, bool RAGGED_N>
IMT_DEVICE void score_tile_reduce(const f32x4 (&acc)[8][4], f32x2* red, int m0, int n0, const XlWave w, int N, int V,
                                  const T* __restrict__ bias, const int64_t* __restrict__ target, float* __restrict__ tlogit) {
  const XlOwn own(w);
  const int nl = n0 + own.col(0);  // first column of this lane's j = 0 quad
  f32x4 bv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // ragged: bias has exactly V entries -- quads are 4-aligned and V need not be, so the last quad is read by element
    if (!bias) bv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    else if (!RAGGED_N) bv[j] = Vec4<T>::load(bias + nl + 16 * j);
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const int n = nl + 16 * j + e; bv[j][e] = n < V ? to_f32<T>(bias[n]) : 0.f; }
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int rl = own.row(i), row = m0 + rl;
    const int64_t t = row < N ? target[row] : (int64_t)-1;
    // column of the target relative to this lane's first column: 16 j + e for e < 4, anything else is not mine
    const int tc = (t >= 0 && t < V) ? (int)t - nl : -1;
    f32x4 v[4];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = acc[i][j] + bv[j];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (RAGGED_N && nl + 16 * j + e >= V) v[j][e] = -INFINITY;
        mx = fmaxf(mx, v[j][e]);
      }
    }
    // exactly one lane of the grid per counted row; a wave meets a target in ~3 % of its row groups at V = 30000, so the
    // 16 compare-selects sit behind a branch instead of in every group
    const bool mine = tc >= 0 && tc < 64 && (tc & 15) < 4;
    if (__builtin_amdgcn_ballot_w64(mine) != 0) {  // wave-uniform: a real branch, not 16 predicated selects per group
      float tv = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) if (tc == 16 * j + e) tv = v[j][e];
      if (mine) tlogit[row] = tv;
    }
    // sum exp(v - max) as exp2((v - max) * log2 e) on the packed fp32 pipe (two elements per issue slot for the subtract,
    // the scale and the partial sums; the exponential itself is a quarter-rate instruction)
    const float b = mx == -INFINITY ? 0.f : mx;
    const f32x2 b2 = {b, b};
    f32x2 s2 = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x2 lo = (f32x2{v[j][0], v[j][1]} - b2) * 1.4426950408889634f, hi = (f32x2{v[j][2], v[j][3]} - b2) * 1.4426950408889634f;
      s2 += f32x2{__builtin_amdgcn_exp2f(lo.x), __builtin_amdgcn_exp2f(lo.y)};
      s2 += f32x2{__builtin_amdgcn_exp2f(hi.x), __builtin_amdgcn_exp2f(hi.y)};
    }
    float s = s2.x + s2.y;
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) {
      const float mo = __shfl_xor(mx, o, 64), so = __shfl_xor(s, o, 64);
      lse_merge(mx, s, mo, so);
    }
    if (own.lg == 0) red[rl * 4 + w.wni] = f32x2{mx, s};
  }
}

template <typename T>
__global__ __launch_bounds__(XL_THREADS) void score_xl_kernel(const T* __restrict__ X, int64_t ldx, int64_t x_bytes,
                                                              const T* __restrict__ W, int64_t ldw, int64_t w_bytes, int N, int V,
                                                              int K, const T* __restrict__ bias, const int64_t* __restrict__ target,
                                                              f32x2* __restrict__ part, float* __restrict__ tlogit,
                                                              unsigned long long* trace) {
  constexpr int BK = TileGeom<T, true>::BK;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nbx = (V + 255) / 256, nby = (N + 255) / 256;
  const int bid = imt_xcd_block(blockIdx.x, nbx * nby);
  const int bx = bid % nbx;
  const int m0 = (bid / nbx) * 256, n0 = bx * 256;
  const int nt = K / BK;  // whole K tiles (host-checked)
  const XlWave w;

  IMT_STAMP(trace, 0);
  DmaPair<T> dma;
  if (w.loads_a) dma.template init<true>(X, ldx, x_bytes, m0, w.wave);
  else           dma.template init<true>(W, ldw, w_bytes, n0, w.wave - 4);

  f32x4 acc[8][4];
  xl_zero(acc);
  // gemm_xl_kernel's own K loop: the logits are the ones imt_gemm would have produced in fp32
  xl_k_loop<T, IMT_NT>(acc, smem, dma, w, 0, nt, 0, trace, [](const char*) {});
  IMT_STAMP(trace, 2);
  __syncthreads();  // everyone has read the last stage: LDS is free
  f32x2* red = reinterpret_cast<f32x2*>(smem);  // [256 rows][4 waves wni], 8 KiB
  if (n0 + 256 > V) score_tile_reduce<T, true>(acc, red, m0, n0, w, N, V, bias, target, tlogit);
  else              score_tile_reduce<T, false>(acc, red, m0, n0, w, N, V, bias, target, tlogit);
  __syncthreads();
  IMT_STAMP(trace, 3);
  if (threadIdx.x < SCORE_ROWS && m0 + (int)threadIdx.x < N) {
    const f32x4 p01 = *reinterpret_cast<const f32x4*>(red + threadIdx.x * 4);
    const f32x4 p23 = *reinterpret_cast<const f32x4*>(red + threadIdx.x * 4 + 2);
    float m = p01[0], s = p01[1];
    lse_merge(m, s, p01[2], p01[3]);
    lse_merge(m, s, p23[0], p23[1]);
    lse_merge(m, s, p23[2], p23[3]);
    part[(int64_t)bx * N + m0 + threadIdx.x] = f32x2{m, s};
  }
  IMT_STAMP(trace, 4);
}

// lse and log-prob of one row from its per-column-tile partials, in tile order
IMT_DEVICE void score_row(const f32x2* __restrict__ part, const float* __restrict__ tlogit, const int64_t* __restrict__ target,
                          int row, int N, int V, int ntile, float& lse, float& lp, bool& counted) {
  float m = -INFINITY;
  for (int i = 0; i < ntile; ++i) m = fmaxf(m, part[(int64_t)i * N + row][0]);
  float s = 0.f;
  for (int i = 0; i < ntile; ++i) {
    const f32x2 p = part[(int64_t)i * N + row];
    s += p[1] * expf(p[0] - m);
  }
  lse = m + logf(s);
  const int64_t t = target[row];
  counted = t >= 0 && t < V;
  lp = counted ? tlogit[row] - lse : 0.f;
}

// workgroups [0, nrb): 256 rows each -> logprob / lse.  workgroups nrb + s: sentence s -> seg_score[s], its rows
// recomputed from the partials (the launch has no order between workgroups) and summed in a fixed order: thread t takes
// rows off + t, off + t + 256, ... in sequence, then a fixed LDS tree.
__global__ __launch_bounds__(SCORE_ROWS) void score_combine_kernel(const f32x2* __restrict__ part, const float* __restrict__ tlogit,
                                                                   const int64_t* __restrict__ target, float* __restrict__ logprob,
                                                                   float* __restrict__ lse_out, const int64_t* __restrict__ seg_offsets,
                                                                   float* __restrict__ seg_score, int N, int V, int ntile, int nrb,
                                                                   int normalize) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < nrb) {
    const int row = blockIdx.x * SCORE_ROWS + tid;
    if (row >= N) return;
    float lse, lp;
    bool counted;
    score_row(part, tlogit, target, row, N, V, ntile, lse, lp, counted);
    logprob[row] = lp;
    if (lse_out) lse_out[row] = lse;
    return;
  }
  __shared__ float sh_sum[SCORE_ROWS];
  __shared__ int sh_cnt[SCORE_ROWS];
  const int seg = blockIdx.x - nrb;
  int64_t r0 = seg_offsets[seg], r1 = seg_offsets[seg + 1];
  r0 = r0 < 0 ? 0 : r0;           // host-side offsets are the caller's: never index outside [0, N)
  r1 = r1 > N ? (int64_t)N : r1;
  float sum = 0.f;
  int cnt = 0;
  for (int64_t r = r0 + tid; r < r1; r += SCORE_ROWS) {
    float lse, lp;
    bool counted;
    score_row(part, tlogit, target, (int)r, N, V, ntile, lse, lp, counted);
    sum += lp;
    cnt += counted ? 1 : 0;
  }
  sh_sum[tid] = sum;
  sh_cnt[tid] = cnt;
  __syncthreads();
  for (int o = SCORE_ROWS / 2; o > 0; o >>= 1) {
    if (tid < o) { sh_sum[tid] += sh_sum[tid + o]; sh_cnt[tid] += sh_cnt[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) seg_score[seg] = (normalize && sh_cnt[0] > 0) ? sh_sum[0] / (float)sh_cnt[0] : sh_sum[0];
}

template <typename T> int launch_score(const imt_score_args* a, hipStream_t st) {
  auto kern = score_xl_kernel<T>;
  static const bool lds_ok = allow_lds(kern, XL_LDS);
  IMT_CHECK_LDS(lds_ok, "score_rows", XL_LDS);
  const int ntile = imt_cdiv(a->V, 256), nrb = imt_cdiv(a->N, 256);
  float* tlogit = reinterpret_cast<float*>(a->ws);
  f32x2* part = reinterpret_cast<f32x2*>(reinterpret_cast<char*>(a->ws) + imt_align256((int64_t)a->N * 4));
  const int64_t x_bytes = view_bytes(a->N, a->ldx, a->K, sizeof(T)), w_bytes = view_bytes(a->V, a->ldw, a->K, sizeof(T));
  const double es = sizeof(T);
  {
    const char* kind = sizeof(T) == 2 ? "score_xl_bf16" : "score_xl_f32";
    if (imt_prof_enabled() && getenv("IMT_PROF_SHAPES")) kind = imt_prof_intern(kind, a->N, a->V, a->K);
    ImtProfScope prof(kind, 2.0 * a->N * a->V * a->K,
                      ((double)a->N * a->K + (double)a->V * a->K + a->V) * es + (double)a->N * (8.0 * ntile + 12.0), st);
    ImtTrace tr("score_xl", ntile * nrb, st);  // IMT_TRACE=score_xl: phases = first K tile landed | K loop | reduction | stores
    hipLaunchKernelGGL(kern, dim3(ntile * nrb), dim3(XL_THREADS), XL_LDS, st, reinterpret_cast<const T*>(a->x), a->ldx, x_bytes,
                       reinterpret_cast<const T*>(a->w), a->ldw, w_bytes, a->N, a->V, a->K, reinterpret_cast<const T*>(a->bias), a->target,
                       part, tlogit, tr.dev);
    IMT_CHECK_LAUNCH();
    if (tr.dev) fprintf(stderr, "[score_xl %s %dx%dx%d]\n", kind, a->N, a->V, a->K);
  }
  {
    const int n_seg = a->seg_offsets ? a->n_seg : 0;
    ImtProfScope prof("score_combine", 0.0, (double)a->N * (8.0 * ntile * (n_seg ? 2 : 1) + 20.0), st);
    hipLaunchKernelGGL(score_combine_kernel, dim3(nrb + n_seg), dim3(SCORE_ROWS), 0, st, part, tlogit, a->target, a->logprob, a->lse,
                       a->seg_offsets, a->seg_score, a->N, a->V, ntile, nrb, a->normalize);
    IMT_CHECK_LAUNCH();
  }
  return IMT_OK;
}

}  // namespace

extern "C" int64_t imt_score_ws_bytes(int N, int V) {
  if (N <= 0 || V <= 0) return 0;
  return imt_align256((int64_t)N * 4) + (int64_t)imt_cdiv(V, 256) * N * 8;
}

extern "C" int imt_score_supported(int dtype, int V, int K) {
  if (!imt_ok_dtype(dtype) || V <= 0 || K <= 0) return 0;
  const int es = imt_dtype_bytes(dtype);
  if (K % (128 / es) != 0) return 0;                              // whole K tiles (128 bytes of K)
  if ((int64_t)(V + 256) * K * es >= ((int64_t)1 << 31)) return 0;  // 32-bit DMA offsets over the weight, ragged tile included
  return 1;
}

extern "C" int imt_score_rows(const imt_score_args* a, void* stream) {
  IMT_CHECK_ARG(a != nullptr, "score_rows: null args");
  IMT_CHECK_ARG(imt_ok_dtype(a->dtype), "score_rows: bad dtype %d", a->dtype);
  IMT_CHECK_ARG(a->x != nullptr, "score_rows: x is null");
  IMT_CHECK_ARG(a->w != nullptr, "score_rows: w is null");
  IMT_CHECK_ARG(a->target != nullptr, "score_rows: target is null");
  IMT_CHECK_ARG(a->logprob != nullptr, "score_rows: logprob is null");
  IMT_CHECK_ARG(a->N > 0, "score_rows: N = %d must be positive", a->N);
  IMT_CHECK_ARG(a->V > 0, "score_rows: V = %d must be positive", a->V);
  IMT_CHECK_ARG(a->K > 0, "score_rows: K = %d must be positive", a->K);
  IMT_CHECK_ARG(a->ws != nullptr && a->ws_bytes >= imt_score_ws_bytes(a->N, a->V), "score_rows: ws_bytes = %lld is below imt_score_ws_bytes = %lld",
                (long long)(a->ws ? a->ws_bytes : 0), (long long)imt_score_ws_bytes(a->N, a->V));
  IMT_CHECK_ARG(imt_score_supported(a->dtype, a->V, a->K), "score_rows: (dtype %d, V %d, K %d) is not taken by the fused kernel (K must be a whole "
                "number of 128-byte K tiles)", a->dtype, a->V, a->K);
  const int es = imt_dtype_bytes(a->dtype);
  if (const int rc = xl_check_rows("score_rows", "x", "ldx", a->x, a->ldx, a->N, a->K, es)) return rc;
  if (const int rc = xl_check_rows("score_rows", "w", "ldw", a->w, a->ldw, a->V, a->K, es)) return rc;
  IMT_CHECK_ARG(!a->bias || (uintptr_t)a->bias % 16 == 0, "score_rows: bias must be 16-byte aligned");
  IMT_CHECK_ARG((uintptr_t)a->ws % 16 == 0, "score_rows: ws must be 16-byte aligned");
  if (a->seg_offsets) {
    IMT_CHECK_ARG(a->n_seg > 0 && a->n_seg <= (1 << 20), "score_rows: n_seg = %d with seg_offsets", a->n_seg);
    IMT_CHECK_ARG(a->seg_score != nullptr, "score_rows: seg_score is null with seg_offsets");
  }
  hipStream_t st = (hipStream_t)stream;
  return a->dtype == IMT_BF16 ? launch_score<bf16_t>(a, st) : launch_score<float>(a, st);
}
