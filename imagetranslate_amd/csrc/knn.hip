// k nearest neighbours by inner product (see include/imt_hip.h, imt_knn_rows): for every query row the k largest
// s[r, c] = x[r, :] . y[c, :] and their columns, WITHOUT ever storing the [N, M] similarities.
//
// knn_xl_kernel is gemm_xl_kernel's NT main loop (gemm_xl.hpp: 256 x 256 tile, two 64-KiB LDS-DMA stages, 8 waves as
// 2 (m) x 4 (n), acc[8][4] per wave), run by ONE workgroup over all column tiles of its column range (split), in ascending
// column order.  The workgroup keeps, per row, a list of the k best (value, column) seen so far, sorted by value descending
// then column ascending, in 16 KiB of LDS behind the two stages ([slot][row], so row t's k-th value -- the bar a newcomer has
// to beat -- is one conflict-free read).  After a tile's K loop:
//   1. select: lane (lr, lg) of wave (wmi, wni) holds, per 16-row group i, 16 products of row 128 wmi + 16 i + lr (columns
//      n0 + 64 wni + 16 j + 4 lg + e; columns >= M of the ragged last tile -> -inf: the DMA zero-filled them, and a 0 beats
//      every negative cosine).  A product is a candidate only if it is STRICTLY above the row's k-th value: columns arrive in
//      ascending order, so a tie with a listed entry loses.  No candidate in the wave (a wave-uniform ballot branch, the
//      usual case once the lists have warmed up): 16 compares and one 4-byte sentinel store per row group.  Otherwise up to
//      k rounds of (lane's best over 16, two xor-shuffles over the row's 4 lanes, strike the winner) write the wave's
//      candidates of the row, best first, into the free stage memory [wni][round][row];
//   2. merge: thread t inserts the candidates of row t into its list, waves in column order; a candidate goes BEHIND every
//      entry of equal value (its column is higher), so the order rule is total and the list does not depend on the split.
// At the end thread t stores row t's list to the workspace [row][split][k]; knn_combine_kernel merges the splits of a row
// in split (= column) order by the same insertion and adds index_base.  No atomics anywhere; two runs are bit-identical,
// and so are runs with different splits: every product comes from the same K loop wherever its tile runs.
#include <limits.h>
#include <math.h>
#include "gemm_xl.hpp"

namespace {

constexpr int KNN_ROWS = 256;                                // rows per workgroup of both kernels
constexpr int KNN_KMAX = IMT_KNN_MAX_K;
constexpr int KNN_LIST_BYTES = 2 * KNN_KMAX * KNN_ROWS * 4;  // values + columns, [slot][row]
constexpr int KNN_LDS = XL_LDS + KNN_LIST_BYTES;             // 144 KiB of the CU's 160
static_assert(2 * 4 * KNN_KMAX * KNN_ROWS * 4 <= XL_LDS, "the candidates of a tile live in the stage memory");

// (c, col) into row t's sorted list; the caller has checked c > lv[k - 1] (so it lands at or before the last slot).  Entries
// of equal value stay in front: they came from lower columns.
IMT_DEVICE void knn_insert(float* lv, int* li, int t, int k, float c, int col) {
  int p = k - 1;
  while (p > 0 && c > lv[(p - 1) * KNN_ROWS + t]) {
    lv[p * KNN_ROWS + t] = lv[(p - 1) * KNN_ROWS + t];
    li[p * KNN_ROWS + t] = li[(p - 1) * KNN_ROWS + t];
    --p;
  }
  lv[p * KNN_ROWS + t] = c;
  li[p * KNN_ROWS + t] = col;
}

template <bool RAGGED_M>
IMT_DEVICE void knn_tile_select(const f32x4 (&acc)[8][4], const float* lv, float* candv, int* candc, int n0, int wmi, int wni,
                                int M, int k) {
  const int lane = threadIdx.x & 63, lr = lane & 15, lg = lane >> 4;
  const int nl = n0 + 64 * wni + 4 * lg;  // first column of this lane's j = 0 quad
  float* cv = candv + wni * KNN_KMAX * KNN_ROWS;
  int* cc = candc + wni * KNN_KMAX * KNN_ROWS;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int rl = 128 * wmi + 16 * i + lr;
    const float bar = lv[(k - 1) * KNN_ROWS + rl];
    f32x4 v[4];
    bool any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = acc[i][j];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (RAGGED_M && nl + 16 * j + e >= M) v[j][e] = -INFINITY;
        any = any || v[j][e] > bar;
      }
    }
    if (__builtin_amdgcn_ballot_w64(any) == 0) {  // wave-uniform: nothing in these 16 rows x 64 columns beats its row's list
      if (lg == 0) cv[rl] = -INFINITY;
      continue;
    }
    for (int s = 0; s < k; ++s) {
      // the lane's best remaining candidate: first (= lowest column) among equals; INT_MAX marks "none"
      float bv = bar;
      int bc = INT_MAX;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (v[j][e] > bv) { bv = v[j][e]; bc = nl + 16 * j + e; }
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oc = __shfl_xor(bc, o, 64);
        if (ov > bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
      }
      const bool got = bc != INT_MAX;
      if (lg == 0) {
        cv[s * KNN_ROWS + rl] = got ? bv : -INFINITY;  // -inf ends the row's candidates of this wave
        cc[s * KNN_ROWS + rl] = bc;
      }
      if (__builtin_amdgcn_ballot_w64(got) == 0) break;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (nl + 16 * j + e == bc) v[j][e] = -INFINITY;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(XL_THREADS) void knn_xl_kernel(const T* __restrict__ X, int64_t ldx, int64_t x_bytes,
                                                            const T* __restrict__ Y, int64_t ldy, int64_t y_bytes, int N, int M,
                                                            int K, int k, int splits, float* __restrict__ pval,
                                                            int* __restrict__ pidx) {
  constexpr int BK = TileGeom<T, true>::BK;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ntile = (M + 255) / 256, nrb = (N + 255) / 256;
  const int bid = imt_xcd_block(blockIdx.x, nrb * splits);
  const int sp = bid % splits;
  const int m0 = (bid / splits) * 256;
  const int c0 = (int)((int64_t)sp * ntile / splits), c1 = (int)((int64_t)(sp + 1) * ntile / splits);  // may be empty
  const int nt = K / BK;  // whole K tiles (host-checked)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wmi = wave >> 2, wni = wave & 3, wn = (wni & 1) * 64;
  const bool loads_a = wave < 4;

  float* lv = reinterpret_cast<float*>(smem + XL_LDS);  // [k slots][256 rows]
  int* li = reinterpret_cast<int*>(smem + XL_LDS + KNN_LIST_BYTES / 2);
  float* candv = reinterpret_cast<float*>(smem);        // [4 waves wni][k rounds][256 rows], in the stages after a K loop
  int* candc = reinterpret_cast<int*>(smem + 4 * KNN_KMAX * KNN_ROWS * 4);
  for (int q = threadIdx.x; q < KNN_KMAX * KNN_ROWS; q += XL_THREADS) { lv[q] = -INFINITY; li[q] = -1; }
  __syncthreads();

  DmaPair<T> dma;
  if (loads_a) dma.template init<true>(X, ldx, x_bytes, m0, wave);
  auto issue = [&](int slot, int t) { dma.issue(smem + slot * XL_STAGE + (loads_a ? 0 : 2 * TILE_BYTES), t); };

  for (int ct = c0; ct < c1; ++ct) {
    const int n0 = ct * 256;
    if (!loads_a) dma.template init<true>(Y, ldy, y_bytes, n0, wave - 4);
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // A COPY of xl_k_loop (gemm_xl.hpp; same K order: the products are the ones imt_gemm would have produced in fp32), kept
    // because this kernel measured 1.5-3 % slower in bf16 through the shared function (207 against 203 VGPRs); keep the two alike
    issue(0, 0);
    for (int t = 0; t < nt; ++t) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_barrier" ::: "memory");
      const bool issue_now = t + 1 < nt;
      if (issue_now && wave < 4) issue((t + 1) & 1, t + 1);
      const char* st = smem + (t & 1) * XL_STAGE;
      compute_tile_xl<T, IMT_NT, 0>(acc, st + wmi * TILE_BYTES, st + (2 + (wni >> 1)) * TILE_BYTES, wn);
      if (issue_now && wave >= 4) issue((t + 1) & 1, t + 1);
      compute_tile_xl<T, IMT_NT, 1>(acc, st + wmi * TILE_BYTES, st + (2 + (wni >> 1)) * TILE_BYTES, wn);
    }
    __syncthreads();  // everyone has read the last stage: the stages are free for the candidates
    if (n0 + 256 > M) knn_tile_select<true>(acc, lv, candv, candc, n0, wmi, wni, M, k);
    else              knn_tile_select<false>(acc, lv, candv, candc, n0, wmi, wni, M, k);
    __syncthreads();
    if (threadIdx.x < KNN_ROWS) {
      const int t = threadIdx.x;
      for (int w = 0; w < 4; ++w)
        for (int s = 0; s < k; ++s) {
          const int q = (w * KNN_KMAX + s) * KNN_ROWS + t;
          const float c = candv[q];
          if (!(c > lv[(k - 1) * KNN_ROWS + t])) break;  // sentinel, or no better than the k-th: neither is the rest
          knn_insert(lv, li, t, k, c, candc[q]);
        }
    }
    __syncthreads();  // candidates consumed before the next tile's first DMA lands on them; the bars are up to date
  }

  if (threadIdx.x < KNN_ROWS && m0 + (int)threadIdx.x < N) {
    const int64_t o = ((int64_t)(m0 + threadIdx.x) * splits + sp) * k;
    for (int s = 0; s < k; ++s) {
      pval[o + s] = lv[s * KNN_ROWS + threadIdx.x];
      pidx[o + s] = li[s * KNN_ROWS + threadIdx.x];
    }
  }
}

// one thread per row: the splits' lists in split (= column) order through the same insertion
__global__ __launch_bounds__(KNN_ROWS) void knn_combine_kernel(const float* __restrict__ pval, const int* __restrict__ pidx,
                                                               float* __restrict__ val, int32_t* __restrict__ idx, int N, int k,
                                                               int splits, int index_base) {
  __shared__ float lv[KNN_KMAX * KNN_ROWS];
  __shared__ int li[KNN_KMAX * KNN_ROWS];
  const int t = threadIdx.x, row = blockIdx.x * KNN_ROWS + t;
  if (row >= N) return;
  for (int s = 0; s < k; ++s) { lv[s * KNN_ROWS + t] = -INFINITY; li[s * KNN_ROWS + t] = -1; }
  for (int sp = 0; sp < splits; ++sp) {
    const int64_t o = ((int64_t)row * splits + sp) * k;
    for (int s = 0; s < k; ++s) {
      const float c = pval[o + s];
      if (!(c > lv[(k - 1) * KNN_ROWS + t])) break;
      knn_insert(lv, li, t, k, c, pidx[o + s]);
    }
  }
  for (int s = 0; s < k; ++s) {
    const int c = li[s * KNN_ROWS + t];
    val[(int64_t)row * k + s] = lv[s * KNN_ROWS + t];
    idx[(int64_t)row * k + s] = c >= 0 ? c + index_base : -1;
  }
}

// enough (row block, split) workgroups for the chip's 256 CUs, never more splits than column tiles
int knn_pick_splits(int N, int M) {
  const int nrb = imt_cdiv(N, 256), ntile = imt_cdiv(M, 256);
  int s = imt_cdiv(256, nrb);
  if (s > ntile) s = ntile;
  if (s > IMT_KNN_MAX_SPLITS) s = IMT_KNN_MAX_SPLITS;
  return s < 1 ? 1 : s;
}

template <typename T> int launch_knn(const imt_knn_args* a, int splits, hipStream_t st) {
  auto kern = knn_xl_kernel<T>;
  static const bool lds_ok = allow_lds(kern, KNN_LDS);
  IMT_CHECK_LDS(lds_ok, "knn_rows", KNN_LDS);
  const int nrb = imt_cdiv(a->N, 256), ntile = imt_cdiv(a->M, 256);
  const int64_t cells = (int64_t)a->N * splits * a->k;
  float* pval = reinterpret_cast<float*>(a->ws);
  int* pidx = reinterpret_cast<int*>(reinterpret_cast<char*>(a->ws) + imt_align256(cells * 4));
  const int64_t x_bytes = view_bytes(a->N, a->ldx, a->K, sizeof(T)), y_bytes = view_bytes(a->M, a->ldy, a->K, sizeof(T));
  const double es = sizeof(T);
  {
    const char* kind = sizeof(T) == 2 ? "knn_xl_bf16" : "knn_xl_f32";
    if (imt_prof_enabled() && getenv("IMT_PROF_SHAPES")) kind = imt_prof_intern(kind, a->N, a->M, a->K);
    ImtProfScope prof(kind, 2.0 * a->N * a->M * a->K,
                      ((double)nrb * a->M * a->K + (double)ntile * a->N * a->K) * es + (double)cells * 8.0, st);
    hipLaunchKernelGGL(kern, dim3(nrb * splits), dim3(XL_THREADS), KNN_LDS, st, reinterpret_cast<const T*>(a->x), a->ldx, x_bytes,
                       reinterpret_cast<const T*>(a->y), a->ldy, y_bytes, a->N, a->M, a->K, a->k, splits, pval, pidx);
    IMT_CHECK_LAUNCH();
  }
  {
    ImtProfScope prof("knn_combine", 0.0, (double)cells * 8.0 + (double)a->N * a->k * 8.0, st);
    hipLaunchKernelGGL(knn_combine_kernel, dim3(nrb), dim3(KNN_ROWS), 0, st, pval, pidx, a->val, a->idx, a->N, a->k, splits,
                       a->index_base);
    IMT_CHECK_LAUNCH();
  }
  return IMT_OK;
}

}  // namespace

extern "C" int64_t imt_knn_ws_bytes(int N, int M, int k, int splits) {
  if (N <= 0 || M <= 0 || k <= 0 || k > IMT_KNN_MAX_K || splits < 0 || splits > IMT_KNN_MAX_SPLITS) return 0;
  if (splits == 0) splits = knn_pick_splits(N, M);
  const int64_t cells = (int64_t)N * splits * k;
  return imt_align256(cells * 4) + cells * 4;
}

extern "C" int imt_knn_supported(int dtype, int K) {
  if (!imt_ok_dtype(dtype) || K <= 0) return 0;
  return K % (128 / imt_dtype_bytes(dtype)) == 0;  // whole K tiles (128 bytes of K)
}

extern "C" int imt_knn_rows(const imt_knn_args* a, void* stream) {
  IMT_CHECK_ARG(a != nullptr, "knn_rows: null args");
  IMT_CHECK_ARG(imt_ok_dtype(a->dtype), "knn_rows: bad dtype %d", a->dtype);
  IMT_CHECK_ARG(a->x != nullptr, "knn_rows: x is null");
  IMT_CHECK_ARG(a->y != nullptr, "knn_rows: y is null");
  IMT_CHECK_ARG(a->val != nullptr, "knn_rows: val is null");
  IMT_CHECK_ARG(a->idx != nullptr, "knn_rows: idx is null");
  IMT_CHECK_ARG(a->N > 0, "knn_rows: N = %d must be positive", a->N);
  IMT_CHECK_ARG(a->M > 0, "knn_rows: M = %d must be positive", a->M);
  IMT_CHECK_ARG(a->K > 0, "knn_rows: K = %d must be positive", a->K);
  IMT_CHECK_ARG(a->k >= 1 && a->k <= IMT_KNN_MAX_K, "knn_rows: k = %d outside 1..%d", a->k, IMT_KNN_MAX_K);
  IMT_CHECK_ARG(a->splits >= 0 && a->splits <= IMT_KNN_MAX_SPLITS, "knn_rows: splits = %d outside 0..%d", a->splits, IMT_KNN_MAX_SPLITS);
  IMT_CHECK_ARG(imt_knn_supported(a->dtype, a->K), "knn_rows: (dtype %d, K %d) is not taken (K must be a whole number of 128-byte K tiles)",
                a->dtype, a->K);
  const int es = imt_dtype_bytes(a->dtype);
  if (const int rc = xl_check_rows("knn_rows", "x", "ldx", a->x, a->ldx, a->N, a->K, es)) return rc;
  if (const int rc = xl_check_rows("knn_rows", "y", "ldy", a->y, a->ldy, a->M, a->K, es)) return rc;
  IMT_CHECK_ARG(a->index_base >= 0 && (int64_t)a->index_base + a->M <= (int64_t)INT32_MAX, "knn_rows: index_base = %d with M = %d leaves int32",
                a->index_base, a->M);
  const int64_t need = imt_knn_ws_bytes(a->N, a->M, a->k, a->splits);
  IMT_CHECK_ARG(a->ws != nullptr && a->ws_bytes >= need, "knn_rows: ws_bytes = %lld is below imt_knn_ws_bytes = %lld",
                (long long)(a->ws ? a->ws_bytes : 0), (long long)need);
  IMT_CHECK_ARG((uintptr_t)a->ws % 16 == 0, "knn_rows: ws must be 16-byte aligned");
  const int splits = a->splits ? a->splits : knn_pick_splits(a->N, a->M);
  hipStream_t st = (hipStream_t)stream;
  return a->dtype == IMT_BF16 ? launch_knn<bf16_t>(a, splits, st) : launch_knn<float>(a, splits, st);
}
