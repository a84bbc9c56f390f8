// Word alignment of sentence pairs by embedding similarity, "argmax / intersection" (see include/imt_hip.h, imt_align_pairs):
// per pair b the cosine of every (source token, target token) of the pair's ranges, the arg-max of every row and of every
// column, and the mutual links -- WITHOUT storing the [B, S, T] similarities or a normalised copy of either operand.
//
// One workgroup (4 waves) owns a pair and walks its ranges in 64 x 64 tiles, row blocks outside, column tiles inside, both
// counted from the range's begin (a tagged sentence of 66 tokens is one tile, not two).  Per tile:
//   1. K loop over d in steps of 128 bytes: thread t brings 16 bytes of two rows of each operand into registers (rows past
//      the range's end: zeros, so nothing outside x / y is ever addressed), adds their squares to its running sums -- the
//      norms come from the very values that are staged -- and writes them to one of two swizzled LDS stages; one barrier per
//      step, the next step's loads are in flight under the MFMAs.  Wave w holds source rows 16 w .. 16 w + 15 of the block
//      against the tile's 64 columns: acc[nt] is D[target 16 nt + 4 g + e][source r] of mma.hpp's lane (r, g).
//   2. the 8 threads of a row add up their squares (xor-shuffles, a fixed order) and leave max(sqrt, 1e-12) in LDS.
//   3. select: sim = acc / (|x| |y|), -inf outside the ranges.  Forward: the lane's best of 16 columns (ascending, strict >),
//      then the row's 4 lanes by (value desc, column asc), then against the row's running best of the earlier column tiles
//      (strict >: the lowest column of equal value stays).  Backward: every column's best over the wave's 16 rows by the
//      same order (4 xor-shuffles), to LDS per wave; thread j then folds the 4 waves, in row order, into the pair's running
//      column maxima (strict > again, and row blocks arrive in ascending order).
// At the end thread i writes fwd / link of position i and thread j bwd of position j: the mutual test reads the finished
// column maxima from LDS.  Everything a pair needs is in its own workgroup, so its outputs depend neither on B nor on its
// neighbours, and no order of arrival enters any result: two calls give the same bits.
#include <limits.h>
#include <math.h>
#include "mma.hpp"

namespace {

constexpr int AL_TILE = 64;                    // rows and columns of a tile
constexpr int AL_RB = 128;                     // bytes of d per staged step (one swizzled LDS row)
constexpr int AL_THREADS = 256;
constexpr int AL_MAX = IMT_ALIGN_MAX_LEN;
constexpr int AL_TILE_BYTES = AL_TILE * AL_RB;  // 8 KiB per operand per stage
// LDS of a workgroup: 2 stages x 2 operands x 8 KiB + 4 x 2 KiB of running maxima + 2.5 KiB of norms and wave candidates
// = 42.5 KiB: three workgroups per CU within its 160 KiB.
static_assert(4 * AL_TILE_BYTES + 4 * AL_MAX * 4 + 2 * AL_TILE * 4 + 8 * AL_TILE * 4 <= 48 * 1024, "three workgroups per CU");

struct AlignP {
  const void* x; int64_t ldx, bsx;
  const void* y; int64_t ldy, bsy;
  const int32_t* xr; const int32_t* yr;
  int S, T, d;
  float min_sim;
  int32_t* link; int32_t* fwd_idx; float* fwd_val; int32_t* bwd_idx; float* bwd_val;
};

template <typename T> IMT_DEVICE float sumsq16(u32x4 v);
template <> IMT_DEVICE float sumsq16<float>(u32x4 v) {
  const f32x4 f = __builtin_bit_cast(f32x4, v);
  return fmaf(f[3], f[3], fmaf(f[2], f[2], fmaf(f[1], f[1], f[0] * f[0])));
}
template <> IMT_DEVICE float sumsq16<bf16_t>(u32x4 v) {
  const bf16x8 h = __builtin_bit_cast(bf16x8, v);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s = fmaf((float)h[j], (float)h[j], s);
  return s;
}

IMT_DEVICE int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <typename T>
__global__ __launch_bounds__(AL_THREADS) void align_kernel(AlignP p) {
  constexpr int EPC = 16 / sizeof(T), KC = AL_RB / sizeof(T);
  __shared__ __attribute__((aligned(16))) char stage[2][2][AL_TILE_BYTES];  // [stage][x | y]
  __shared__ float fwd_v[AL_MAX], bwd_v[AL_MAX];
  __shared__ int fwd_i[AL_MAX], bwd_i[AL_MAX];
  __shared__ float xn[AL_TILE], yn[AL_TILE];
  __shared__ float cand_v[4][AL_TILE];
  __shared__ int cand_i[4][AL_TILE];

  const int b = blockIdx.x, tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int xb = clampi(p.xr[2 * b], 0, p.S), xe = clampi(p.xr[2 * b + 1], xb, p.S);
  const int yb = clampi(p.yr[2 * b], 0, p.T), ye = clampi(p.yr[2 * b + 1], yb, p.T);
  const T* X = reinterpret_cast<const T*>(p.x) + (int64_t)b * p.bsx;
  const T* Y = reinterpret_cast<const T*>(p.y) + (int64_t)b * p.bsy;
  const int nk = p.d / KC;  // whole steps (host-checked)

  for (int q = tid; q < AL_MAX; q += AL_THREADS) {
    fwd_v[q] = -INFINITY; bwd_v[q] = -INFINITY;
    fwd_i[q] = -1; bwd_i[q] = -1;
  }
  __syncthreads();

  // this thread's part of a staged step: 16-byte chunk sc of tile rows sr and sr + 32, of both operands
  const int sr = tid >> 3, sc = tid & 7;

  for (int r0 = xb; r0 < xe; r0 += AL_TILE) {
    const int i = r0 + 16 * wave + r;  // this lane's source position
    float run_v = -INFINITY;
    int run_i = -1;
    for (int c0 = yb; c0 < ye; c0 += AL_TILE) {
      f32x4 acc[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      float ssx[2] = {0.f, 0.f}, ssy[2] = {0.f, 0.f};
      u32x4 rx[2], ry[2];
      auto fetch = [&](int t) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int xrow = r0 + sr + 32 * u, yrow = c0 + sr + 32 * u;
          rx[u] = u32x4{0u, 0u, 0u, 0u};
          ry[u] = u32x4{0u, 0u, 0u, 0u};
          if (xrow < xe) rx[u] = *reinterpret_cast<const u32x4*>(X + (int64_t)xrow * p.ldx + (int64_t)t * KC + sc * EPC);
          if (yrow < ye) ry[u] = *reinterpret_cast<const u32x4*>(Y + (int64_t)yrow * p.ldy + (int64_t)t * KC + sc * EPC);
        }
      };
      fetch(0);
      for (int t = 0; t < nk; ++t) {
        char* sx = stage[t & 1][0];
        char* sy = stage[t & 1][1];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          *reinterpret_cast<u32x4*>(sx + tile_off<AL_RB>(sr + 32 * u, sc)) = rx[u];
          *reinterpret_cast<u32x4*>(sy + tile_off<AL_RB>(sr + 32 * u, sc)) = ry[u];
          ssx[u] += sumsq16<T>(rx[u]);
          ssy[u] += sumsq16<T>(ry[u]);
        }
        // one barrier per step: stage t & 1 was last read in step t - 2, which every wave left before the barrier of t - 1
        __syncthreads();
        if (t + 1 < nk) fetch(t + 1);
#pragma unroll
        for (int ks = 0; ks < AL_RB / 64; ++ks) {
          const typename Frag<T>::type xf = lds_frag_kcontig<T, AL_RB>(sx, 16 * wave, 4 * ks);
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) mma16(acc[nt], lds_frag_kcontig<T, AL_RB>(sy, 16 * nt, 4 * ks), xf);
        }
      }
      // norms: the 8 threads of a row (consecutive lanes) in a fixed order
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
          ssx[u] += __shfl_xor(ssx[u], o, 64);
          ssy[u] += __shfl_xor(ssy[u], o, 64);
        }
        if (sc == 0) {
          xn[sr + 32 * u] = fmaxf(sqrtf(ssx[u]), 1e-12f);
          yn[sr + 32 * u] = fmaxf(sqrtf(ssy[u]), 1e-12f);
        }
      }
      __syncthreads();  // norms visible; every wave has left the K loop (the stages are free for the next tile)

      const float nx = xn[16 * wave + r];
      const bool row_ok = i < xe;
      float bv = -INFINITY;
      int bj = INT_MAX;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int jl = 16 * nt + 4 * g + e, j = c0 + jl;
          const float s = (row_ok && j < ye) ? acc[nt][e] / (nx * yn[jl]) : -INFINITY;
          if (s > bv) { bv = s; bj = j; }
          // backward: this column's best over the wave's 16 rows
          float cv = s;
          int ci = s > -INFINITY ? i : INT_MAX;
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) {
            const float ov = __shfl_xor(cv, o, 64);
            const int oi = __shfl_xor(ci, o, 64);
            if (better(ov, oi, cv, ci)) { cv = ov; ci = oi; }
          }
          if (r == 0) { cand_v[wave][jl] = cv; cand_i[wave][jl] = ci; }
        }
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (better(ov, oj, bv, bj)) { bv = ov; bj = oj; }
      }
      if (bv > run_v) { run_v = bv; run_i = bj; }
      __syncthreads();  // the waves' column candidates are in LDS
      if (tid < AL_TILE && c0 + tid < ye) {
        const int j = c0 + tid;
        float v = bwd_v[j];
        int bi = bwd_i[j];
#pragma unroll
        for (int w = 0; w < 4; ++w)
          if (cand_v[w][tid] > v) { v = cand_v[w][tid]; bi = cand_i[w][tid]; }
        bwd_v[j] = v;
        bwd_i[j] = bi;
      }
      // (the next tile's K loop has a barrier between this read of the candidates / norms and their next writes)
    }
    if (g == 0 && i < xe) { fwd_v[i] = run_v; fwd_i[i] = run_i; }
  }
  __syncthreads();

  for (int q = tid; q < p.S; q += AL_THREADS) {
    const int fi = fwd_i[q];
    const float fv = fwd_v[q];
    const int64_t o = (int64_t)b * p.S + q;
    p.fwd_idx[o] = fi;
    p.fwd_val[o] = fv;
    p.link[o] = (fi >= 0 && bwd_i[fi] == q && fv >= p.min_sim) ? fi : -1;
  }
  for (int q = tid; q < p.T; q += AL_THREADS) {
    const int64_t o = (int64_t)b * p.T + q;
    p.bwd_idx[o] = bwd_i[q];
    p.bwd_val[o] = bwd_v[q];
  }
}

// elements from a pair's first to past its last: (rows - 1) * ld + d; false on 64-bit overflow
bool align_pair_extent(int rows, int d, int64_t ld, int64_t* out) {
  int64_t c;
  return !__builtin_mul_overflow((int64_t)(rows - 1), ld, &c) && !__builtin_add_overflow(c, (int64_t)d, out);
}
// ((B - 1) * bs + extent) * element size, the byte offset past the view's end, must fit in 63 bits
bool align_view_ok(int B, int64_t bs, int64_t extent, int es) {
  int64_t a, e;
  return !__builtin_mul_overflow((int64_t)(B - 1), bs, &a) && !__builtin_add_overflow(a, extent, &e) &&
         !__builtin_mul_overflow(e, (int64_t)es, &e);
}

}  // namespace

extern "C" int imt_align_supported(int dtype, int d) {
  if (!imt_ok_dtype(dtype) || d <= 0) return 0;
  return d % (AL_RB / imt_dtype_bytes(dtype)) == 0;
}

extern "C" int imt_align_pairs(const imt_align_args* a, void* stream) {
  IMT_CHECK_ARG(a != nullptr, "align_pairs: null args");
  IMT_CHECK_ARG(imt_ok_dtype(a->dtype), "align_pairs: bad dtype %d", a->dtype);
  IMT_CHECK_ARG(a->x != nullptr, "align_pairs: x is null");
  IMT_CHECK_ARG(a->y != nullptr, "align_pairs: y is null");
  IMT_CHECK_ARG(a->xr != nullptr, "align_pairs: xr is null");
  IMT_CHECK_ARG(a->yr != nullptr, "align_pairs: yr is null");
  IMT_CHECK_ARG(a->link != nullptr, "align_pairs: link is null");
  IMT_CHECK_ARG(a->fwd_idx != nullptr && a->fwd_val != nullptr, "align_pairs: fwd_idx / fwd_val is null");
  IMT_CHECK_ARG(a->bwd_idx != nullptr && a->bwd_val != nullptr, "align_pairs: bwd_idx / bwd_val is null");
  IMT_CHECK_ARG(a->B > 0, "align_pairs: B = %d must be positive", a->B);
  IMT_CHECK_ARG(a->S >= 1 && a->S <= IMT_ALIGN_MAX_LEN, "align_pairs: S = %d outside 1..%d", a->S, IMT_ALIGN_MAX_LEN);
  IMT_CHECK_ARG(a->T >= 1 && a->T <= IMT_ALIGN_MAX_LEN, "align_pairs: T = %d outside 1..%d", a->T, IMT_ALIGN_MAX_LEN);
  IMT_CHECK_ARG(imt_align_supported(a->dtype, a->d), "align_pairs: (dtype %d, d %d) is not taken (d must be a whole number of 128-byte steps)",
                a->dtype, a->d);
  const int es = imt_dtype_bytes(a->dtype), epv = 16 / es;
  IMT_CHECK_ARG(a->ldx >= a->d && a->ldy >= a->d, "align_pairs: ldx = %lld / ldy = %lld below d = %d", (long long)a->ldx, (long long)a->ldy, a->d);
  IMT_CHECK_ARG(a->ldx % epv == 0 && a->bsx % epv == 0 && (uintptr_t)a->x % 16 == 0, "align_pairs: x / ldx / bsx must keep rows 16-byte aligned");
  IMT_CHECK_ARG(a->ldy % epv == 0 && a->bsy % epv == 0 && (uintptr_t)a->y % 16 == 0, "align_pairs: y / ldy / bsy must keep rows 16-byte aligned");
  int64_t ex = 0, ey = 0;
  IMT_CHECK_ARG(align_pair_extent(a->S, a->d, a->ldx, &ex) && align_pair_extent(a->T, a->d, a->ldy, &ey),
                "align_pairs: a pair of x / y overflows 64-bit offsets");
  IMT_CHECK_ARG(a->bsx >= ex, "align_pairs: bsx = %lld below the extent of a pair (S = %d, ldx = %lld)", (long long)a->bsx, a->S,
                (long long)a->ldx);
  IMT_CHECK_ARG(a->bsy >= ey, "align_pairs: bsy = %lld below the extent of a pair (T = %d, ldy = %lld)", (long long)a->bsy, a->T,
                (long long)a->ldy);
  IMT_CHECK_ARG(align_view_ok(a->B, a->bsx, ex, es) && align_view_ok(a->B, a->bsy, ey, es),
                "align_pairs: x / y views overflow 64-bit byte offsets");
  AlignP p;
  p.x = a->x; p.ldx = a->ldx; p.bsx = a->bsx;
  p.y = a->y; p.ldy = a->ldy; p.bsy = a->bsy;
  p.xr = a->xr; p.yr = a->yr;
  p.S = a->S; p.T = a->T; p.d = a->d;
  p.min_sim = a->min_sim;
  p.link = a->link; p.fwd_idx = a->fwd_idx; p.fwd_val = a->fwd_val; p.bwd_idx = a->bwd_idx; p.bwd_val = a->bwd_val;
  hipStream_t st = (hipStream_t)stream;
  return imt_by_dtype(a->dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    const double es_d = sizeof(T);
    ImtProfScope prof(sizeof(T) == 2 ? "align_bf16" : "align_f32", 2.0 * a->B * a->S * a->T * a->d,
                      (double)a->B * ((double)a->S + a->T) * a->d * es_d + (double)a->B * (12.0 * a->S + 8.0 * a->T), st);
    hipLaunchKernelGGL(align_kernel<T>, dim3(a->B), dim3(AL_THREADS), 0, st, p);
    IMT_CHECK_LAUNCH();
    return (int)IMT_OK;
  });
}
