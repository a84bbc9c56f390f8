// Fused multi-head attention forward / backward (HF BertSelfAttention semantics):
//   P = softmax(Q K^T * scale + (1 - mask) * -10000) ; [dropout] ; O = P V
// Flash-style: the [Tq,Tk] score matrix never reaches HBM; forward saves one log-sum-exp per query row,
// backward recomputes P from it.
//
// Layout of the work (wave64, 16x16 MFMA tiles, see mma.hpp):
//   fwd / dQ  : one workgroup = 64 query rows of one (batch, head); each of its 4 waves owns 16 queries with
//               the QUERY on the MFMA lane (S^T = K Q^T), so row max / row sum / rescale are lane-local plus
//               two cross-lane shuffles, and the S^T accumulators are directly the B operand of
//               O^T = V^T P^T (resp. dQ^T = K^T dS^T).  K/V tiles of 64 keys are staged in swizzled LDS;
//               V (resp. K) is consumed through the transposed LDS read.
//   dK/dV     : one workgroup = 64 keys; KEY on the lane (S = Q K^T), dV^T / dK^T accumulate in registers over
//               all query tiles; Q and dO tiles are staged once and read both row-wise and transposed.
// Nothing is summed across workgroups: no atomics, bitwise reproducible.
#include <stdlib.h>
#include <type_traits>
#include "mma.hpp"

namespace {

struct AttnP {
  int B, H, Tq, Tk;
  const void* Q; int64_t ldq;
  const void* K; int64_t ldk;
  const void* V; int64_t ldv;
  void* O; int64_t ldo;
  float* lse;
  const uint8_t* key_mask;
  const uint8_t* query_mask;
  const uint8_t* mask3d;
  int causal;
  float scale;
  uint32_t drop_thresh; float inv_keep; uint64_t seed;
  const void* dO; int64_t lddo;
  void* dQ; int64_t lddq;
  void* dK; int64_t lddk;
  void* dV; int64_t lddv;
  unsigned long long* trace;  // tuning only (IMT_TRACE)
  float* delta;
};

// stage a [64 rows][DH] tile (rows row0.. of one (b,h)) into swizzled LDS, zero-filling rows >= nrows
template <typename T, int DH>
IMT_DEVICE void stage_tile(char* tile, const T* base, int64_t ld, int row0, int nrows) {
  constexpr int RB = DH * sizeof(T), CPR = RB / 16, EPC = 16 / sizeof(T);
  // (Kept as a loop with the load under its bounds test: hoisting all loads of a tile into registers, as the short-sequence
  // kernels do in their prologues, costs the register-bound dK/dV kernel 200 spilled registers -- C4 2.1 -> 2.8 ms.)
  for (int q = threadIdx.x; q < 64 * CPR; q += 256) {
    const int tr = q / CPR, c = q % CPR;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row0 + tr < nrows) v = *reinterpret_cast<const u32x4*>(base + (int64_t)(row0 + tr) * ld + c * EPC);
    *reinterpret_cast<u32x4*>(tile + tile_off<RB>(tr, c)) = v;
  }
}

// load NS register fragments of row (row0 + lane&15) straight from global (K-contiguous operand)
template <typename T, int DH>
IMT_DEVICE void load_row_frags(typename Frag<T>::type (&f)[DH * sizeof(T) / 64], const T* base, int64_t ld, int row0,
                               int nrows) {
  constexpr int NS = DH * sizeof(T) / 64, EPC = 16 / sizeof(T);
  const int l = threadIdx.x & 63, r = l & 15, g = l >> 4;
  typedef typename Frag<T>::type frag_t;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    const u32x4 v = *reinterpret_cast<const u32x4*>(base + (int64_t)min(row0 + r, nrows - 1) * ld + (4 * s + g) * EPC);
    f[s] = __builtin_bit_cast(frag_t, (row0 + r < nrows) ? v : z);  // unconditional load + select (see stage_tile)
  }
}

// MASK3D = false: the kernel instance for launches without an explicit [B, Tq, Tk] mask -- the per-element test of the
// pointer is a branch + exec save/restore + wait skeleton around a global load, ~10 scalar instructions per element
// even when the pointer is null.
template <bool MASK3D = true>
IMT_DEVICE bool mask_ok(const AttnP& p, int b, int i, int j, bool key_ok, bool query_ok) {
  bool ok = key_ok && query_ok;
  if (p.causal) ok = ok && (j <= i);
  if (MASK3D) {
    if (p.mask3d && i < p.Tq && j < p.Tk) ok = ok && (p.mask3d[((int64_t)b * p.Tq + i) * p.Tk + j] != 0);
  }
  return ok;
}
// Dropout of the attention probabilities: attn_drop_word / attn_drop_keep (common.hpp) -- one finaliser call per PAIR of
// neighbouring keys of a query; pair index = ((b*H + h)*Tq + i) * ceil(Tk/2) + (j >> 1).
IMT_DEVICE uint64_t attn_pair_row(const AttnP& p, int b, int h, int i) {
  return ((uint64_t)(b * p.H + h) * (uint64_t)p.Tq + (uint64_t)i) * (uint64_t)((p.Tk + 1) >> 1);
}

// accumulator tiles -> operand fragments of the following product (see mma.hpp, "permuted-K")
template <typename T> struct AccOperand;
template <> struct AccOperand<float> {
  static constexpr int NFR = 4;  // one fragment per 16-row tile
  static IMT_DEVICE f32x4 get(const f32x4 (&t)[4], int u) { return t[u]; }
  template <int RB> static IMT_DEVICE f32x4 lds(const char* tile, int u, int col0) { return lds_frag_kperm_f32<RB>(tile, 16 * u, col0); }
};
template <> struct AccOperand<bf16_t> {
  static constexpr int NFR = 2;  // one fragment per PAIR of 16-row tiles
  static IMT_DEVICE bf16x8 get(const f32x4 (&t)[4], int u) { return acc_pair_to_frag(t[2 * u], t[2 * u + 1]); }
  template <int RB> static IMT_DEVICE bf16x8 lds(const char* tile, int u, int col0) { return lds_frag_kperm_bf16<RB>(tile, 32 * u, col0); }
};

// =========================================================================================== forward
template <typename T, int DH, bool MASK3D>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 4 : 3) void attn_fwd_kernel(AttnP p) {
  constexpr int RB = DH * sizeof(T), NS = RB / 64, NDT = DH / 16;
  typedef typename Frag<T>::type frag_t;
  constexpr int NSUB = (RB > 128) ? 1 : 2;  // 64-row sub-tiles staged per barrier pair (LDS budget)
  __shared__ __attribute__((aligned(16))) char Ks[NSUB][64 * RB];
  __shared__ __attribute__((aligned(16))) char Vs[NSUB][64 * RB];
  __shared__ uint8_t kmask_s[NSUB * 64];

  const int nqt = (p.Tq + 63) / 64;
  const int lid = imt_xcd_block(blockIdx.x, gridDim.x);  // batch-major: XCD x owns batches [x*B/8, (x+1)*B/8)
  const int b = lid / (p.H * nqt), h = (lid / nqt) % p.H, tile_x = lid % nqt;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int q0 = tile_x * 64 + wave * 16;
  const int i = q0 + r;  // this lane's query row
  const T* Qb = reinterpret_cast<const T*>(p.Q) + (int64_t)b * p.Tq * p.ldq + h * DH;
  const T* Kb = reinterpret_cast<const T*>(p.K) + (int64_t)b * p.Tk * p.ldk + h * DH;
  const T* Vb = reinterpret_cast<const T*>(p.V) + (int64_t)b * p.Tk * p.ldv + h * DH;

  frag_t qf[NS];
  load_row_frags<T, DH>(qf, Qb, p.ldq, q0, p.Tq);
  const bool query_ok = (p.query_mask && i < p.Tq) ? (p.query_mask[(int64_t)b * p.Tq + i] != 0) : true;

  f32x4 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  const int nkt = (p.Tk + 63) / 64;
  for (int kt0 = 0; kt0 < nkt; kt0 += NSUB) {
    __syncthreads();  // previous tiles fully consumed
    // all the loads of up to NSUB key tiles (K, V, mask) are in flight together: one memory round trip per 128 keys
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
      if (kt0 + sub < nkt) {
        stage_tile<T, DH>(Ks[sub], Kb, p.ldk, (kt0 + sub) * 64, p.Tk);
        stage_tile<T, DH>(Vs[sub], Vb, p.ldv, (kt0 + sub) * 64, p.Tk);
      }
    }
    if (threadIdx.x < NSUB * 64) {
      const int j = kt0 * 64 + threadIdx.x;
      kmask_s[threadIdx.x] = (j < p.Tk) ? (p.key_mask ? p.key_mask[(int64_t)b * p.Tk + j] : (uint8_t)1) : (uint8_t)0;
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
    const int kt = kt0 + sub;
    if (kt >= nkt) break;
    const char* Kt = Ks[sub];
    const char* Vt = Vs[sub];
    const uint8_t* kmask_t = kmask_s + 64 * sub;

    // S^T tiles: rows <- keys (16 per tile), cols <- this wave's 16 queries
    f32x4 s[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      s[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NS; ++ks) mma16(s[nt], lds_frag_kcontig<T, RB>(Kt, 16 * nt, 4 * ks), qf[ks]);
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int jl = 16 * nt + 4 * g + e, j = kt * 64 + jl;
        float v = s[nt][e] * p.scale + (mask_ok<MASK3D>(p, b, i, j, kmask_t[jl] != 0, query_ok) ? 0.f : -10000.0f);
        if (j >= p.Tk) v = -INFINITY;
        s[nt][e] = v;
        tmax = fmaxf(tmax, v);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m_run, tmax);
    const float alpha = __expf(m_run - m_new);
    m_run = m_new;
    float psum = 0.f;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float pv = __expf(s[nt][e] - m_new);
        psum += pv;
        s[nt][e] = pv;
      }
    if (p.drop_thresh) {
      const uint32_t key = dropout_key(p.seed);
      const uint64_t prow = attn_pair_row(p, b, h, i) + (uint64_t)((kt * 64 + 4 * g) >> 1);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int e2 = 0; e2 < 2; ++e2) {  // keys 16nt + 4g + 2e2, +1: one pair
          const uint32_t w = attn_drop_word(key, prow + 8 * nt + e2);
          s[nt][2 * e2] = (w & 0xffffu) >= p.drop_thresh ? s[nt][2 * e2] * p.inv_keep : 0.f;
          s[nt][2 * e2 + 1] = (w >> 16) >= p.drop_thresh ? s[nt][2 * e2 + 1] * p.inv_keep : 0.f;
        }
    }
    l_run = l_run * alpha + psum;  // per-lane partial; lanes r, r+16, r+32, r+48 are combined at the end
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) o[dt] *= alpha;
    // O^T[d][m] += V^T[d][key] P^T[key][m]
#pragma unroll
    for (int u = 0; u < AccOperand<T>::NFR; ++u) {
      const frag_t pf = AccOperand<T>::get(s, u);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) mma16(o[dt], AccOperand<T>::template lds<RB>(Vt, u, 16 * dt), pf);
    }
    }  // sub
  }
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  const float inv_l = 1.0f / l_run;
  if (i < p.Tq) {
    T* Ob = reinterpret_cast<T*>(p.O) + ((int64_t)b * p.Tq + i) * p.ldo + h * DH;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) Vec4<T>::store(Ob + 16 * dt + 4 * g, o[dt] * inv_l);
    if (g == 0 && p.lse) p.lse[((int64_t)b * p.H + h) * p.Tq + i] = m_run + __logf(l_run);
  }
}

// =========================================================================================== forward, short sequences
// Tq, Tk <= 128, bf16: one workgroup (8 waves, 16 queries each) per (batch, head).  K and V are staged ONCE for all
// 128 queries (the 64-query kernel above stages them once per query tile), and with every key resident the softmax is
// a single pass: all S^T tiles, one max, one exp/sum, then O^T = V^T P^T -- no running rescale.
template <int DH, bool MASK3D>
__global__ __launch_bounds__(512, 4) void attn_fwd_short_kernel(AttnP p) {
  typedef bf16_t T;
  constexpr int RB = DH * 2, NS = RB / 64, NDT = DH / 16;
  typedef typename Frag<T>::type frag_t;
  __shared__ __attribute__((aligned(16))) char Ks[128 * RB];
  __shared__ __attribute__((aligned(16))) char Vs[128 * RB];
  __shared__ uint8_t kmask_s[128];
  const int lid = imt_xcd_block(blockIdx.x, gridDim.x);
  const int b = lid / p.H, h = lid % p.H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int q0 = wave * 16, i = q0 + r;
  const T* Qb = reinterpret_cast<const T*>(p.Q) + (int64_t)b * p.Tq * p.ldq + h * DH;
  const T* Kb = reinterpret_cast<const T*>(p.K) + (int64_t)b * p.Tk * p.ldk + h * DH;
  const T* Vb = reinterpret_cast<const T*>(p.V) + (int64_t)b * p.Tk * p.ldv + h * DH;
  // every global load of the kernel is requested here, unconditionally (clamped rows, a valid stand-in address for an
  // absent mask) and before the first use: ONE memory round trip in front of the barrier instead of one per load
  IMT_STAMP(p.trace, 0);
  constexpr int CPR = RB / 16, NIT = 128 * CPR / 512;
  u32x4 vk[NIT], vv[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int q = threadIdx.x + it * 512, tr = min(q / CPR, p.Tk - 1), c = q % CPR;
    vk[it] = *reinterpret_cast<const u32x4*>(Kb + (int64_t)tr * p.ldk + c * 8);
    vv[it] = *reinterpret_cast<const u32x4*>(Vb + (int64_t)tr * p.ldv + c * 8);
  }
  frag_t qf[NS];
  load_row_frags<T, DH>(qf, Qb, p.ldq, q0, p.Tq);
  const uint8_t* kmp = p.key_mask ? p.key_mask + (int64_t)b * p.Tk + min((int)threadIdx.x & 127, p.Tk - 1) : reinterpret_cast<const uint8_t*>(Kb);
  const uint8_t* qmp = p.query_mask ? p.query_mask + (int64_t)b * p.Tq + min(i, p.Tq - 1) : reinterpret_cast<const uint8_t*>(Qb);
  const uint8_t kmv = *kmp, qmv = *qmp;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int q = threadIdx.x + it * 512, tr = q / CPR, c = q % CPR;
    const u32x4 z = {0u, 0u, 0u, 0u};
    *reinterpret_cast<u32x4*>(Ks + tile_off<RB>(tr, c)) = (tr < p.Tk) ? vk[it] : z;
    *reinterpret_cast<u32x4*>(Vs + tile_off<RB>(tr, c)) = (tr < p.Tk) ? vv[it] : z;
  }
  if (threadIdx.x < 128) {
    const int j = threadIdx.x;
    kmask_s[j] = (j < p.Tk) ? (p.key_mask ? kmv : (uint8_t)1) : (uint8_t)0;
  }
  const bool query_ok = (p.query_mask && i < p.Tq) ? (qmv != 0) : true;
  __syncthreads();
  IMT_STAMP(p.trace, 1);
  if (q0 >= p.Tq) return;  // whole wave past the last query (no barrier follows)

  // S^T: 8 tiles of 16 keys x this wave's 16 queries
  f32x4 s[8];
  float tmax = -INFINITY;
#pragma unroll
  for (int nt = 0; nt < 8; ++nt) {
    s[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NS; ++ks) mma16(s[nt], lds_frag_kcontig<T, RB>(Ks, 16 * nt, 4 * ks), qf[ks]);
    const uint32_t km4 = *reinterpret_cast<const uint32_t*>(kmask_s + 16 * nt + 4 * g);  // this lane's 4 keys
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = 16 * nt + 4 * g + e;
      float v = s[nt][e] * p.scale + (mask_ok<MASK3D>(p, b, i, j, ((km4 >> (8 * e)) & 0xffu) != 0, query_ok) ? 0.f : -10000.0f);
      if (j >= p.Tk) v = -INFINITY;
      s[nt][e] = v;
      tmax = fmaxf(tmax, v);
    }
  }
  tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
  tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
  IMT_STAMP(p.trace, 2);
  float psum = 0.f;
#pragma unroll
  for (int nt = 0; nt < 8; ++nt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float pv = __expf(s[nt][e] - tmax);
      psum += pv;
      s[nt][e] = pv;
    }
  if (p.drop_thresh) {  // one uniform branch around all 32 elements; 16 finaliser calls for them (pairs of keys)
    const uint32_t key = dropout_key(p.seed);
    const uint32_t prow = (uint32_t)attn_pair_row(p, b, h, i) + (uint32_t)(2 * g);  // (host: B*H*Tq*Tk < 2^32 for this kernel)
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
#pragma unroll
      for (int e2 = 0; e2 < 2; ++e2) {
        const uint32_t w = attn_drop_word(key, prow + 8 * nt + e2);
        s[nt][2 * e2] = (w & 0xffffu) >= p.drop_thresh ? s[nt][2 * e2] * p.inv_keep : 0.f;
        s[nt][2 * e2 + 1] = (w >> 16) >= p.drop_thresh ? s[nt][2 * e2 + 1] * p.inv_keep : 0.f;
      }
  }
  psum += __shfl_xor(psum, 16, 64);
  psum += __shfl_xor(psum, 32, 64);
  IMT_STAMP(p.trace, 3);
  f32x4 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 4; ++u) {  // 32 keys per MFMA k-step
    const frag_t pf = acc_pair_to_frag(s[2 * u], s[2 * u + 1]);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) mma16(o[dt], lds_frag_kperm_bf16<RB>(Vs, 32 * u, 16 * dt), pf);
  }
  const float inv_l = 1.0f / psum;
  if (i < p.Tq) {
    T* Ob = reinterpret_cast<T*>(p.O) + ((int64_t)b * p.Tq + i) * p.ldo + h * DH;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) Vec4<T>::store(Ob + 16 * dt + 4 * g, o[dt] * inv_l);
    if (g == 0 && p.lse) p.lse[((int64_t)b * p.H + h) * p.Tq + i] = tmax + __logf(psum);
  }
  IMT_STAMP(p.trace, 4);
}

// =========================================================================================== backward: dQ
template <typename T, int DH, bool MASK3D>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 4 : 3) void attn_bwd_dq_kernel(AttnP p) {
  constexpr int RB = DH * sizeof(T), NS = RB / 64, NDT = DH / 16;
  typedef typename Frag<T>::type frag_t;
  constexpr int NSUB = (RB > 128) ? 1 : 2;
  __shared__ __attribute__((aligned(16))) char Ks[NSUB][64 * RB];
  __shared__ __attribute__((aligned(16))) char Vs[NSUB][64 * RB];
  __shared__ uint8_t kmask_s[NSUB * 64];

  const int nqt = (p.Tq + 63) / 64;
  const int lid = imt_xcd_block(blockIdx.x, gridDim.x);  // batch-major: XCD x owns batches [x*B/8, (x+1)*B/8)
  const int b = lid / (p.H * nqt), h = (lid / nqt) % p.H, tile_x = lid % nqt;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int q0 = tile_x * 64 + wave * 16;
  const int i = q0 + r;
  const T* Qb = reinterpret_cast<const T*>(p.Q) + (int64_t)b * p.Tq * p.ldq + h * DH;
  const T* Kb = reinterpret_cast<const T*>(p.K) + (int64_t)b * p.Tk * p.ldk + h * DH;
  const T* Vb = reinterpret_cast<const T*>(p.V) + (int64_t)b * p.Tk * p.ldv + h * DH;
  const T* dOb = reinterpret_cast<const T*>(p.dO) + (int64_t)b * p.Tq * p.lddo + h * DH;

  frag_t qf[NS], dof[NS];
  load_row_frags<T, DH>(qf, Qb, p.ldq, q0, p.Tq);
  load_row_frags<T, DH>(dof, dOb, p.lddo, q0, p.Tq);
  const bool query_ok = (p.query_mask && i < p.Tq) ? (p.query_mask[(int64_t)b * p.Tq + i] != 0) : true;
  const int64_t srow = ((int64_t)b * p.H + h) * p.Tq + (i < p.Tq ? i : 0);
  const float lse_i = p.lse[srow];
  // delta_i = rowsum(dO * O) of this lane's query row, computed here from the row fragments (the lanes r, r+16, r+32,
  // r+48 hold the four 16-byte chunks of each 64-byte k-step) and published for the dK/dV kernel that runs next.
  float delta_i = 0.f;
  {
    const T* Ob = reinterpret_cast<const T*>(p.O) + (int64_t)b * p.Tq * p.ldo + h * DH;
    frag_t of[NS];
    load_row_frags<T, DH>(of, Ob, p.ldo, q0, p.Tq);
#pragma unroll
    for (int ks = 0; ks < NS; ++ks)
#pragma unroll
      for (int e = 0; e < Frag<T>::EPC; ++e) delta_i += (float)dof[ks][e] * (float)of[ks][e];
    delta_i += __shfl_xor(delta_i, 16, 64);
    delta_i += __shfl_xor(delta_i, 32, 64);
    if (g == 0 && i < p.Tq) p.delta[srow] = delta_i;
  }

  f32x4 dq[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nkt = (p.Tk + 63) / 64;
  for (int kt0 = 0; kt0 < nkt; kt0 += NSUB) {
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
      if (kt0 + sub < nkt) {
        stage_tile<T, DH>(Ks[sub], Kb, p.ldk, (kt0 + sub) * 64, p.Tk);
        stage_tile<T, DH>(Vs[sub], Vb, p.ldv, (kt0 + sub) * 64, p.Tk);
      }
    }
    if (threadIdx.x < NSUB * 64) {
      const int j = kt0 * 64 + threadIdx.x;
      kmask_s[threadIdx.x] = (j < p.Tk) ? (p.key_mask ? p.key_mask[(int64_t)b * p.Tk + j] : (uint8_t)1) : (uint8_t)0;
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
    const int kt = kt0 + sub;
    if (kt >= nkt) break;
    const char* Kt = Ks[sub];
    const char* Vt = Vs[sub];
    const uint8_t* kmask_t = kmask_s + 64 * sub;
    f32x4 s[4], dp[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      s[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      dp[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NS; ++ks) {
        mma16(s[nt], lds_frag_kcontig<T, RB>(Kt, 16 * nt, 4 * ks), qf[ks]);
        mma16(dp[nt], lds_frag_kcontig<T, RB>(Vt, 16 * nt, 4 * ks), dof[ks]);
      }
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int jl = 16 * nt + 4 * g + e, j = kt * 64 + jl;
        float v = s[nt][e] * p.scale + (mask_ok<MASK3D>(p, b, i, j, kmask_t[jl] != 0, query_ok) ? 0.f : -10000.0f);
        float pv = (j < p.Tk) ? __expf(v - lse_i) : 0.f;
        float dpv = dp[nt][e];
        if (p.drop_thresh)
          dpv = attn_drop_keep(attn_drop_word(dropout_key(p.seed), attn_pair_row(p, b, h, i) + (uint64_t)(j >> 1)), j, p.drop_thresh) ? dpv * p.inv_keep : 0.f;
        s[nt][e] = pv * (dpv - delta_i);  // dS^T
      }
#pragma unroll
    for (int u = 0; u < AccOperand<T>::NFR; ++u) {
      const frag_t dsf = AccOperand<T>::get(s, u);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) mma16(dq[dt], AccOperand<T>::template lds<RB>(Kt, u, 16 * dt), dsf);
    }
    }  // sub
  }
  if (i < p.Tq) {
    T* dQb = reinterpret_cast<T*>(p.dQ) + ((int64_t)b * p.Tq + i) * p.lddq + h * DH;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) Vec4<T>::store(dQb + 16 * dt + 4 * g, dq[dt] * p.scale);
  }
}

// =========================================================================================== backward: dK, dV
template <typename T, int DH, bool MASK3D>
__global__ __launch_bounds__(256, (DH == 64 && sizeof(T) == 2) ? 3 : 2) void attn_bwd_dkdv_kernel(AttnP p) {
  constexpr int RB = DH * sizeof(T), NS = RB / 64, NDT = DH / 16;
  typedef typename Frag<T>::type frag_t;
  constexpr int NSUB = (RB > 128) ? 1 : 2;
  __shared__ __attribute__((aligned(16))) char Qs[NSUB][64 * RB];
  __shared__ __attribute__((aligned(16))) char dOs[NSUB][64 * RB];
  __shared__ float lse_s[NSUB * 64], delta_s[NSUB * 64];
  __shared__ uint8_t qmask_s[NSUB * 64];

  const int nkt0 = (p.Tk + 63) / 64;
  const int lid = imt_xcd_block(blockIdx.x, gridDim.x);
  const int b = lid / (p.H * nkt0), h = (lid / nkt0) % p.H, tile_x = lid % nkt0;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int k0 = tile_x * 64 + wave * 16;
  const int j = k0 + r;  // this lane's key
  const T* Qb = reinterpret_cast<const T*>(p.Q) + (int64_t)b * p.Tq * p.ldq + h * DH;
  const T* Kb = reinterpret_cast<const T*>(p.K) + (int64_t)b * p.Tk * p.ldk + h * DH;
  const T* Vb = reinterpret_cast<const T*>(p.V) + (int64_t)b * p.Tk * p.ldv + h * DH;
  const T* dOb = reinterpret_cast<const T*>(p.dO) + (int64_t)b * p.Tq * p.lddo + h * DH;

  frag_t kf[NS], vf[NS];
  load_row_frags<T, DH>(kf, Kb, p.ldk, k0, p.Tk);
  load_row_frags<T, DH>(vf, Vb, p.ldv, k0, p.Tk);
  const bool key_ok = (j < p.Tk) ? (p.key_mask ? (p.key_mask[(int64_t)b * p.Tk + j] != 0) : true) : false;

  f32x4 dk[NDT], dv[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) { dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  const int nqt = (p.Tq + 63) / 64;
  for (int qt0 = 0; qt0 < nqt; qt0 += NSUB) {
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
      if (qt0 + sub < nqt) {
        stage_tile<T, DH>(Qs[sub], Qb, p.ldq, (qt0 + sub) * 64, p.Tq);
        stage_tile<T, DH>(dOs[sub], dOb, p.lddo, (qt0 + sub) * 64, p.Tq);
      }
    }
    if (threadIdx.x < NSUB * 64) {
      const int i = qt0 * 64 + threadIdx.x;
      const int64_t srow = ((int64_t)b * p.H + h) * p.Tq + (i < p.Tq ? i : 0);
      lse_s[threadIdx.x] = p.lse[srow];
      delta_s[threadIdx.x] = p.delta[srow];
      qmask_s[threadIdx.x] = (i < p.Tq) ? (p.query_mask ? p.query_mask[(int64_t)b * p.Tq + i] : (uint8_t)1) : (uint8_t)1;
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
    const int qt = qt0 + sub;
    if (qt >= nqt) break;
    const char* Qt = Qs[sub];
    const char* dOt = dOs[sub];
    const float* lse_t = lse_s + 64 * sub;
    const float* delta_t = delta_s + 64 * sub;
    const uint8_t* qmask_t = qmask_s + 64 * sub;
    // S tiles: rows <- queries (16 per tile), cols <- this wave's 16 keys
    f32x4 s[4], dp[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      s[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      dp[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NS; ++ks) {
        mma16(s[mt], lds_frag_kcontig<T, RB>(Qt, 16 * mt, 4 * ks), kf[ks]);
        mma16(dp[mt], lds_frag_kcontig<T, RB>(dOt, 16 * mt, 4 * ks), vf[ks]);
      }
    }
    f32x4 pd[4];  // dropped P (operand of dV)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int il = 16 * mt + 4 * g + e, i = qt * 64 + il;
        float v = s[mt][e] * p.scale + (mask_ok<MASK3D>(p, b, i, j, key_ok, qmask_t[il] != 0) ? 0.f : -10000.0f);
        float pv = (i < p.Tq && j < p.Tk) ? __expf(v - lse_t[il]) : 0.f;
        float dpv = dp[mt][e], pdv = pv;
        if (p.drop_thresh) {
          const bool keep = attn_drop_keep(attn_drop_word(dropout_key(p.seed), attn_pair_row(p, b, h, i) + (uint64_t)(j >> 1)), j, p.drop_thresh);
          dpv = keep ? dpv * p.inv_keep : 0.f;
          pdv = keep ? pv * p.inv_keep : 0.f;
        }
        pd[mt][e] = pdv;
        s[mt][e] = pv * (dpv - delta_t[il]);  // dS
      }
#pragma unroll
    for (int u = 0; u < AccOperand<T>::NFR; ++u) {
      const frag_t pf = AccOperand<T>::get(pd, u);
      const frag_t dsf = AccOperand<T>::get(s, u);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        mma16(dv[dt], AccOperand<T>::template lds<RB>(dOt, u, 16 * dt), pf);   // dV^T[d][n] += dO^T[d][m] P[m][n]
        mma16(dk[dt], AccOperand<T>::template lds<RB>(Qt, u, 16 * dt), dsf);   // dK^T[d][n] += Q^T[d][m] dS[m][n]
      }
    }
    }  // sub
  }
  if (j < p.Tk) {
    T* dKb = reinterpret_cast<T*>(p.dK) + ((int64_t)b * p.Tk + j) * p.lddk + h * DH;
    T* dVb = reinterpret_cast<T*>(p.dV) + ((int64_t)b * p.Tk + j) * p.lddv + h * DH;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      Vec4<T>::store(dKb + 16 * dt + 4 * g, dk[dt] * p.scale);
      Vec4<T>::store(dVb + 16 * dt + 4 * g, dv[dt]);
    }
  }
}

// =========================================================================================== backward, short sequences
// Tq, Tk <= 128 (the C1 workload: S = T = 128), bf16: ONE workgroup (8 waves) per (batch, head) computes dQ, dK and
// dV together.  The two-kernel path above recomputes S and dP twice, reads Q/K/V/dO/O twice and pays two dependent
// load->compute->store latency chains per attention block; here
//   phase 0: Q and dO (all <= 128 rows) are staged once, delta = rowsum(dO * O) is taken from the row fragments;
//   phase 1: KEY on the lane (wave w owns keys 16w..16w+15, K/V rows in registers): S, P, dP, dS for all queries;
//            dV^T += dO^T P and dK^T += Q^T dS accumulate in registers; dS^T goes to LDS as bf16 [key][query];
//   phase 2: QUERY on the lane (wave w owns queries 16w..): dQ = dS K as a plain K-strided x K-strided product from
//            LDS (dS^T tile, and K parked into the region Q occupied).
// Nothing is summed across workgroups; same dropout mask / mask semantics as the kernels above.
//
// PROJ = true (imt_attention_bwd_proj): the attention output went through the block's output projection, so dO = dY W_o, and
// phase 0 forms this head's slice dO_h = dY[b] (Tq x d_model) W_o[:, 64h .. 64h+63] itself instead of reading what a GEMM
// launch stored: 8 MB less written and read back per block at the C1 shapes, and one launch less.  Wave w owns query rows
// 16w .. 16w+15 (as it does for delta): its dY rows are K-contiguous and come straight from global memory as the MFMA's B
// operand; the W_o slice is K-strided and is staged 256 k at a time, alternately into the dS^T region (unused until phase 1)
// and the Q | dO regions (filled afterwards), read back with the transposed LDS read.  The products are C^T tiles summed over
// ascending 32-element k-steps in fp32 and rounded once to bf16 -- what imt_gemm does for the NN product -- so the dO tile
// in LDS, the fragments delta is taken from and the optional copy in global memory carry the bits the GEMM would have stored.
struct ProjP { const void* dy; int64_t lddy; const void* w; int64_t ldw; int d_model; };

// dynamic LDS of a launch: the Q and dO tiles, the dS^T tile, lse and delta, the query mask
constexpr int fused_lds_bytes(int dh) { return 2 * 128 * (dh * 2) + 128 * 256 + 2 * 128 * 4 + 128; }

template <int DH, bool MASK3D, bool PROJ>
IMT_DEVICE void attn_bwd_fused_body(const AttnP& p, const ProjP& pj) {
  typedef bf16_t T;
  constexpr int RB = DH * 2, NS = RB / 64, NDT = DH / 16;
  typedef typename Frag<T>::type frag_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qs = smem;                        // [128][RB]  (phase 2: K)
  char* dOs = Qs + 128 * RB;              // [128][RB]
  char* dST = dOs + 128 * RB;             // [128 keys][128 queries] bf16, 256-B rows
  float* lse_s = reinterpret_cast<float*>(dST + 128 * 256);
  float* delta_s = lse_s + 128;
  uint8_t* qmask_s = reinterpret_cast<uint8_t*>(delta_s + 128);
  static_assert(fused_lds_bytes(DH) == 128 * RB + 128 * RB + 128 * 256 + 128 * 4 + 128 * 4 + 128, "the launches size LDS for this carve");

  const int lid = imt_xcd_block(blockIdx.x, gridDim.x);
  const int b = lid / p.H, h = lid % p.H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const T* Qb = reinterpret_cast<const T*>(p.Q) + (int64_t)b * p.Tq * p.ldq + h * DH;
  const T* Kb = reinterpret_cast<const T*>(p.K) + (int64_t)b * p.Tk * p.ldk + h * DH;
  const T* Vb = reinterpret_cast<const T*>(p.V) + (int64_t)b * p.Tk * p.ldv + h * DH;
  const T* dOb = reinterpret_cast<const T*>(p.dO) + (int64_t)b * p.Tq * p.lddo + h * DH;
  const T* Ob = reinterpret_cast<const T*>(p.O) + (int64_t)b * p.Tq * p.ldo + h * DH;

  // ---- phase 0
  // every global load of the kernel is requested here, unconditionally (clamped rows, a valid stand-in address for an
  // absent mask) and before the first use: one memory round trip in front of the barrier instead of one per load
  IMT_STAMP(p.trace, 0);
  const int k0 = 16 * wave;
  const int j = k0 + r;  // this lane's key (phase 1)
  frag_t kf[NS], vf[NS];
  bool key_ok;
  {
    constexpr int CPR = RB / 16, NIT = 128 * CPR / 512;
    u32x4 vq[NIT], vo[NIT];
    const int i = 16 * wave + r;  // delta / lse of this wave's 16 query rows
    frag_t of[NS], dof[NS];
    // (PROJ: the Q tile and the O rows are requested under the last W_o chunk, into the registers the chunks came through)
    auto load_q_o = [&]() {
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int q = threadIdx.x + it * 512, tr = min(q / CPR, p.Tq - 1), c = q % CPR;
        vq[it] = *reinterpret_cast<const u32x4*>(Qb + (int64_t)tr * p.ldq + c * 8);
        if (!PROJ) vo[it] = *reinterpret_cast<const u32x4*>(dOb + (int64_t)tr * p.lddo + c * 8);
      }
      load_row_frags<T, DH>(of, Ob, p.ldo, 16 * wave, p.Tq);
    };
    if (!PROJ) load_q_o();
    if (!PROJ) load_row_frags<T, DH>(dof, dOb, p.lddo, 16 * wave, p.Tq);
    load_row_frags<T, DH>(kf, Kb, p.ldk, k0, p.Tk);
    load_row_frags<T, DH>(vf, Vb, p.ldv, k0, p.Tk);
    const float lse_v = p.lse[((int64_t)b * p.H + h) * p.Tq + min(i, p.Tq - 1)];
    const uint8_t* qmp = p.query_mask ? p.query_mask + (int64_t)b * p.Tq + min(i, p.Tq - 1) : reinterpret_cast<const uint8_t*>(Qb);
    const uint8_t* kmp = p.key_mask ? p.key_mask + (int64_t)b * p.Tk + min(j, p.Tk - 1) : reinterpret_cast<const uint8_t*>(Kb);
    const uint8_t qmv = *qmp, kmv = *kmp;
    if constexpr (PROJ) {
      static_assert(!PROJ || DH == 64, "the W_o slice is staged as 128-byte rows");
      constexpr int WK = 256, WIT = WK * CPR / 512;  // k rows of W_o per staged chunk ([WK][64] bf16 = 32 KiB), 16-B chunks per thread
      const int dm = pj.d_model, nks = dm / 32, nch = (nks + 7) / 8;
      const T* Wb = reinterpret_cast<const T*>(pj.w) + h * DH + (threadIdx.x % CPR) * 8;
      const T* dYr = reinterpret_cast<const T*>(pj.dy) + ((int64_t)b * p.Tq + min(i, p.Tq - 1)) * pj.lddy + 8 * g;
      const int wkr = threadIdx.x / CPR;  // this thread's k row within a 64-row slab of the chunk
      u32x4 wv[WIT];
      frag_t af[8];
      // (rows / k offsets past d_model are clamped to valid addresses: those loads are unconditional and never multiplied)
      auto load_w = [&](int ch) {
#pragma unroll
        for (int it = 0; it < WIT; ++it) wv[it] = *reinterpret_cast<const u32x4*>(Wb + (int64_t)min(WK * ch + wkr + 64 * it, dm - 1) * pj.ldw);
      };
      auto stage_w = [&](int ch) -> const char* {
        char* Ws = (ch & 1) ? Qs : dST;  // (the barrier of chunk ch - 1 is behind every wave's reads of chunk ch - 2)
#pragma unroll
        for (int it = 0; it < WIT; ++it) *reinterpret_cast<u32x4*>(Ws + tile_off<RB>(wkr + 64 * it, threadIdx.x % CPR)) = wv[it];
        __syncthreads();
        return Ws;
      };
      load_w(0);
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) af[ks] = *reinterpret_cast<const frag_t*>(dYr + min(32 * ks, dm - 32));
      f32x4 acc[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      // every chunk but the last is whole: its 8 k-steps run without a test, each followed by the request for the same k-step
      // of the next chunk into the registers it has just freed
#pragma unroll 1
      for (int ch = 0; ch + 1 < nch; ++ch) {
        const char* Ws = stage_w(ch);
        load_w(ch + 1);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) mma16(acc[nt], lds_frag_kstrided_bf16<RB>(Ws, 32 * ks, 16 * nt), af[ks]);  // C^T tile: rows <- n, cols <- query
          af[ks] = *reinterpret_cast<const frag_t*>(dYr + min(WK * (ch + 1) + 32 * ks, dm - 32));
        }
      }
      {
        const char* Ws = stage_w(nch - 1);
        load_q_o();
        const int nk = nks - 8 * (nch - 1);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
          if (ks < nk) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) mma16(acc[nt], lds_frag_kstrided_bf16<RB>(Ws, 32 * ks, 16 * nt), af[ks]);
          }
        }
      }
      __syncthreads();  // every wave is done with the W_o chunks: Q and dO may land in their regions
      // lane (r, g) of tile nt holds dO[query 16 wave + r][16 nt + 4 g + e]; rows >= Tq (clamped loads) are zero, as staged
      T* dOg = (p.dO && i < p.Tq) ? const_cast<T*>(dOb) + (int64_t)i * p.lddo : nullptr;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const f32x4 v = (i < p.Tq) ? acc[nt] : f32x4{0.f, 0.f, 0.f, 0.f};
        const bf16x4 w = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
        const int col = 16 * nt + 4 * g;
        *reinterpret_cast<bf16x4*>(dOs + tile_off<RB>(i, col >> 3) + ((col & 7) << 1)) = w;
        if (dOg) *reinterpret_cast<bf16x4*>(dOg + col) = w;
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int q = threadIdx.x + it * 512, tr = q / CPR, c = q % CPR;
      const u32x4 z = {0u, 0u, 0u, 0u};
      *reinterpret_cast<u32x4*>(Qs + tile_off<RB>(tr, c)) = (tr < p.Tq) ? vq[it] : z;
      if (!PROJ) *reinterpret_cast<u32x4*>(dOs + tile_off<RB>(tr, c)) = (tr < p.Tq) ? vo[it] : z;
    }
    if constexpr (PROJ) {  // this wave's own 16 rows of the tile, in the layout load_row_frags gives
#pragma unroll
      for (int s = 0; s < NS; ++s) dof[s] = lds_frag_kcontig<T, RB>(dOs, 16 * wave, 4 * s);
    }
    float d = 0.f;
#pragma unroll
    for (int ks = 0; ks < NS; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e) d += (float)dof[ks][e] * (float)of[ks][e];
    d += __shfl_xor(d, 16, 64);
    d += __shfl_xor(d, 32, 64);
    if (g == 0) {
      delta_s[i] = d;
      lse_s[i] = lse_v;
      qmask_s[i] = (i < p.Tq && p.query_mask) ? qmv : (uint8_t)1;
    }
    key_ok = (j < p.Tk) ? (p.key_mask ? (kmv != 0) : true) : false;
  }
  __syncthreads();
  IMT_STAMP(p.trace, 1);

  // ---- phase 1
  f32x4 dk[NDT], dv[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) { dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  const int nqt = (p.Tq + 63) / 64;
#pragma unroll 1
  for (int qt = 0; qt < 2; ++qt) {
    const char* Qt = Qs + qt * 64 * RB;
    const char* dOt = dOs + qt * 64 * RB;
    f32x4 s[4], dp[4], pd[4];
    if (qt < nqt) {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        s[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        dp[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NS; ++ks) {
          mma16(s[mt], lds_frag_kcontig<T, RB>(Qt, 16 * mt, 4 * ks), kf[ks]);
          mma16(dp[mt], lds_frag_kcontig<T, RB>(dOt, 16 * mt, 4 * ks), vf[ks]);
        }
      }
      // pair index of (query i, this lane's key j) = pair_base + i * ceil(Tk / 2): one finaliser call per element here (the
      // lane's four elements are four different queries)
      const uint32_t dkey = dropout_key(p.seed);
      const uint32_t tkp = (uint32_t)((p.Tk + 1) >> 1);
      const uint32_t pair_base = (uint32_t)(b * p.H + h) * (uint32_t)p.Tq * tkp + (uint32_t)(j >> 1);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        // this lane's 4 consecutive queries: their lse / delta / mask bytes in one LDS read each
        const int i0 = qt * 64 + 16 * mt + 4 * g;
        const f32x4 lse4 = *reinterpret_cast<const f32x4*>(lse_s + i0), del4 = *reinterpret_cast<const f32x4*>(delta_s + i0);
        const uint32_t qm4 = *reinterpret_cast<const uint32_t*>(qmask_s + i0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = i0 + e;
          float v = s[mt][e] * p.scale + (mask_ok<MASK3D>(p, b, i, j, key_ok, ((qm4 >> (8 * e)) & 0xffu) != 0) ? 0.f : -10000.0f);
          float pv = (i < p.Tq && j < p.Tk) ? __expf(v - lse4[e]) : 0.f;
          float dpv = dp[mt][e], pdv = pv;
          if (p.drop_thresh) {  // (host guarantees B*H*Tq*Tk < 2^32 for this kernel)
            const bool keep = attn_drop_keep(attn_drop_word(dkey, pair_base + (uint32_t)i * tkp), j, p.drop_thresh);
            dpv = keep ? dpv * p.inv_keep : 0.f;
            pdv = keep ? pv * p.inv_keep : 0.f;
          }
          pd[mt][e] = pdv;
          s[mt][e] = pv * (dpv - del4[e]);  // dS[i][j]
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const frag_t pf = acc_pair_to_frag(pd[2 * u], pd[2 * u + 1]);
        const frag_t dsf = acc_pair_to_frag(s[2 * u], s[2 * u + 1]);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          mma16(dv[dt], lds_frag_kperm_bf16<RB>(dOt, 32 * u, 16 * dt), pf);   // dV^T[d][key] += dO^T[d][q] P[q][key]
          mma16(dk[dt], lds_frag_kperm_bf16<RB>(Qt, 32 * u, 16 * dt), dsf);   // dK^T[d][key] += Q^T[d][q] dS[q][key]
        }
      }
    } else {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) s[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // dS^T[key j][queries 64qt + 16mt + 4g .. +3] (bf16, 8 bytes)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int q_first = qt * 64 + 16 * mt + 4 * g;
      bf16x4 w = {(bf16_t)s[mt][0], (bf16_t)s[mt][1], (bf16_t)s[mt][2], (bf16_t)s[mt][3]};
      *reinterpret_cast<bf16x4*>(dST + tile_off<256>(j, q_first >> 3) + ((q_first & 7) << 1)) = w;
    }
  }
  if (j < p.Tk) {
    T* dKb = reinterpret_cast<T*>(p.dK) + ((int64_t)b * p.Tk + j) * p.lddk + h * DH;
    T* dVb = reinterpret_cast<T*>(p.dV) + ((int64_t)b * p.Tk + j) * p.lddv + h * DH;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      Vec4<T>::store(dKb + 16 * dt + 4 * g, dk[dt] * p.scale);
      Vec4<T>::store(dVb + 16 * dt + 4 * g, dv[dt]);
    }
  }
  IMT_STAMP(p.trace, 2);
  __syncthreads();  // every wave is done with Q / dO; dS^T is complete
  IMT_STAMP(p.trace, 3);
  char* Ks = Qs;
#pragma unroll
  for (int ks = 0; ks < NS; ++ks) *reinterpret_cast<frag_t*>(Ks + tile_off<RB>(k0 + r, 4 * ks + g)) = kf[ks];
  __syncthreads();

  // ---- phase 2: dQ[q][d] = scale * sum_key dS[q][key] K[key][d]
  f32x4 dq[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nks = (p.Tk + 31) / 32;
#pragma unroll 1
  for (int kstep = 0; kstep < nks; ++kstep) {
    const frag_t fa = lds_frag_kstrided_bf16<256>(dST, 32 * kstep, 16 * wave);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) mma16(dq[dt], lds_frag_kstrided_bf16<RB>(Ks, 32 * kstep, 16 * dt), fa);
  }
  const int i = 16 * wave + r;
  if (i < p.Tq) {
    T* dQb = reinterpret_cast<T*>(p.dQ) + ((int64_t)b * p.Tq + i) * p.lddq + h * DH;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) Vec4<T>::store(dQb + 16 * dt + 4 * g, dq[dt] * p.scale);
  }  IMT_STAMP(p.trace, 4);
}
template <int DH, bool MASK3D>
__global__ __launch_bounds__(512, 4) void attn_bwd_fused_kernel(AttnP p) {
  attn_bwd_fused_body<DH, MASK3D, false>(p, ProjP());
}
template <bool MASK3D>
__global__ __launch_bounds__(512, 4) void attn_bwd_proj_kernel(AttnP p, ProjP pj) {
  attn_bwd_fused_body<64, MASK3D, true>(p, pj);
}

// =========================================================================================== backward: fused, 129-256 keys / queries
// The MASS shapes (BASELINE configs[4]: encoder self-attention 256 x 256, decoder cross-attention 128 x 256) took the
// two-kernel path above: S / dP recomputed twice, Q / K / V / dO read twice, 1.25 ms of a 10.7 ms step.  Same fusion as
// attn_bwd_fused_kernel, re-cut so that it fits 160 KiB of LDS at 256 keys: ONE workgroup (8 waves) per (batch, head),
//   phase 0: K / V rows in registers (KEY on the lane: wave w owns keys 32w .. 32w+31 as two groups of 16), K parked in LDS
//            once for phase 2, delta = rowsum(dO * O) and lse of all queries in LDS;
//   then per tile of 64 QUERIES (its Q / dO rows staged through registers one tile ahead):
//   phase 1: S, P, dP, dS for (64 queries x this wave's 32 keys); dV^T += dO^T P, dK^T += Q^T dS stay in registers over all
//            query tiles; dS^T of the tile goes to LDS as bf16 [key][query];
//   phase 2: QUERY on the lane: dQ[64 x dh] = dS K from LDS (wave = 16 queries x half of dh), stored at once.
// The [key][query] tile is 32 KiB instead of 128: 82 KiB in all.  Nothing is summed across workgroups (no atomics); same
// masks, same dropout draws as every other attention kernel.
constexpr int fused256_lds_bytes(int dh) { return 256 * (dh * 2) + 2 * 64 * (dh * 2) + 256 * 128 + 2 * 256 * 4 + 256; }  // K, Q | dO tiles, dS^T, lse | delta, query mask

template <int DH, bool MASK3D>
__global__ __launch_bounds__(512, 2) void attn_bwd_fused256_kernel(AttnP p) {
  typedef bf16_t T;
  constexpr int RB = DH * 2, NS = RB / 64, NDT = DH / 16, CPR = RB / 16;
  typedef typename Frag<T>::type frag_t;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;                         // [256 keys][RB]
  char* Qt = Ks + 256 * RB;                // [64][RB]   current query tile
  char* dOt = Qt + 64 * RB;                // [64][RB]
  char* dST = dOt + 64 * RB;               // [256 keys][64 queries] bf16, 128-B rows
  float* lse_s = reinterpret_cast<float*>(dST + 256 * 128);
  float* delta_s = lse_s + 256;
  uint8_t* qmask_s = reinterpret_cast<uint8_t*>(delta_s + 256);
  static_assert(fused256_lds_bytes(DH) == 256 * RB + 64 * RB + 64 * RB + 256 * 128 + 256 * 4 + 256 * 4 + 256, "the launch sizes LDS for this carve");

  const int lid = imt_xcd_block(blockIdx.x, gridDim.x);
  const int b = lid / p.H, h = lid % p.H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const T* Qb = reinterpret_cast<const T*>(p.Q) + (int64_t)b * p.Tq * p.ldq + h * DH;
  const T* Kb = reinterpret_cast<const T*>(p.K) + (int64_t)b * p.Tk * p.ldk + h * DH;
  const T* Vb = reinterpret_cast<const T*>(p.V) + (int64_t)b * p.Tk * p.ldv + h * DH;
  const T* dOb = reinterpret_cast<const T*>(p.dO) + (int64_t)b * p.Tq * p.lddo + h * DH;
  const T* Ob = reinterpret_cast<const T*>(p.O) + (int64_t)b * p.Tq * p.ldo + h * DH;
  const int nqt = (p.Tq + 63) / 64;

  // ---- phase 0: every load requested up front, unconditionally (clamped rows / stand-in addresses)
  frag_t kf[2][NS], vf[2][NS];
  bool key_ok[2];
  // one 16-byte chunk of the 64-row Q / dO tile per thread (DH = 32: the first 256 threads), prefetched one tile ahead
  const int st_row = (int)threadIdx.x / CPR, st_c = (int)threadIdx.x % CPR;
  const bool stager = st_row < 64;
  u32x4 vq, vo;
  auto prefetch = [&](int qt) {
    const int tr = min(qt * 64 + min(st_row, 63), p.Tq - 1);
    vq = *reinterpret_cast<const u32x4*>(Qb + (int64_t)tr * p.ldq + st_c * 8);
    vo = *reinterpret_cast<const u32x4*>(dOb + (int64_t)tr * p.lddo + st_c * 8);
  };
  prefetch(0);
  {
#pragma unroll
    for (int kg = 0; kg < 2; ++kg) {
      load_row_frags<T, DH>(kf[kg], Kb, p.ldk, 32 * wave + 16 * kg, p.Tk);
      load_row_frags<T, DH>(vf[kg], Vb, p.ldv, 32 * wave + 16 * kg, p.Tk);
    }
    frag_t of[2][NS], dof[2][NS];
    float lse_v[2];
    uint8_t qmv[2], kmv[2];
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int i = 128 * ps + 16 * wave + r;
      load_row_frags<T, DH>(of[ps], Ob, p.ldo, 128 * ps + 16 * wave, p.Tq);
      load_row_frags<T, DH>(dof[ps], dOb, p.lddo, 128 * ps + 16 * wave, p.Tq);
      lse_v[ps] = p.lse[((int64_t)b * p.H + h) * p.Tq + min(i, p.Tq - 1)];
      const uint8_t* qmp = p.query_mask ? p.query_mask + (int64_t)b * p.Tq + min(i, p.Tq - 1) : reinterpret_cast<const uint8_t*>(Qb);
      qmv[ps] = *qmp;
    }
#pragma unroll
    for (int kg = 0; kg < 2; ++kg) {
      const int j = 32 * wave + 16 * kg + r;
      const uint8_t* kmp = p.key_mask ? p.key_mask + (int64_t)b * p.Tk + min(j, p.Tk - 1) : reinterpret_cast<const uint8_t*>(Kb);
      kmv[kg] = *kmp;
    }
#pragma unroll
    for (int kg = 0; kg < 2; ++kg) {
      const int j = 32 * wave + 16 * kg + r;
      key_ok[kg] = (j < p.Tk) ? (p.key_mask ? (kmv[kg] != 0) : true) : false;
#pragma unroll
      for (int ks = 0; ks < NS; ++ks) *reinterpret_cast<frag_t*>(Ks + tile_off<RB>(j, 4 * ks + g)) = kf[kg][ks];  // rows >= Tk: zeros
    }
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int i = 128 * ps + 16 * wave + r;
      float d = 0.f;
#pragma unroll
      for (int ks = 0; ks < NS; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) d += (float)dof[ps][ks][e] * (float)of[ps][ks][e];
      d += __shfl_xor(d, 16, 64);
      d += __shfl_xor(d, 32, 64);
      if (g == 0) {
        delta_s[i] = d;
        lse_s[i] = lse_v[ps];
        qmask_s[i] = (i < p.Tq && p.query_mask) ? qmv[ps] : (uint8_t)1;
      }
    }
  }

  f32x4 dk[2][NDT], dv[2][NDT];
#pragma unroll
  for (int kg = 0; kg < 2; ++kg)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) { dk[kg][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[kg][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  const uint32_t dkey = dropout_key(p.seed);
  const uint32_t tkp = (uint32_t)((p.Tk + 1) >> 1);
  const int nks = (p.Tk + 31) / 32;
  const int qg = wave & 3, dhalf = wave >> 2;   // phase 2: 16 queries x half of the head dimension per wave
  constexpr int NDH = (NDT + 1) / 2;

#pragma unroll 1
  for (int qt = 0; qt < nqt; ++qt) {
    // the staged tile: rows past Tq are zeros.  (Every wave has left phase 2 of the previous tile -- which reads neither Qt
    // nor dOt -- only after the barrier that closed its phase 1, so these writes cannot overtake a reader.)
    if (stager) {
      const u32x4 z = {0u, 0u, 0u, 0u};
      const bool in = qt * 64 + st_row < p.Tq;
      *reinterpret_cast<u32x4*>(Qt + tile_off<RB>(st_row, st_c)) = in ? vq : z;
      *reinterpret_cast<u32x4*>(dOt + tile_off<RB>(st_row, st_c)) = in ? vo : z;
    }
    __syncthreads();  // tile staged (first trip: K, delta, lse too); dS^T of the previous tile fully consumed
    if (qt + 1 < nqt) prefetch(qt + 1);

    // ---- phase 1
#pragma unroll
    for (int kg = 0; kg < 2; ++kg) {
      const int j = 32 * wave + 16 * kg + r;  // this lane's key
      f32x4 s[4], dp[4], pd[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        s[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        dp[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NS; ++ks) {
          mma16(s[mt], lds_frag_kcontig<T, RB>(Qt, 16 * mt, 4 * ks), kf[kg][ks]);
          mma16(dp[mt], lds_frag_kcontig<T, RB>(dOt, 16 * mt, 4 * ks), vf[kg][ks]);
        }
      }
      const uint32_t pair_base = (uint32_t)(b * p.H + h) * (uint32_t)p.Tq * tkp + (uint32_t)(j >> 1);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int i0 = qt * 64 + 16 * mt + 4 * g;  // this lane's 4 consecutive queries
        const f32x4 lse4 = *reinterpret_cast<const f32x4*>(lse_s + i0), del4 = *reinterpret_cast<const f32x4*>(delta_s + i0);
        const uint32_t qm4 = *reinterpret_cast<const uint32_t*>(qmask_s + i0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = i0 + e;
          float v = s[mt][e] * p.scale + (mask_ok<MASK3D>(p, b, i, j, key_ok[kg], ((qm4 >> (8 * e)) & 0xffu) != 0) ? 0.f : -10000.0f);
          float pv = (i < p.Tq && j < p.Tk) ? __expf(v - lse4[e]) : 0.f;
          float dpv = dp[mt][e], pdv = pv;
          if (p.drop_thresh) {  // (host guarantees B*H*Tq*Tk < 2^32 for this kernel)
            const bool keep = attn_drop_keep(attn_drop_word(dkey, pair_base + (uint32_t)i * tkp), j, p.drop_thresh);
            dpv = keep ? dpv * p.inv_keep : 0.f;
            pdv = keep ? pv * p.inv_keep : 0.f;
          }
          pd[mt][e] = pdv;
          s[mt][e] = pv * (dpv - del4[e]);  // dS[i][j]
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const frag_t pf = acc_pair_to_frag(pd[2 * u], pd[2 * u + 1]);
        const frag_t dsf = acc_pair_to_frag(s[2 * u], s[2 * u + 1]);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          mma16(dv[kg][dt], lds_frag_kperm_bf16<RB>(dOt, 32 * u, 16 * dt), pf);   // dV^T[d][key] += dO^T[d][q] P[q][key]
          mma16(dk[kg][dt], lds_frag_kperm_bf16<RB>(Qt, 32 * u, 16 * dt), dsf);   // dK^T[d][key] += Q^T[d][q] dS[q][key]
        }
      }
      // dS^T[key j][local queries 16mt + 4g .. +3] (bf16, 8 bytes)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int ql = 16 * mt + 4 * g;
        bf16x4 w = {(bf16_t)s[mt][0], (bf16_t)s[mt][1], (bf16_t)s[mt][2], (bf16_t)s[mt][3]};
        *reinterpret_cast<bf16x4*>(dST + tile_off<128>(j, ql >> 3) + ((ql & 7) << 1)) = w;
      }
    }
    __syncthreads();  // dS^T of this tile complete

    // ---- phase 2: dQ[q][d] = scale * sum_key dS[q][key] K[key][d]
    f32x4 dq[NDH];
#pragma unroll
    for (int t = 0; t < NDH; ++t) dq[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (dhalf * NDH < NDT) {  // (uniform per wave; DH = 32 with NDT = 2: both halves hold one tile)
#pragma unroll 2
      for (int kstep = 0; kstep < nks; ++kstep) {
        const frag_t fa = lds_frag_kstrided_bf16<128>(dST, 32 * kstep, 16 * qg);
#pragma unroll
        for (int t = 0; t < NDH; ++t) mma16(dq[t], lds_frag_kstrided_bf16<RB>(Ks, 32 * kstep, 16 * (dhalf * NDH + t)), fa);
      }
      const int i = qt * 64 + 16 * qg + r;
      if (i < p.Tq) {
        T* dQb = reinterpret_cast<T*>(p.dQ) + ((int64_t)b * p.Tq + i) * p.lddq + h * DH;
#pragma unroll
        for (int t = 0; t < NDH; ++t) Vec4<T>::store(dQb + 16 * (dhalf * NDH + t) + 4 * g, dq[t] * p.scale);
      }
    }
  }
#pragma unroll
  for (int kg = 0; kg < 2; ++kg) {
    const int j = 32 * wave + 16 * kg + r;
    if (j < p.Tk) {
      T* dKb = reinterpret_cast<T*>(p.dK) + ((int64_t)b * p.Tk + j) * p.lddk + h * DH;
      T* dVb = reinterpret_cast<T*>(p.dV) + ((int64_t)b * p.Tk + j) * p.lddv + h * DH;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        Vec4<T>::store(dKb + 16 * dt + 4 * g, dk[kg][dt] * p.scale);
        Vec4<T>::store(dVb + 16 * dt + 4 * g, dv[kg][dt]);
      }
    }
  }
}

int check_args(const imt_attn_args* a, bool bwd, bool need_dO = true) {
  IMT_CHECK_ARG(a != nullptr, "attention: null args");
  IMT_CHECK_ARG(imt_ok_dtype(a->dtype), "attention: bad dtype");
  IMT_CHECK_ARG(a->head_dim == 32 || a->head_dim == 64, "attention: head_dim %d unsupported (32 or 64)", a->head_dim);
  IMT_CHECK_ARG(a->B > 0 && a->H > 0 && a->Tq > 0 && a->Tk > 0, "attention: bad dims");
  const int al = (a->dtype == IMT_BF16) ? 8 : 4;
  IMT_CHECK_ARG(a->Q && a->K && a->V && a->O, "attention: null tensor");
  IMT_CHECK_ARG(a->ldq % al == 0 && a->ldk % al == 0 && a->ldv % al == 0 && a->ldo % al == 0, "attention: ld must be 16-B multiples");
  IMT_CHECK_ARG((((uintptr_t)a->Q | (uintptr_t)a->K | (uintptr_t)a->V | (uintptr_t)a->O) & 15) == 0, "attention: 16-B alignment");
  if (bwd) {
    IMT_CHECK_ARG((a->dO || !need_dO) && a->dQ && a->dK && a->dV && a->lse && a->delta, "attention_bwd: null tensor");
    IMT_CHECK_ARG(a->lddo % al == 0 && a->lddq % al == 0 && a->lddk % al == 0 && a->lddv % al == 0, "attention_bwd: ld alignment");
    IMT_CHECK_ARG((((uintptr_t)a->dO | (uintptr_t)a->dQ | (uintptr_t)a->dK | (uintptr_t)a->dV) & 15) == 0, "attention_bwd: 16-B alignment");
  }
  return IMT_OK;
}

AttnP make_params(const imt_attn_args* a) {
  AttnP p;
  p.B = a->B; p.H = a->H; p.Tq = a->Tq; p.Tk = a->Tk;
  p.Q = a->Q; p.ldq = a->ldq; p.K = a->K; p.ldk = a->ldk; p.V = a->V; p.ldv = a->ldv; p.O = a->O; p.ldo = a->ldo;
  p.lse = a->lse; p.key_mask = a->key_mask; p.query_mask = a->query_mask; p.mask3d = a->mask3d; p.causal = a->causal;
  p.scale = a->scale;
  p.drop_thresh = dropout_thresh(a->dropout_p);
  p.inv_keep = a->dropout_p > 0.f ? 1.f / (1.f - a->dropout_p) : 1.f;
  p.seed = a->dropout_seed;
  p.dO = a->dO; p.lddo = a->lddo; p.dQ = a->dQ; p.lddq = a->lddq; p.dK = a->dK; p.lddk = a->lddk; p.dV = a->dV; p.lddv = a->lddv; p.trace = nullptr;
  p.delta = a->delta;
  return p;
}

// ------------------------------------------------------------------------------------------------ plan
// The tuning switches, read once per entry-point call and not cached: the suite flips them inside one process.
struct AttnSwitches { bool no_short_fwd, no_fused_bwd, no_fused256; };
AttnSwitches read_switches() {
  return {getenv("IMT_ATTN_NO_SHORT_FWD") != nullptr, getenv("IMT_ATTN_NO_FUSED_BWD") != nullptr, getenv("IMT_ATTN_NO_FUSED256") != nullptr};
}

enum FwdKernel { FWD_TILED, FWD_SHORT };
enum BwdKernel { BWD_PAIR, BWD_FUSED, BWD_FUSED256 };
constexpr int ONE_WG_T = 128, ONE_WG_T256 = 256;  // queries and keys one workgroup per (batch, head) holds: short / fused, fused-256

// the one-workgroup kernels index dropout elements with 32 bits
bool one_wg_fits(int B, int H, int Tq, int Tk, int limit) {
  return Tq <= limit && Tk <= limit && (double)B * H * Tq * Tk < 4294967296.0;
}
// (head_dim and the mask kind pick the template instance of the planned kernel, not the kernel)
FwdKernel plan_fwd(int dtype, int head_dim, int B, int H, int Tq, int Tk, bool has_mask3d, const AttnSwitches& sw) {
  if (dtype == IMT_F32) return FWD_TILED;
  return Tq > 64 && one_wg_fits(B, H, Tq, Tk, ONE_WG_T) && !sw.no_short_fwd ? FWD_SHORT : FWD_TILED;
}
BwdKernel plan_bwd(int dtype, int head_dim, int B, int H, int Tq, int Tk, bool has_mask3d, const AttnSwitches& sw) {
  if (dtype == IMT_F32 || sw.no_fused_bwd) return BWD_PAIR;
  if (one_wg_fits(B, H, Tq, Tk, ONE_WG_T)) return BWD_FUSED;
  // 129 .. 256 keys / queries (MASS: encoder self-attention at 256 tokens, the decoder's cross-attention over them)
  return one_wg_fits(B, H, Tq, Tk, ONE_WG_T256) && !sw.no_fused256 ? BWD_FUSED256 : BWD_PAIR;
}

// ------------------------------------------------------------------------------------------------ launch
// Host dispatch on the head_dim (checked: 32 | 64) and on the presence of a 3-D mask: f(tag) with tag() a compile-time constant,
// so that a launch names its template instance once (imt_by_dtype's counterparts; they nest).  The compiler emits the kernel
// instances in the order in which launch_fwd / launch_bwd come to name them (fp32 before bf16, statements top to bottom, the outer
// helper's cases before the inner one's); the nesting at each site keeps the code object's order, and so its bytes, as they were.
template <typename F> int by_head_dim(int head_dim, F&& f) {
  return head_dim == 32 ? f(std::integral_constant<int, 32>()) : f(std::integral_constant<int, 64>());
}
template <typename F> int by_mask3d(const AttnP& p, F&& f) { return p.mask3d ? f(std::true_type()) : f(std::false_type()); }
// raises the dynamic-LDS limit of a kernel instance, once per instance
template <auto KERNEL> void allow_lds(int bytes) {
  static const hipError_t once = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  (void)once;
}
template <typename K, typename... A> int launch(K kernel, int blocks, int threads, int lds, hipStream_t st, const A&... args) {
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds, st, args...);
  IMT_CHECK_LAUNCH();
  return IMT_OK;
}
AttnP traced(AttnP p, const ImtTrace& tr) { p.trace = tr.dev; return p; }
// for the profiler: the multiply-adds of one [Tq, Tk] x head_dim product; the bytes of rq operands of Tq rows and rk of Tk rows
double attn_work(const AttnP& p, int dh) { return (double)p.B * p.H * p.Tq * p.Tk * dh; }
double attn_io(const AttnP& p, int dh, size_t es, double rq, double rk) { return ((double)p.B * p.H * dh * es) * (rq * p.Tq + rk * p.Tk); }

template <typename T> int launch_fwd(FwdKernel k, const AttnP& p, int head_dim, hipStream_t st) {
  ImtProfScope prof(sizeof(T) == 2 ? "attn_fwd_bf16" : "attn_fwd_f32", 4.0 * attn_work(p, head_dim), attn_io(p, head_dim, sizeof(T), 2.0, 2.0), st);
  if constexpr (sizeof(T) == 2) {  // (the one-workgroup kernels exist in bf16 only)
    if (k == FWD_SHORT) {
      ImtTrace tr("attn_fwd", p.B * p.H, st);
      return by_head_dim(head_dim, [&](auto dh) {
        return by_mask3d(p, [&](auto m3) { return launch(attn_fwd_short_kernel<dh(), m3()>, p.B * p.H, 512, 0, st, traced(p, tr)); });
      });
    }
  }
  return by_head_dim(head_dim, [&](auto dh) {
    return by_mask3d(p, [&](auto m3) { return launch(attn_fwd_kernel<T, dh(), m3()>, imt_cdiv(p.Tq, 64) * p.H * p.B, 256, 0, st, p); });
  });
}

template <typename T> int launch_bwd(BwdKernel k, const AttnP& p, int head_dim, hipStream_t st) {
  const double work = attn_work(p, head_dim);
  if constexpr (sizeof(T) == 2) {  // (the one-workgroup kernels exist in bf16 only)
    const double io = attn_io(p, head_dim, 2, 4.0, 4.0);
    if (k == BWD_FUSED)
      return by_mask3d(p, [&](auto m3) {
        return by_head_dim(head_dim, [&](auto dh) {
          constexpr auto kernel = attn_bwd_fused_kernel<dh(), m3()>;
          allow_lds<kernel>(fused_lds_bytes(dh()));
          ImtProfScope prof("attn_bwd_fused_bf16", 10.0 * work, io, st);
          ImtTrace tr("attn_bwd", p.B * p.H, st);
          return launch(kernel, p.B * p.H, 512, fused_lds_bytes(dh()), st, traced(p, tr));
        });
      });
    if (k == BWD_FUSED256)
      return by_mask3d(p, [&](auto m3) {
        return by_head_dim(head_dim, [&](auto dh) {
          constexpr auto kernel = attn_bwd_fused256_kernel<dh(), m3()>;
          allow_lds<kernel>(fused256_lds_bytes(dh()));
          ImtProfScope prof("attn_bwd_fused256_bf16", 10.0 * work, io, st);
          return launch(kernel, p.B * p.H, 512, fused256_lds_bytes(dh()), st, p);
        });
      });
  }
  const double io = attn_io(p, head_dim, sizeof(T), 2.0, 2.0) * 1.5;
  return by_head_dim(head_dim, [&](auto dh) {
    {
      ImtProfScope prof(sizeof(T) == 2 ? "attn_bwd_dq_bf16" : "attn_bwd_dq_f32", 6.0 * work, io, st);
      const int rc = by_mask3d(p, [&](auto m3) { return launch(attn_bwd_dq_kernel<T, dh(), m3()>, imt_cdiv(p.Tq, 64) * p.H * p.B, 256, 0, st, p); });
      if (rc) return rc;
    }
    ImtProfScope prof(sizeof(T) == 2 ? "attn_bwd_dkdv_bf16" : "attn_bwd_dkdv_f32", 8.0 * work, io, st);
    return by_mask3d(p, [&](auto m3) { return launch(attn_bwd_dkdv_kernel<T, dh(), m3()>, imt_cdiv(p.Tk, 64) * p.H * p.B, 256, 0, st, p); });
  });
}

}  // namespace

extern "C" int imt_attention_fwd(const imt_attn_args* a, void* stream) {
  int rc = check_args(a, false);
  if (rc) return rc;
  const AttnP p = make_params(a);
  const FwdKernel k = plan_fwd(a->dtype, a->head_dim, a->B, a->H, a->Tq, a->Tk, a->mask3d != nullptr, read_switches());
  return imt_by_dtype(a->dtype, [&](auto tag) { return launch_fwd<typename decltype(tag)::type>(k, p, a->head_dim, (hipStream_t)stream); });
}

extern "C" int imt_attention_bwd(const imt_attn_args* a, void* stream) {
  int rc = check_args(a, true);
  if (rc) return rc;
  const AttnP p = make_params(a);
  const BwdKernel k = plan_bwd(a->dtype, a->head_dim, a->B, a->H, a->Tq, a->Tk, a->mask3d != nullptr, read_switches());
  return imt_by_dtype(a->dtype, [&](auto tag) { return launch_bwd<typename decltype(tag)::type>(k, p, a->head_dim, (hipStream_t)stream); });
}

// Where imt_attention_bwd_proj applies: where imt_attention_bwd runs the fused kernel (the instance this one is a variant of), at
// head_dim 64 without a 3-D mask.  The shape query knows no batch size and plans for one batch element; the call plans for all.
static bool bwd_proj_ok(int dtype, int head_dim, int H, int Tq, int Tk, int d_model, bool has_mask3d, const AttnSwitches& sw) {
  return dtype == IMT_BF16 && head_dim == 64 && H > 0 && H * 64 == d_model && Tq > 0 && Tk > 0 && !has_mask3d &&
         plan_bwd(dtype, head_dim, 1, H, Tq, Tk, has_mask3d, sw) == BWD_FUSED;
}
extern "C" int imt_attention_bwd_proj_supported(int dtype, int head_dim, int H, int Tq, int Tk, int d_model, int has_mask3d) {
  return bwd_proj_ok(dtype, head_dim, H, Tq, Tk, d_model, has_mask3d != 0, read_switches());
}
// Attention backward with dO = dy W_o formed inside the launch (attn_bwd_proj_kernel) instead of by an NN product in front of
// imt_attention_bwd.  a: the backward's arguments; a->dO may be NULL (dO is then never stored) or point at a [B*Tq, >= d_model]
// buffer (lddo) that receives it.  dy [B*Tq, d_model] (lddy): the gradient of the projection's output; w_o [d_model, d_model]
// row-major (ldw), the projection's weight.  dQ / dK / dV (and dO) are bit-identical to the pair's.
extern "C" int imt_attention_bwd_proj(const imt_attn_args* a, const void* dy, int64_t lddy, const void* w_o, int64_t ldw, int d_model,
                                      void* stream) {
  int rc = check_args(a, true, false);
  if (rc) return rc;
  const AttnSwitches sw = read_switches();
  IMT_CHECK_ARG(bwd_proj_ok(a->dtype, a->head_dim, a->H, a->Tq, a->Tk, d_model, a->mask3d != nullptr, sw),
                "attention_bwd_proj: unsupported shape (bf16, head_dim 64, T <= 128, d_model = 64 H, no 3-D mask)");
  IMT_CHECK_ARG(dy && w_o && lddy >= d_model && ldw >= d_model && lddy % 8 == 0 && ldw % 8 == 0 &&
                (((uintptr_t)dy | (uintptr_t)w_o) & 15) == 0, "attention_bwd_proj: dy / w_o missing, misaligned or narrower than d_model");
  IMT_CHECK_ARG(plan_bwd(a->dtype, a->head_dim, a->B, a->H, a->Tq, a->Tk, false, sw) == BWD_FUSED,
                "attention_bwd_proj: too many score elements for 32-bit dropout indices");
  const AttnP p = make_params(a);
  ProjP pj;
  pj.dy = dy; pj.lddy = lddy; pj.w = w_o; pj.ldw = ldw; pj.d_model = d_model;
  hipStream_t st = (hipStream_t)stream;
  allow_lds<attn_bwd_proj_kernel<false>>(fused_lds_bytes(64));
  // (profiled under the kind of the kernel it is an instance of, with the projection's flops and bytes added: the suite pins the
  // short backward's dispatch by that kind)
  ImtProfScope prof("attn_bwd_fused_bf16", 10.0 * attn_work(p, 64) + 2.0 * p.B * p.Tq * (double)d_model * d_model,
                    attn_io(p, 64, 2, 3.0, 4.0) + 2.0 * p.B * p.Tq * d_model + 2.0 * d_model * d_model, st);
  ImtTrace tr("attn_bwd", p.B * p.H, st);
  return launch(attn_bwd_proj_kernel<false>, p.B * p.H, 512, fused_lds_bytes(64), st, traced(p, tr), pj);
}
