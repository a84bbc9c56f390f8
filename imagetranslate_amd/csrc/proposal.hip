// Lexical proposals of Seq2Seq (src/seq2seq.py:110-144): every decoder row attends over the word embeddings of its sentence's
// proposed translations, the result is mixed into the row through a learned per-channel gate, then LayerNorm.
//
//   e_j = table[prop[g, j]], s_j = <x_r, e_j>, p = softmax_j(s), c = sum_j p_j e_j (1e-8 everywhere when the whole group is pad),
//   sg = sigmoid(gate + 1e-8), z = sg x_r + (1 - sg) c, y_r = LayerNorm(z).
//
// Rows r of one group g = r / rows_per_group share the P gathered table rows E_g.  A workgroup (4 waves) takes one group and a tile
// of its rows; a wave owns RW rows at a time and a lane the columns lane * 4 + 256 k of each (x, the running sum and the other
// per-row vectors live in registers, KD = ceil(d / 256) f32x4 each).  E_g is walked in tiles of PT <= 64 proposals staged in LDS
// (<= 32 KB in either dtype: PT = 32768 / row bytes); a tile's scores sit one per lane, the softmax is the online one (running max,
// sum and weighted sum), and a probability reaches the other lanes by v_readlane.  Nothing of rows * P * d elements exists: the
// forward saves the raw scores [rows, P] and (softmax max and sum, LayerNorm mean and rstd) per row.
//
// Backward, five launches on the caller's workspace:
//   rows kernel   : recomputes c from the saved scores, LayerNorm / gate / softmax backward per row; writes dx, p and ds [rows, P],
//                   dc [rows, d], and per-workgroup partial sums of dgamma / dbeta / dsg;
//   fold kernel   : adds the partials in workgroup order into dgamma, dbeta, dgate (+=);
//   group kernel  : de[g, j] = sum over the rows r of g, in order, of p_rj dc_r + ds_rj x_r  -> workspace [G, P, d] fp32;
//   chain kernel  : for every entry of prop the next entry with the same id and whether an earlier one exists;
//   scatter kernel: the FIRST entry of every id adds its chain, in entry order, and then adds the sum to the table's gradient row --
//                   one writer per row, pad (and out-of-range) ids skipped.
// No float atomics and every sum in a fixed order: two calls on the same data give the same bits.
#include <type_traits>
#include "common.hpp"
#include <math.h>

namespace {

constexpr int PROP_THREADS = 256;
constexpr int PROP_WAVES = PROP_THREADS / 64;
constexpr int PROP_TILE_BYTES = 32768;  // E tile in LDS
constexpr int PROP_FWD_RW = 4;          // rows a wave owns at a time (forward: x and the running sum in registers)
constexpr int PROP_BWD_RW = 2;          // backward keeps four vectors per row
constexpr int PROP_GROUP_JI = 8;        // proposals per thread of the group kernel
constexpr int PROP_CHAIN_CHUNK = 1024;  // ids staged per step of the chain kernel

inline int prop_tile(int dtype, int d, int P) {
  int pt = PROP_TILE_BYTES / (d * imt_dtype_bytes(dtype));
  if (pt > 64) pt = 64;
  if (pt > P) pt = P;
  return pt < 1 ? 1 : pt;
}
inline int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

struct PropWs {
  int64_t p, ds, dc, part, de, next, first, total;  // byte offsets
  int64_t nwg;
};
inline PropWs prop_ws_layout(int64_t rows, int rpg, int P, int d) {
  PropWs w;
  const int64_t G = rows / rpg;
  const int rt = PROP_WAVES * PROP_BWD_RW;
  w.nwg = G * ((rpg + rt - 1) / rt);
  int64_t o = 0;
  w.p = o; o += align16(rows * P * 4);
  w.ds = o; o += align16(rows * P * 4);
  w.dc = o; o += align16(rows * (int64_t)d * 4);
  w.part = o; o += align16(w.nwg * 3 * d * 4);
  w.de = o; o += align16(G * P * d * 4);
  w.next = o; o += align16(G * P * 4);
  w.first = o; o += align16(G * P * 4);
  w.total = o;
  return w;
}

// rows of the table named by prop[g, j0 .. j0 + cnt) -> LDS tile [cnt, d] (raw elements); an id outside [0, V) reads row 0
template <typename T>
IMT_DEVICE void stage_tile(T* es, const T* __restrict__ table, const int64_t* __restrict__ pg, int j0, int cnt, int d, int64_t V) {
  const int ncol4 = d >> 2;
  for (int i = threadIdx.x; i < cnt * ncol4; i += PROP_THREADS) {
    const int j = i / ncol4, c = (i - j * ncol4) * 4;
    int64_t id = pg[j0 + j];
    if (id < 0 || id >= V) id = 0;
    *reinterpret_cast<typename Vec4<T>::type*>(es + (int64_t)j * d + c) = Vec4<T>::load_raw(table + id * d + c);
  }
}

IMT_DEVICE float lane_bcast(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }
IMT_DEVICE float dot4p(f32x4 a, f32x4 b) { return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]; }
IMT_DEVICE float sum4(f32x4 a) { return (a[0] + a[1]) + (a[2] + a[3]); }
IMT_DEVICE f32x4 sigmoid4(f32x4 g) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = 1.0f / (1.0f + expf(-(g[e] + 1e-8f)));
  return r;
}

// does the group hold anything but pad?  every thread must call
IMT_DEVICE bool group_all_pad(const int64_t* __restrict__ pg, int P, int64_t pad) {
  int any = 0;
  for (int j = threadIdx.x; j < P; j += PROP_THREADS) any |= pg[j] != pad;
  return !__syncthreads_or(any);
}

template <typename T, int KD>
__global__ __launch_bounds__(PROP_THREADS) void prop_fwd_kernel(const T* __restrict__ x, const T* __restrict__ table,
                                                                const int64_t* __restrict__ prop, const float* __restrict__ gate,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                T* __restrict__ y, float* __restrict__ scores, float* __restrict__ stats,
                                                                int rpg, int P, int d, int64_t V, int64_t pad, float eps, int PT,
                                                                int tiles_per_group) {
  constexpr int RW = PROP_FWD_RW;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* es = reinterpret_cast<T*>(smem);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g = blockIdx.x / tiles_per_group;
  const int rt = blockIdx.x % tiles_per_group;
  const int64_t* pg = prop + g * P;
  const bool all_pad = group_all_pad(pg, P, pad);
  bool cv[KD];
  int col[KD];
#pragma unroll
  for (int k = 0; k < KD; ++k) { col[k] = lane * 4 + 256 * k; cv[k] = col[k] < d; }
  bool rv[RW];
  int64_t row[RW];
  f32x4 xv[RW][KD], acc[RW][KD];
  float m[RW], l[RW];
#pragma unroll
  for (int i = 0; i < RW; ++i) {
    const int rg = rt * (PROP_WAVES * RW) + i * PROP_WAVES + wave;
    rv[i] = rg < rpg;
    row[i] = g * rpg + (rv[i] ? rg : 0);
    m[i] = -INFINITY; l[i] = 0.f;
#pragma unroll
    for (int k = 0; k < KD; ++k) {
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      xv[i][k] = (rv[i] && cv[k]) ? Vec4<T>::load(x + row[i] * d + col[k]) : zero;
      acc[i][k] = zero;
    }
  }
  for (int j0 = 0; j0 < P; j0 += PT) {
    const int cnt = min(PT, P - j0);
    __syncthreads();  // the previous tile has been read
    stage_tile<T>(es, table, pg, j0, cnt, d, V);
    __syncthreads();
    float s[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) s[i] = -INFINITY;
    for (int j = 0; j < cnt; ++j) {
      f32x4 ev[KD];
#pragma unroll
      for (int k = 0; k < KD; ++k) ev[k] = cv[k] ? Vec4<T>::load(es + (int64_t)j * d + col[k]) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < RW; ++i) {
        float part = 0.f;
#pragma unroll
        for (int k = 0; k < KD; ++k) part += dot4p(xv[i][k], ev[k]);
        part = wave_sum(part);
        if (lane == j) s[i] = part;
      }
    }
    float p[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
      if (rv[i] && lane < cnt) scores[row[i] * P + j0 + lane] = s[i];
      const float mn = fmaxf(m[i], wave_max(s[i]));
      const float alpha = expf(m[i] - mn);
      p[i] = lane < cnt ? expf(s[i] - mn) : 0.f;
      l[i] = l[i] * alpha + wave_sum(p[i]);
      m[i] = mn;
#pragma unroll
      for (int k = 0; k < KD; ++k) acc[i][k] *= alpha;
    }
    for (int j = 0; j < cnt; ++j) {
      f32x4 ev[KD];
#pragma unroll
      for (int k = 0; k < KD; ++k) ev[k] = cv[k] ? Vec4<T>::load(es + (int64_t)j * d + col[k]) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < RW; ++i) {
        const float pj = lane_bcast(p[i], j);
#pragma unroll
        for (int k = 0; k < KD; ++k) acc[i][k] += ev[k] * pj;
      }
    }
  }
  // gate, LayerNorm, store
  const float inv_d = 1.0f / (float)d;
#pragma unroll
  for (int i = 0; i < RW; ++i) {
    f32x4 z[KD];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < KD; ++k) {
      z[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (cv[k]) {
        const f32x4 sg = sigmoid4(Vec4<float>::load(gate + col[k]));
        const f32x4 c = all_pad ? f32x4{1e-8f, 1e-8f, 1e-8f, 1e-8f} : acc[i][k] / l[i];
        z[k] = sg * xv[i][k] + (1.0f - sg) * c;
        sum += sum4(z[k]);
      }
    }
    const float mean = wave_sum(sum) * inv_d;
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < KD; ++k)
      if (cv[k]) { const f32x4 dz = z[k] - mean; sq += dot4p(dz, dz); }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) * inv_d + eps);
    if (rv[i]) {
#pragma unroll
      for (int k = 0; k < KD; ++k)
        if (cv[k])
          Vec4<T>::store(y + row[i] * d + col[k], (z[k] - mean) * rstd * Vec4<float>::load(gamma + col[k]) + Vec4<float>::load(beta + col[k]));
      if (lane == 0) {
        stats[row[i] * 4 + 0] = m[i];
        stats[row[i] * 4 + 1] = l[i];
        stats[row[i] * 4 + 2] = mean;
        stats[row[i] * 4 + 3] = rstd;
      }
    }
  }
}

template <typename T, int KD>
__global__ __launch_bounds__(PROP_THREADS) void prop_bwd_rows_kernel(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ table,
                                                                     const int64_t* __restrict__ prop, const float* __restrict__ gate,
                                                                     const float* __restrict__ gamma, const float* __restrict__ scores,
                                                                     const float* __restrict__ stats, T* __restrict__ dx,
                                                                     float* __restrict__ ws_p, float* __restrict__ ws_ds, float* __restrict__ ws_dc,
                                                                     float* __restrict__ ws_part, int rpg, int P, int d, int64_t V, int64_t pad,
                                                                     int PT, int tiles_per_group, int tile_bytes) {
  constexpr int RW = PROP_BWD_RW;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* es = reinterpret_cast<T*>(smem);
  float* red = reinterpret_cast<float*>(smem + tile_bytes);  // [3, d]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g = blockIdx.x / tiles_per_group;
  const int rt = blockIdx.x % tiles_per_group;
  const int64_t* pg = prop + g * P;
  const bool all_pad = group_all_pad(pg, P, pad);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  bool cv[KD];
  int col[KD];
#pragma unroll
  for (int k = 0; k < KD; ++k) { col[k] = lane * 4 + 256 * k; cv[k] = col[k] < d; }
  bool rv[RW];
  int64_t row[RW];
  float smax[RW], ssum[RW];  // p_j = exp(s_j - max) / sum, the forward's own rounding
  f32x4 va[RW][KD];  // c, then dc
  f32x4 vb[RW][KD];  // the part of dx that is sg dz, then all of dx
#pragma unroll
  for (int i = 0; i < RW; ++i) {
    const int rg = rt * (PROP_WAVES * RW) + i * PROP_WAVES + wave;
    rv[i] = rg < rpg;
    row[i] = g * rpg + (rv[i] ? rg : 0);
    smax[i] = stats[row[i] * 4 + 0];
    ssum[i] = stats[row[i] * 4 + 1];
#pragma unroll
    for (int k = 0; k < KD; ++k) va[i][k] = zero;
  }
  // c = sum_j p_j e_j from the saved scores; p -> workspace
  for (int j0 = 0; j0 < P; j0 += PT) {
    const int cnt = min(PT, P - j0);
    __syncthreads();
    stage_tile<T>(es, table, pg, j0, cnt, d, V);
    __syncthreads();
    float p[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
      p[i] = lane < cnt ? expf(scores[row[i] * P + j0 + lane] - smax[i]) / ssum[i] : 0.f;
      if (rv[i] && lane < cnt) ws_p[row[i] * P + j0 + lane] = p[i];
    }
    for (int j = 0; j < cnt; ++j) {
#pragma unroll
      for (int k = 0; k < KD; ++k) {
        const f32x4 ev = cv[k] ? Vec4<T>::load(es + (int64_t)j * d + col[k]) : zero;
#pragma unroll
        for (int i = 0; i < RW; ++i) va[i][k] += ev * lane_bcast(p[i], j);
      }
    }
  }
  // LayerNorm and gate backward
  const float inv_d = 1.0f / (float)d;
  f32x4 pgam[KD], pbet[KD], psg[KD];
#pragma unroll
  for (int k = 0; k < KD; ++k) pgam[k] = pbet[k] = psg[k] = zero;
  float D[RW];
#pragma unroll
  for (int i = 0; i < RW; ++i) {
    const float mean = stats[row[i] * 4 + 2], rstd = stats[row[i] * 4 + 3];
    f32x4 zh[KD], dzh[KD], xc[KD], sgv[KD];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < KD; ++k) {
      zh[k] = dzh[k] = xc[k] = sgv[k] = zero;
      if (cv[k] && rv[i]) {
        const f32x4 xv = Vec4<T>::load(x + row[i] * d + col[k]);
        const f32x4 dyv = Vec4<T>::load(dy + row[i] * d + col[k]);
        const f32x4 c = all_pad ? f32x4{1e-8f, 1e-8f, 1e-8f, 1e-8f} : va[i][k];
        va[i][k] = c;
        sgv[k] = sigmoid4(Vec4<float>::load(gate + col[k]));
        const f32x4 z = sgv[k] * xv + (1.0f - sgv[k]) * c;
        zh[k] = (z - mean) * rstd;
        dzh[k] = dyv * Vec4<float>::load(gamma + col[k]);
        xc[k] = xv - c;
        pgam[k] += dyv * zh[k];
        pbet[k] += dyv;
        s1 += sum4(dzh[k]);
        s2 += dot4p(dzh[k], zh[k]);
      }
    }
    s1 = wave_sum(s1) * inv_d;
    s2 = wave_sum(s2) * inv_d;
    float dd = 0.f;
#pragma unroll
    for (int k = 0; k < KD; ++k) {
      f32x4 dc = zero, dxs = zero;
      if (cv[k] && rv[i]) {
        const f32x4 dz = (dzh[k] - s1 - zh[k] * s2) * rstd;
        psg[k] += dz * xc[k];
        dxs = sgv[k] * dz;
        if (!all_pad) dc = (1.0f - sgv[k]) * dz;
        dd += dot4p(dc, va[i][k]);
        Vec4<float>::store(ws_dc + row[i] * d + col[k], dc);
      }
      va[i][k] = dc;
      vb[i][k] = dxs;
    }
    D[i] = wave_sum(dd);  // sum_j p_j dp_j = <dc, c>
  }
  // softmax backward: dp_j = <dc, e_j>, ds_j = p_j (dp_j - D), dx += sum_j ds_j e_j
  for (int j0 = 0; j0 < P; j0 += PT) {
    const int cnt = min(PT, P - j0);
    __syncthreads();
    stage_tile<T>(es, table, pg, j0, cnt, d, V);
    __syncthreads();
    float dp[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) dp[i] = 0.f;
    for (int j = 0; j < cnt; ++j) {
      f32x4 ev[KD];
#pragma unroll
      for (int k = 0; k < KD; ++k) ev[k] = cv[k] ? Vec4<T>::load(es + (int64_t)j * d + col[k]) : zero;
#pragma unroll
      for (int i = 0; i < RW; ++i) {
        float part = 0.f;
#pragma unroll
        for (int k = 0; k < KD; ++k) part += dot4p(va[i][k], ev[k]);
        part = wave_sum(part);
        if (lane == j) dp[i] = part;
      }
    }
    float ds[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
      const float p = lane < cnt ? expf(scores[row[i] * P + j0 + lane] - smax[i]) / ssum[i] : 0.f;
      ds[i] = p * (dp[i] - D[i]);
      if (rv[i] && lane < cnt) ws_ds[row[i] * P + j0 + lane] = ds[i];
    }
    for (int j = 0; j < cnt; ++j) {
#pragma unroll
      for (int k = 0; k < KD; ++k) {
        const f32x4 ev = cv[k] ? Vec4<T>::load(es + (int64_t)j * d + col[k]) : zero;
#pragma unroll
        for (int i = 0; i < RW; ++i) vb[i][k] += ev * lane_bcast(ds[i], j);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < RW; ++i)
    if (rv[i]) {
#pragma unroll
      for (int k = 0; k < KD; ++k)
        if (cv[k]) Vec4<T>::store(dx + row[i] * d + col[k], vb[i][k]);
    }
  // this workgroup's sums over its rows of dy zhat, dy and dz (x - c): the waves add in turn
  for (int w = 0; w < PROP_WAVES; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int k = 0; k < KD; ++k)
        if (cv[k]) {
          f32x4 a = pgam[k], b = pbet[k], c = psg[k];
          if (w > 0) {
            a += Vec4<float>::load(red + col[k]);
            b += Vec4<float>::load(red + d + col[k]);
            c += Vec4<float>::load(red + 2 * d + col[k]);
          }
          Vec4<float>::store(red + col[k], a);
          Vec4<float>::store(red + d + col[k], b);
          Vec4<float>::store(red + 2 * d + col[k], c);
        }
    }
  }
  __syncthreads();
  float* part = ws_part + (int64_t)blockIdx.x * 3 * d;
  for (int i = threadIdx.x; i < 3 * d; i += PROP_THREADS) part[i] = red[i];
}

// dgamma, dbeta += the partial sums in workgroup order; dgate += (sum of the dsg partials) sg (1 - sg)
__global__ __launch_bounds__(256) void prop_fold_kernel(const float* __restrict__ part, const float* __restrict__ gate, float* __restrict__ dgate,
                                                       float* __restrict__ dgamma, float* __restrict__ dbeta, int64_t nwg, int d) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * d) return;
  float s = 0.f;
#pragma unroll 8
  for (int64_t w = 0; w < nwg; ++w) s += part[w * 3 * d + i];
  const int which = i / d, c = i - which * d;
  if (which == 0) dgamma[c] += s;
  else if (which == 1) dbeta[c] += s;
  else {
    const float sg = 1.0f / (1.0f + expf(-(gate[c] + 1e-8f)));
    dgate[c] += s * sg * (1.0f - sg);
  }
}

// de[g, j, :] = sum over the rows r of group g, in order, of p_rj dc_r + ds_rj x_r.  Thread (jsub, cg): columns cg * 4 .. + 3 of the
// proposals j0 + jsub + JG i, i < PROP_GROUP_JI, JG = 256 / (d / 4).
template <typename T>
__global__ __launch_bounds__(PROP_THREADS) void prop_bwd_group_kernel(const T* __restrict__ x, const float* __restrict__ ws_p,
                                                                      const float* __restrict__ ws_ds, const float* __restrict__ ws_dc,
                                                                      float* __restrict__ de, int rpg, int P, int d, int jtiles) {
  constexpr int JI = PROP_GROUP_JI;
  const int ncol4 = d >> 2, JG = PROP_THREADS / ncol4;
  const int cg = threadIdx.x % ncol4, jsub = threadIdx.x / ncol4;
  if (jsub >= JG) return;  // no barrier in this kernel
  const int64_t g = blockIdx.x / jtiles;
  const int j0 = (blockIdx.x % jtiles) * (JG * JI);
  f32x4 acc[JI];
  int jj[JI];
#pragma unroll
  for (int i = 0; i < JI; ++i) {
    acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    jj[i] = j0 + jsub + JG * i;
  }
  for (int r = 0; r < rpg; ++r) {
    const int64_t row = g * rpg + r;
    const f32x4 dc = Vec4<float>::load(ws_dc + row * d + cg * 4);
    const f32x4 xv = Vec4<T>::load(x + row * d + cg * 4);
#pragma unroll
    for (int i = 0; i < JI; ++i)
      if (jj[i] < P) acc[i] += dc * ws_p[row * P + jj[i]] + xv * ws_ds[row * P + jj[i]];
  }
#pragma unroll
  for (int i = 0; i < JI; ++i)
    if (jj[i] < P) Vec4<float>::store(de + (g * P + jj[i]) * d + cg * 4, acc[i]);
}

// entry i of prop (flattened [G * P]): next[i] = the next entry with the same id or -1, first[i] = 1 when no earlier entry has it.
// Pad and out-of-range ids: first 0, next -1 (they get no gradient).
__global__ __launch_bounds__(256) void prop_chain_kernel(const int64_t* __restrict__ prop, int* __restrict__ next, int* __restrict__ first,
                                                        int n, int64_t V, int64_t pad) {
  __shared__ int64_t ids[PROP_CHAIN_CHUNK];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int64_t mine = i < n ? prop[i] : pad;
  const bool live = i < n && mine != pad && mine >= 0 && mine < V;
  int nx = -1, has_prev = 0;
  for (int k0 = 0; k0 < n; k0 += PROP_CHAIN_CHUNK) {
    const int cnt = min(PROP_CHAIN_CHUNK, n - k0);
    __syncthreads();
    for (int k = threadIdx.x; k < cnt; k += 256) ids[k] = prop[k0 + k];
    __syncthreads();
    if (live) {
      for (int k = 0; k < cnt; ++k) {
        const int kk = k0 + k;
        if (ids[k] == mine) {
          has_prev |= kk < i;
          if (kk > i && nx < 0) nx = kk;
        }
      }
    }
  }
  if (i < n) {
    next[i] = live ? nx : -1;
    first[i] = live && !has_prev;
  }
}

// one workgroup per entry; only the first entry of an id works: dtable[id] += the sum of its chain's de rows, in entry order
__global__ __launch_bounds__(256) void prop_scatter_kernel(const int64_t* __restrict__ prop, const int* __restrict__ next,
                                                          const int* __restrict__ first, const float* __restrict__ de,
                                                          float* __restrict__ dtable, int d) {
  const int i = blockIdx.x;
  if (!first[i]) return;
  const int t = threadIdx.x;
  if (t >= (d >> 2)) return;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = i; k >= 0; k = next[k]) acc += Vec4<float>::load(de + (int64_t)k * d + t * 4);
  float* out = dtable + prop[i] * d + t * 4;
  Vec4<float>::store(out, Vec4<float>::load(out) + acc);
}

// what both entry points refuse, in the order dtype, rows, rows_per_group, P, d
int prop_validate(const char* what, int dtype, int64_t rows, int rpg, int P, int d, int64_t vocab) {
  IMT_CHECK_ARG(imt_ok_dtype(dtype), "%s: bad dtype", what);
  IMT_CHECK_ARG(rows >= 0 && rows <= 0x7fffffff, "%s: row count outside [0, 2^31)", what);
  IMT_CHECK_ARG(rpg >= 1, "%s: rows_per_group must be at least 1", what);
  IMT_CHECK_ARG(rows % rpg == 0, "%s: rows is not a multiple of rows_per_group", what);
  IMT_CHECK_ARG(P >= 1, "%s: P must be at least 1", what);
  IMT_CHECK_ARG((rows / rpg) * (int64_t)P <= 0x7fffffff, "%s: more than 2^31 proposal entries", what);
  IMT_CHECK_ARG(vocab >= 1, "%s: empty table", what);
  if (d < 4 || d % 4 != 0 || d > IMT_PROPOSAL_MAX_D) {
    imt_set_error("%s: d must be a multiple of 4 in [4, %d]", what, IMT_PROPOSAL_MAX_D);
    return IMT_ERR_UNSUPPORTED;
  }
  return IMT_OK;
}

template <typename F> int by_kd(int d, F&& f) {
  switch ((d + 255) / 256) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    default: return f(std::integral_constant<int, 4>());
  }
}

}  // namespace

extern "C" int64_t imt_proposal_attn_ws_bytes(int64_t rows, int rows_per_group, int P, int d) {
  const int rc = prop_validate("proposal_attn_ws_bytes", IMT_F32, rows, rows_per_group, P, d, 1);
  if (rc != IMT_OK) return rc;
  return prop_ws_layout(rows, rows_per_group, P, d).total;
}

extern "C" int imt_proposal_attn_fwd(int dtype, const void* x, const void* table, const int64_t* prop, const float* gate,
                                     const float* gamma, const float* beta, void* y, float* scores, float* stats, int64_t rows,
                                     int rows_per_group, int P, int d, int64_t vocab, int64_t pad_idx, float eps, void* stream) {
  const int rc = prop_validate("proposal_attn_fwd", dtype, rows, rows_per_group, P, d, vocab);
  if (rc != IMT_OK) return rc;
  if (rows == 0) return IMT_OK;
  IMT_CHECK_ARG(x && table && prop && gate && gamma && beta && y && scores && stats, "proposal_attn_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int PT = prop_tile(dtype, d, P);
  const int rt = PROP_WAVES * PROP_FWD_RW;
  const int tiles = (rows_per_group + rt - 1) / rt;
  const int64_t nwg = (rows / rows_per_group) * tiles;
  IMT_CHECK_ARG(nwg <= 0x7fffffff, "proposal_attn_fwd: too many workgroups");
  const size_t lds = (size_t)PT * d * imt_dtype_bytes(dtype);
  ImtProfScope prof("proposal_attn_fwd", 4.0 * rows * P * d, (double)nwg * P * d * imt_dtype_bytes(dtype), st);
  return imt_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return by_kd(d, [&](auto kd) {
      constexpr int KD = decltype(kd)::value;
      hipLaunchKernelGGL((prop_fwd_kernel<T, KD>), dim3((unsigned)nwg), dim3(PROP_THREADS), lds, st, (const T*)x, (const T*)table, prop, gate,
                         gamma, beta, (T*)y, scores, stats, rows_per_group, P, d, vocab, pad_idx, eps, PT, tiles);
      IMT_CHECK_LAUNCH();
      return IMT_OK;
    });
  });
}

extern "C" int imt_proposal_attn_bwd(int dtype, const void* dy, const void* x, const void* table, const int64_t* prop, const float* gate,
                                     const float* gamma, const float* scores, const float* stats, void* dx, float* dtable, float* dgate,
                                     float* dgamma, float* dbeta, void* ws, int64_t ws_bytes, int64_t rows, int rows_per_group, int P, int d,
                                     int64_t vocab, int64_t pad_idx, void* stream) {
  const int rc = prop_validate("proposal_attn_bwd", dtype, rows, rows_per_group, P, d, vocab);
  if (rc != IMT_OK) return rc;
  if (rows == 0) return IMT_OK;
  IMT_CHECK_ARG(dy && x && table && prop && gate && gamma && scores && stats && dx && dtable && dgate && dgamma && dbeta && ws,
                "proposal_attn_bwd: null pointer");
  const PropWs w = prop_ws_layout(rows, rows_per_group, P, d);
  IMT_CHECK_ARG(ws_bytes >= w.total, "proposal_attn_bwd: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)w.total);
  IMT_CHECK_ARG(((uintptr_t)ws & 15) == 0, "proposal_attn_bwd: workspace not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  unsigned char* base = (unsigned char*)ws;
  float* ws_p = (float*)(base + w.p);
  float* ws_ds = (float*)(base + w.ds);
  float* ws_dc = (float*)(base + w.dc);
  float* ws_part = (float*)(base + w.part);
  float* ws_de = (float*)(base + w.de);
  int* ws_next = (int*)(base + w.next);
  int* ws_first = (int*)(base + w.first);
  const int64_t G = rows / rows_per_group;
  const int n_entries = (int)(G * P);
  const int PT = prop_tile(dtype, d, P);
  const int tiles = (rows_per_group + PROP_WAVES * PROP_BWD_RW - 1) / (PROP_WAVES * PROP_BWD_RW);
  const int tile_bytes = (int)align16((int64_t)PT * d * imt_dtype_bytes(dtype));
  const size_t lds = (size_t)tile_bytes + (size_t)3 * d * 4;
  const int JT = (PROP_THREADS / (d >> 2)) * PROP_GROUP_JI;
  const int jtiles = (P + JT - 1) / JT;
  IMT_CHECK_ARG(w.nwg <= 0x7fffffff && G * jtiles <= 0x7fffffff, "proposal_attn_bwd: too many workgroups");
  ImtProfScope prof("proposal_attn_bwd", 12.0 * rows * P * d, 2.0 * w.nwg * P * d * imt_dtype_bytes(dtype) + 8.0 * G * P * d, st);
  return imt_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const int rc2 = by_kd(d, [&](auto kd) {
      constexpr int KD = decltype(kd)::value;
      hipLaunchKernelGGL((prop_bwd_rows_kernel<T, KD>), dim3((unsigned)w.nwg), dim3(PROP_THREADS), lds, st, (const T*)dy, (const T*)x,
                         (const T*)table, prop, gate, gamma, scores, stats, (T*)dx, ws_p, ws_ds, ws_dc, ws_part, rows_per_group, P, d, vocab,
                         pad_idx, PT, tiles, tile_bytes);
      IMT_CHECK_LAUNCH();
      return IMT_OK;
    });
    if (rc2 != IMT_OK) return rc2;
    hipLaunchKernelGGL(prop_fold_kernel, dim3(imt_cdiv(3 * d, 256)), dim3(256), 0, st, ws_part, gate, dgate, dgamma, dbeta, w.nwg, d);
    IMT_CHECK_LAUNCH();
    hipLaunchKernelGGL(prop_bwd_group_kernel<T>, dim3((unsigned)(G * jtiles)), dim3(PROP_THREADS), 0, st, (const T*)x, ws_p, ws_ds, ws_dc, ws_de,
                       rows_per_group, P, d, jtiles);
    IMT_CHECK_LAUNCH();
    hipLaunchKernelGGL(prop_chain_kernel, dim3(imt_cdiv(n_entries, 256)), dim3(256), 0, st, prop, ws_next, ws_first, n_entries, vocab, pad_idx);
    IMT_CHECK_LAUNCH();
    hipLaunchKernelGGL(prop_scatter_kernel, dim3((unsigned)n_entries), dim3(256), 0, st, prop, ws_next, ws_first, ws_de, dtable, d);
    IMT_CHECK_LAUNCH();
    return IMT_OK;
  });
}
