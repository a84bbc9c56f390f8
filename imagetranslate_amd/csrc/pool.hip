// Contrastive tail of ImageMassSeq2Seq (src/image_model.py:231-264): one-vector attention pooling of a [rows, S, d] tensor to
// unit vectors (forward and backward), and the image-to-text contrastive loss with its gradients.
//
// Pooling, one workgroup (4 waves) per sentence:
//   score_s = x_s . w + b, a masked position is set to exactly -10000 (masked_fill, :241,246), p = softmax(score),
//   v = sum_s p_s x_s, u = v / (|v| + 1e-4) (:255-258).
// x is read from HBM once when the sentence fits in LDS beside the small per-position arrays (imt_attn_pool_plan == 1): the
// score pass keeps the raw elements in LDS and the weighted sum reads them there.  Otherwise (plan 2) the weighted sum reads
// x a second time; nothing reads it a third time.  The backward follows the same plan: dp_s = dv . x_s is the first read, the
// pass that writes dx and accumulates dw the second.  All statistics and sums are fp32 and every reduction has a fixed order
// (wave butterflies, then partial sums added in index order; dw / db as per-sentence partials folded in sentence order by a
// second launch): the same call on the same data gives the same bits.
//
// Sentence pooling of Caption2Image (src/image_model.py:430-436) is the same four phases -- row scores, masked softmax, weighted
// sum, store -- on xd = dropout(x) (training), without the normalisation, and v is written in the compute dtype (it feeds the
// decoder GEMM).  One kernel pair serves both, templated on the kind; LDS keeps the RAW sentence either way, the dropout factor
// of an element is recomputed from its index wherever the element is used.
#include <type_traits>
#include "common.hpp"
#include <math.h>

namespace {

constexpr int POOL_THREADS = 256;
constexpr int POOL_PART_FLOATS = 1024;  // column-group partial sums: (256 / (d / 4)) groups x d floats <= 1024
enum PoolKind { POOL_UNIT, POOL_SENT };  // unit vectors u = v / (|v| + 1e-4) in fp32 | v of dropout(x) in the compute dtype
template <typename T, int KIND> using pool_out_t = typename std::conditional<KIND == POOL_UNIT, float, T>::type;  // of u / du | v / dv

inline int round4(int s) { return (s + 3) & ~3; }
// LDS besides x: reduction scratch, two per-position arrays (scores / probabilities), the partial sums, one d-vector
inline int64_t pool_small_bytes(int S, int d) { return 64 + 2 * (int64_t)round4(S) * 4 + POOL_PART_FLOATS * 4 + (int64_t)d * 4; }
inline int64_t pool_x_bytes(int dtype, int S, int d) { return (int64_t)S * d * imt_dtype_bytes(dtype); }

struct PoolLds {
  float* red; float* sc; float* pr; float* part; float* vec; unsigned char* xs;
};
IMT_DEVICE PoolLds pool_lds(unsigned char* smem, int S, int d) {
  PoolLds l;
  const int S4 = (S + 3) & ~3;
  l.red = reinterpret_cast<float*>(smem);
  l.sc = l.red + 16;
  l.pr = l.sc + S4;
  l.part = l.pr + S4;
  l.vec = l.part + POOL_PART_FLOATS;
  l.xs = reinterpret_cast<unsigned char*>(l.vec + d);
  return l;
}

// sums / maxima over the 256 threads in a fixed order; every thread must call
IMT_DEVICE float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
IMT_DEVICE float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
IMT_DEVICE float dot4(f32x4 a, f32x4 b) { return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]; }

// Dropout of the pooled tensor (sentence pooling of Caption2Image): the decision for element i of the flattened tensor is the one
// imt_add_rows_dropout makes under the same seed; base = flat index of the sentence's first element.  thresh == 0: no dropout.
struct PoolDrop {
  uint32_t thresh; float inv_keep; uint64_t seed, base;
};
// 1 / (1 - p) where elements idx0 .. idx0 + 3 (idx0 % 4 == 0) are kept, 0 where they are dropped
IMT_DEVICE f32x4 drop_scale4(const PoolDrop& dr, uint64_t idx0) {
  f32x4 s = {1.f, 1.f, 1.f, 1.f};
  dropout_apply4(s, dr.seed, idx0, dr.thresh, dr.inv_keep);
  return s;
}

// dot product of every position's row with vec[0..d) (global T or LDS fp32), one wave per position; out[s] = the sum.  The raw
// elements are kept in LDS when keep_x.  DROP: the row is dropout(x) (the raw elements are what LDS keeps).
template <typename T, typename TV, bool DROP = false>
IMT_DEVICE void row_dots(const T* __restrict__ xr, const TV* __restrict__ vec, T* xs, float* out, int S, int d, bool keep_x,
                         const PoolDrop dr = PoolDrop()) {
  constexpr int U = 4;  // positions per wave iteration: their loads are in flight together (one position's sum order is unchanged)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s0 = wave * U; s0 < S; s0 += (POOL_THREADS / 64) * U) {
    float acc[U] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane * 4; c < d; c += 256) {
      const f32x4 vv = Vec4<TV>::load(vec + c);
      typename Vec4<T>::type raw[U];
#pragma unroll
      for (int k = 0; k < U; ++k)
        if (s0 + k < S) raw[k] = Vec4<T>::load_raw(xr + (int64_t)(s0 + k) * d + c);
#pragma unroll
      for (int k = 0; k < U; ++k)
        if (s0 + k < S) {
          if (keep_x) *reinterpret_cast<typename Vec4<T>::type*>(xs + (int64_t)(s0 + k) * d + c) = raw[k];
          if constexpr (DROP) {
            f32x4 xv = Vec4<T>::cvt(raw[k]);
            if (dr.thresh) xv *= drop_scale4(dr, dr.base + (uint64_t)(s0 + k) * d + c);
            acc[k] += dot4(xv, vv);
          } else {
            acc[k] += dot4(Vec4<T>::cvt(raw[k]), vv);
          }
        }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const float a = wave_sum(acc[k]);
      if (lane == 0 && s0 + k < S) out[s0 + k] = a;
    }
  }
}

// l.sc[s]: x_s . w  ->  p_s = softmax over s of (x_s . w + bias, or exactly -10000 where mask is 0); also written to probs
IMT_DEVICE void pool_softmax(const PoolLds& l, const uint8_t* __restrict__ mask, float* __restrict__ probs, float bias, int64_t row,
                             int S) {
  const int t = threadIdx.x;
  float m = -INFINITY;
  for (int s = t; s < S; s += POOL_THREADS) {
    const float v = (mask && !mask[row * S + s]) ? -10000.0f : l.sc[s] + bias;
    l.sc[s] = v;
    m = fmaxf(m, v);
  }
  m = block_max(m, l.red);
  float sum = 0.f;
  for (int s = t; s < S; s += POOL_THREADS) {
    const float e = expf(l.sc[s] - m);
    l.sc[s] = e;
    sum += e;
  }
  sum = block_sum(sum, l.red);
  const float inv = 1.0f / sum;
  for (int s = t; s < S; s += POOL_THREADS) {
    const float p = l.sc[s] * inv;
    l.sc[s] = p;
    probs[row * S + s] = p;
  }
  __syncthreads();
}

// The sums over s (v in the forward, dw in the backward) use a column-group layout: thread t = (g, cg), cg = t % (d/4),
// g = t / (d/4) < G = 256 / (d/4), adds positions g, g + G, ... of columns cg * 4 .. cg * 4 + 3 into its acc.  This adds the G
// partial vectors of every column group in the order g = 0, 1, ...: threads t < d / 4 return the total of column group t, the
// others zeros; every thread must call.
IMT_DEVICE f32x4 colgroup_fold(const PoolLds& l, int d, f32x4 acc) {
  const int t = threadIdx.x, ncol4 = d >> 2, G = POOL_THREADS / ncol4;
  const int cg = t % ncol4, g = t / ncol4;
  if (g < G) Vec4<float>::store(l.part + g * d + cg * 4, acc);
  __syncthreads();
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (t < ncol4)
    for (int k = 0; k < G; ++k) v += Vec4<float>::load(l.part + k * d + t * 4);
  return v;
}

template <typename T, int KIND>
__global__ __launch_bounds__(POOL_THREADS) void pool_fwd_kernel(const T* __restrict__ x, const T* __restrict__ w, const T* __restrict__ b,
                                                                const uint8_t* __restrict__ mask, pool_out_t<T, KIND>* __restrict__ out,
                                                                float* __restrict__ probs, float* __restrict__ norm, int S, int d,
                                                                int keep_x, uint32_t thresh, float inv_keep, uint64_t seed) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const PoolLds l = pool_lds(smem, S, d);
  T* xs = reinterpret_cast<T*>(l.xs);
  const int64_t row = blockIdx.x;
  const T* xr = x + row * S * d;
  const int t = threadIdx.x, ncol4 = d >> 2;
  const PoolDrop dr = {thresh, inv_keep, seed, (uint64_t)row * (uint64_t)S * (uint64_t)d};
  // scores (first read of x)
  row_dots<T, T, KIND == POOL_SENT>(xr, w, xs, l.sc, S, d, keep_x != 0, dr);
  __syncthreads();
  pool_softmax(l, mask, probs, to_f32<T>(b[0]), row, S);
  // weighted sum (second read of x, or LDS)
  const int G = POOL_THREADS / ncol4, cg = t % ncol4, g = t / ncol4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (g < G) {
#pragma unroll 4
    for (int s = g; s < S; s += G) {
      f32x4 xv = keep_x ? Vec4<T>::load(xs + (int64_t)s * d + cg * 4) : Vec4<T>::load(xr + (int64_t)s * d + cg * 4);
      if constexpr (KIND == POOL_SENT) {
        if (thresh) xv *= drop_scale4(dr, dr.base + (uint64_t)s * d + cg * 4);
      }
      acc += xv * l.sc[s];
    }
  }
  const f32x4 v = colgroup_fold(l, d, acc);
  if constexpr (KIND == POOL_UNIT) {
    const float ss = block_sum(dot4(v, v), l.red);
    const float r = sqrtf(ss);
    if (t < ncol4) Vec4<float>::store(out + row * d + t * 4, v * (1.0f / (r + 1e-4f)));
    if (t == 0) norm[row] = r;
  } else {
    if (t < ncol4) Vec4<T>::store(out + row * d + t * 4, v);
  }
}

// dx, and this sentence's partial dw [d] / db (folded by attn_pool_fold_kernel).  Unit vectors, u = v / (r + eps), r = |v|:
// dv = du / (r + eps) - u (du . u) / r; sentence pooling: dv as given.  With xd = x, or dropout(x) for the sentence pooling:
// dp_s = dv . xd_s;  dscore_s = p_s (dp_s - sum_t p_t dp_t), 0 at a masked position (its score is a constant);
// d(xd_s) = p_s dv + dscore_s w, and dx = the dropout's backward of that (same mask, same scale);  dw = sum_s dscore_s xd_s;
// db = sum_s dscore_s.
template <typename T, int KIND>
__global__ __launch_bounds__(POOL_THREADS) void pool_bwd_kernel(const T* __restrict__ x, const T* __restrict__ w, const uint8_t* __restrict__ mask,
                                                                const float* __restrict__ probs, const pool_out_t<T, KIND>* __restrict__ dout,
                                                                const float* __restrict__ u, const float* __restrict__ norm,
                                                                const float* __restrict__ du_scale, T* __restrict__ dx,
                                                                float* __restrict__ dw_part, float* __restrict__ db_part, int S, int d,
                                                                int keep_x, uint32_t thresh, float inv_keep, uint64_t seed) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const PoolLds l = pool_lds(smem, S, d);
  T* xs = reinterpret_cast<T*>(l.xs);
  const int64_t row = blockIdx.x;
  const T* xr = x + row * S * d;
  const int t = threadIdx.x, ncol4 = d >> 2;
  const PoolDrop dr = {thresh, inv_keep, seed, (uint64_t)row * (uint64_t)S * (uint64_t)d};
  // dv
  if constexpr (KIND == POOL_UNIT) {
    f32x4 uv = {0.f, 0.f, 0.f, 0.f}, gv = {0.f, 0.f, 0.f, 0.f};
    if (t < ncol4) {
      uv = Vec4<float>::load(u + row * d + t * 4);
      gv = Vec4<float>::load(dout + row * d + t * 4);
      if (du_scale) gv *= du_scale[0];
    }
    const float gu = block_sum(dot4(gv, uv), l.red);
    const float r = norm[row];
    const float coef = r > 0.f ? gu / r : 0.f;
    if (t < ncol4) Vec4<float>::store(l.vec + t * 4, gv * (1.0f / (r + 1e-4f)) - uv * coef);
  } else {
    if (t < ncol4) Vec4<float>::store(l.vec + t * 4, Vec4<T>::load(dout + row * d + t * 4));
  }
  for (int s = t; s < S; s += POOL_THREADS) l.pr[s] = probs[row * S + s];
  __syncthreads();
  // dp (first read of x)
  row_dots<T, float, KIND == POOL_SENT>(xr, l.vec, xs, l.sc, S, d, keep_x != 0, dr);
  __syncthreads();
  float c0 = 0.f;
  for (int s = t; s < S; s += POOL_THREADS) c0 += l.pr[s] * l.sc[s];
  c0 = block_sum(c0, l.red);
  float dbl = 0.f;
  for (int s = t; s < S; s += POOL_THREADS) {
    const float ds = (mask && !mask[row * S + s]) ? 0.f : l.pr[s] * (l.sc[s] - c0);
    l.sc[s] = ds;
    dbl += ds;
  }
  dbl = block_sum(dbl, l.red);
  // dx and dw (second read of x, or LDS)
  const int G = POOL_THREADS / ncol4, cg = t % ncol4, g = t / ncol4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (g < G) {
    const f32x4 wv = Vec4<T>::load(w + cg * 4), dv = Vec4<float>::load(l.vec + cg * 4);
#pragma unroll 4
    for (int s = g; s < S; s += G) {
      f32x4 xv = keep_x ? Vec4<T>::load(xs + (int64_t)s * d + cg * 4) : Vec4<T>::load(xr + (int64_t)s * d + cg * 4);
      const float ds = l.sc[s];
      f32x4 gx = dv * l.pr[s] + wv * ds;
      if constexpr (KIND == POOL_SENT) {
        if (thresh) {
          const f32x4 sc = drop_scale4(dr, dr.base + (uint64_t)s * d + cg * 4);
          xv *= sc;
          gx *= sc;
        }
      }
      Vec4<T>::store(dx + (row * S + s) * d + cg * 4, gx);
      acc += xv * ds;
    }
  }
  const f32x4 dwv = colgroup_fold(l, d, acc);
  if (t < ncol4) Vec4<float>::store(dw_part + row * d + t * 4, dwv);
  if (t == 0) db_part[row] = dbl;
}

// dw[c] += sum over sentences (in order) of dw_part[row, c]; thread d does the same for db
__global__ __launch_bounds__(256) void attn_pool_fold_kernel(const float* __restrict__ dw_part, const float* __restrict__ db_part,
                                                            float* __restrict__ dw, float* __restrict__ db, int64_t rows, int d) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c > d) return;
  float s = 0.f;
  if (c < d) {
    for (int64_t r = 0; r < rows; ++r) s += dw_part[r * d + c];
    dw[c] += s;
  } else {
    for (int64_t r = 0; r < rows; ++r) s += db_part[r];
    db[0] += s;
  }
}

// ------------------------------------------------------------------------------------------- L2 distance (Caption2Image loss)
// torch.dist(pred, target, 2) / B (src/train_txt2image.py:67) and its gradient in one call.  First launch: workgroup g adds
// the squared differences of its grid-stride share of the 4-element groups -> part[g]; second launch: every workgroup adds the
// partials in index order (the same bits everywhere), workgroup 0 writes the loss, all write dpred = (pred - target) / (r B),
// zeros where r == 0 (torch's subgradient of the norm at 0).
template <typename T>
__global__ __launch_bounds__(256) void l2_partial_kernel(const T* __restrict__ pred, const T* __restrict__ target, float* __restrict__ part,
                                                         int64_t n4) {
  __shared__ float red[16];
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 df = Vec4<T>::load(pred + i * 4) - Vec4<T>::load(target + i * 4);
    acc += dot4(df, df);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

template <typename T>
__global__ __launch_bounds__(256) void l2_scale_kernel(const T* __restrict__ pred, const T* __restrict__ target, const float* __restrict__ part,
                                                       int nparts, float* __restrict__ loss, T* __restrict__ dpred, int64_t n4, float inv_b) {
  __shared__ float ps[IMT_L2_DIST_PARTS];
  if ((int)threadIdx.x < nparts) ps[threadIdx.x] = part[threadIdx.x];
  __syncthreads();
  float ss = 0.f;
  for (int k = 0; k < nparts; ++k) ss += ps[k];
  const float r = sqrtf(ss);
  const float coef = ss > 0.f ? inv_b / r : 0.f;
  if (blockIdx.x == 0 && threadIdx.x == 0) loss[0] = r * inv_b;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)
    Vec4<T>::store(dpred + i * 4, (Vec4<T>::load(pred + i * 4) - Vec4<T>::load(target + i * 4)) * coef);
}

// ------------------------------------------------------------------------------------------- contrastive loss
// Workgroup i: C_ij = img_i . txt_j for every j, row loss log(sum_j exp C_ij + 1e-4) - (C_ii + 1e-4) (:260-262),
// dC_ij = (exp C_ij / (sum_j exp C_ij + 1e-4) - [i == j]) / B, d_img_i = sum_j dC_ij txt_j.
__global__ __launch_bounds__(POOL_THREADS) void contrastive_rows_kernel(const float* __restrict__ img, const float* __restrict__ txt,
                                                                        float* __restrict__ row_loss, float* __restrict__ dc,
                                                                        float* __restrict__ d_img, int B, int N, int d) {
  __shared__ float red[16];
  __shared__ float c[IMT_CONTRASTIVE_MAX_N];
  __shared__ __attribute__((aligned(16))) float iv[IMT_POOL_MAX_D];
  const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ncol4 = d >> 2;
  if (t < ncol4) Vec4<float>::store(iv + t * 4, Vec4<float>::load(img + (int64_t)i * d + t * 4));
  __syncthreads();
  for (int j = wave; j < N; j += POOL_THREADS / 64) {
    float acc = 0.f;
    for (int k = lane * 4; k < d; k += 256) acc += dot4(Vec4<float>::load(iv + k), Vec4<float>::load(txt + (int64_t)j * d + k));
    acc = wave_sum(acc);
    if (lane == 0) c[j] = acc;
  }
  __syncthreads();
  float se = 0.f;
  for (int j = t; j < N; j += POOL_THREADS) se += expf(c[j]);
  se = block_sum(se, red);
  const float den = se + 1e-4f;
  if (t == 0) row_loss[i] = logf(den) - (c[i] + 1e-4f);
  __syncthreads();
  const float inv_b = 1.0f / (float)B;
  for (int j = t; j < N; j += POOL_THREADS) {
    const float g = (expf(c[j]) / den - (j == i ? 1.f : 0.f)) * inv_b;
    c[j] = g;
    dc[(int64_t)i * N + j] = g;
  }
  __syncthreads();
  if (t < ncol4) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < N; ++j) acc += Vec4<float>::load(txt + (int64_t)j * d + t * 4) * c[j];
    Vec4<float>::store(d_img + (int64_t)i * d + t * 4, acc);
  }
}

// Workgroup j: d_txt_j = sum_i dC_ij img_i (in order); workgroup 0 also adds the row losses: loss = sum_i row_loss_i / B (:263)
__global__ __launch_bounds__(POOL_THREADS) void contrastive_cols_kernel(const float* __restrict__ img, const float* __restrict__ dc,
                                                                        const float* __restrict__ row_loss, float* __restrict__ d_txt,
                                                                        float* __restrict__ loss, int B, int N, int d) {
  const int j = blockIdx.x, t = threadIdx.x;
  if (t < (d >> 2)) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < B; ++i) acc += Vec4<float>::load(img + (int64_t)i * d + t * 4) * dc[(int64_t)i * N + j];
    Vec4<float>::store(d_txt + (int64_t)j * d + t * 4, acc);
  }
  if (j == 0 && t == 0) {
    float s = 0.f;
    for (int i = 0; i < B; ++i) s += row_loss[i];
    loss[0] = s / (float)B;
  }
}

// ------------------------------------------------------------------------------------------- two-sided contrastive loss (SenSim)
// src/sen_sim.py:94-103.  scat = [source negatives; sources], tcat = [target negatives; targets]; pair i is src_i = scat[Ns - B + i],
// tgt_i = tcat[Nt - B + i].  Workgroup i: A_ij = src_i . tcat_j, M_ij = tgt_i . scat_j, D_i = sum_j exp A_ij + sum_j exp M_ij + 1e-4,
// row loss log D_i - (src_i . tgt_i + 1e-4) (the dot product is A's column Nt - B + i), dA_ij = exp A_ij / (D_i B),
// dM_ij = exp M_ij / (D_i B), and the part of the pair's own gradients that is a sum over its row:
// row_s_i = sum_j dA_ij tcat_j - tgt_i / B (into d src_i), row_t_i = sum_j dM_ij scat_j - src_i / B (into d tgt_i).
// d src_i holds tgt_i three times -- dA_i,own from this row sum, dM_i,own from the column sum, and - 1 / B -- and the three nearly
// cancel when the pair dominates its denominator (few negatives).  They are added as one coefficient, formed without the
// cancellation: with R_i = D_i - exp A_i,own - exp M_i,own (summed on its own, the pair's two terms left out),
// dA_i,own + dM_i,own - 1 / B = -R_i / (D_i B).  The row sums here and the column sums below leave the pair's own term out.
__global__ __launch_bounds__(POOL_THREADS) void sensim_rows_kernel(const float* __restrict__ scat, const float* __restrict__ tcat,
                                                                   float* __restrict__ row_loss, float* __restrict__ da, float* __restrict__ dm,
                                                                   float* __restrict__ row_s, float* __restrict__ row_t, int B, int Ns, int Nt,
                                                                   int d) {
  __shared__ float red[16];
  __shared__ float a[IMT_CONTRASTIVE_MAX_N];
  __shared__ float m[IMT_CONTRASTIVE_MAX_N];
  __shared__ __attribute__((aligned(16))) float sv[IMT_POOL_MAX_D];
  __shared__ __attribute__((aligned(16))) float tv[IMT_POOL_MAX_D];
  const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ncol4 = d >> 2;
  const float* src = scat + (int64_t)(Ns - B + i) * d;
  const float* tgt = tcat + (int64_t)(Nt - B + i) * d;
  if (t < ncol4) {
    Vec4<float>::store(sv + t * 4, Vec4<float>::load(src + t * 4));
    Vec4<float>::store(tv + t * 4, Vec4<float>::load(tgt + t * 4));
  }
  __syncthreads();
  for (int j = wave; j < Nt; j += POOL_THREADS / 64) {
    float acc = 0.f;
    for (int k = lane * 4; k < d; k += 256) acc += dot4(Vec4<float>::load(sv + k), Vec4<float>::load(tcat + (int64_t)j * d + k));
    acc = wave_sum(acc);
    if (lane == 0) a[j] = acc;
  }
  for (int j = wave; j < Ns; j += POOL_THREADS / 64) {
    float acc = 0.f;
    for (int k = lane * 4; k < d; k += 256) acc += dot4(Vec4<float>::load(tv + k), Vec4<float>::load(scat + (int64_t)j * d + k));
    acc = wave_sum(acc);
    if (lane == 0) m[j] = acc;
  }
  __syncthreads();
  const int own_a = Nt - B + i, own_m = Ns - B + i;
  float sa = 0.f, sm = 0.f;
  for (int j = t; j < Nt; j += POOL_THREADS) sa += j == own_a ? 0.f : expf(a[j]);
  for (int j = t; j < Ns; j += POOL_THREADS) sm += j == own_m ? 0.f : expf(m[j]);
  sa = block_sum(sa, red);
  sm = block_sum(sm, red);
  const float rest = (sa + sm) + 1e-4f;
  const float den = rest + (expf(a[own_a]) + expf(m[own_m]));
  if (t == 0) row_loss[i] = logf(den) - (a[own_a] + 1e-4f);
  __syncthreads();
  const float inv_b = 1.0f / (float)B;
  const float own_coef = -(rest / den) * inv_b;
  for (int j = t; j < Nt; j += POOL_THREADS) {
    const float g = expf(a[j]) / den * inv_b;
    a[j] = g;
    da[(int64_t)i * Nt + j] = g;
  }
  for (int j = t; j < Ns; j += POOL_THREADS) {
    const float g = expf(m[j]) / den * inv_b;
    m[j] = g;
    dm[(int64_t)i * Ns + j] = g;
  }
  __syncthreads();
  if (t == 0) a[own_a] = m[own_m] = 0.f;  // the pair's own term is in own_coef
  __syncthreads();
  if (t < ncol4) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int j = 0; j < Nt; ++j) acc += Vec4<float>::load(tcat + (int64_t)j * d + t * 4) * a[j];
    Vec4<float>::store(row_s + (int64_t)i * d + t * 4, acc + Vec4<float>::load(tv + t * 4) * own_coef);
    f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int j = 0; j < Ns; ++j) acc2 += Vec4<float>::load(scat + (int64_t)j * d + t * 4) * m[j];
    Vec4<float>::store(row_t + (int64_t)i * d + t * 4, acc2 + Vec4<float>::load(sv + t * 4) * own_coef);
  }
}

// Workgroup c < Ns: d_scat_c = sum_i dM_ic tgt_i (in order); when c is one of the last B rows its own pair is left out of the sum
// and row_s of that pair (which holds the pair's own term) is added.  Workgroup Ns + c: d_tcat_c = sum_i dA_ic src_i, plus row_t,
// likewise.  Every output row has this one writer.  Workgroup 0 also adds the row losses.
__global__ __launch_bounds__(POOL_THREADS) void sensim_cols_kernel(const float* __restrict__ scat, const float* __restrict__ tcat,
                                                                   const float* __restrict__ da, const float* __restrict__ dm,
                                                                   const float* __restrict__ row_s, const float* __restrict__ row_t,
                                                                   const float* __restrict__ row_loss, float* __restrict__ d_scat,
                                                                   float* __restrict__ d_tcat, float* __restrict__ loss, int B, int Ns, int Nt,
                                                                   int d) {
  const int t = threadIdx.x;
  const bool src_side = (int)blockIdx.x < Ns;
  const int c = src_side ? (int)blockIdx.x : (int)blockIdx.x - Ns;
  const int n = src_side ? Ns : Nt;
  const float* dc = src_side ? dm : da;                                            // [B, n]
  const float* other = src_side ? tcat + (int64_t)(Nt - B) * d : scat + (int64_t)(Ns - B) * d;  // the B vectors of the other side
  const float* row = src_side ? row_s : row_t;
  float* out = src_side ? d_scat : d_tcat;
  const int own = c - (n - B);  // the pair this row belongs to; negative for a negative sample
  if (t < (d >> 2)) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int i = 0; i < B; ++i) acc += Vec4<float>::load(other + (int64_t)i * d + t * 4) * (i == own ? 0.f : dc[(int64_t)i * n + c]);
    if (own >= 0) acc += Vec4<float>::load(row + (int64_t)own * d + t * 4);
    Vec4<float>::store(out + (int64_t)c * d + t * 4, acc);
  }
  if (blockIdx.x == 0 && t == 0) {
    float s = 0.f;
    for (int i = 0; i < B; ++i) s += row_loss[i];
    loss[0] = s / (float)B;
  }
}

// ------------------------------------------------------------------------------------------- pair dot products (SenSim similarity)
// out_r = a_r . b_r (src/sen_sim.py:112), one wave per row: lane sums of 4-element groups, then the wave butterfly.
__global__ __launch_bounds__(POOL_THREADS) void pair_dot_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                                                                int64_t rows, int d) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (POOL_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;  // whole waves leave: no barrier follows
  float acc = 0.f;
  for (int k = lane * 4; k < d; k += 256) acc += dot4(Vec4<float>::load(a + r * d + k), Vec4<float>::load(b + r * d + k));
  acc = wave_sum(acc);
  if (lane == 0) out[r] = acc;
}

// da_r = g_r b_r, db_r = g_r a_r; one thread per 4-element group, grid-stride
__global__ __launch_bounds__(256) void pair_dot_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ g,
                                                           float* __restrict__ da, float* __restrict__ db, int64_t n4, int ncol4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float gr = g[i / ncol4];
    const f32x4 av = Vec4<float>::load(a + i * 4), bv = Vec4<float>::load(b + i * 4);
    Vec4<float>::store(da + i * 4, bv * gr);
    Vec4<float>::store(db + i * 4, av * gr);
  }
}

int pair_dot_validate(const char* what, int64_t rows, int d) {
  IMT_CHECK_ARG(rows >= 0 && rows <= 0x7fffffff, "%s: row count outside [0, 2^31)", what);
  IMT_CHECK_ARG(d >= 4 && d % 4 == 0, "%s: d must be a positive multiple of 4", what);
  IMT_CHECK_ARG(d <= IMT_POOL_MAX_D, "%s: d above %d is not taken", what, IMT_POOL_MAX_D);
  return IMT_OK;
}

// Everything the four pooling entry points share and that can be settled without touching the device: the shape is refused or
// taken (in the order dtype, rows, S, d, dropout_p), then the LDS plan, the dropout constants and the profiler's bytes of x.
struct PoolPlan { int keep; size_t lds; uint32_t thresh; float inv_keep; double x_bytes; };
int pool_validate(const char* what, int dtype, int64_t rows, int S, int d, float dropout_p, PoolPlan* p) {
  IMT_CHECK_ARG(imt_ok_dtype(dtype), "%s: bad dtype", what);
  IMT_CHECK_ARG(rows >= 0 && rows <= 0x7fffffff, "%s: row count outside [0, 2^31)", what);
  IMT_CHECK_ARG(S >= 1, "%s: S must be at least 1", what);
  IMT_CHECK_ARG(S <= IMT_POOL_MAX_S, "%s: S above %d is not taken", what, IMT_POOL_MAX_S);
  IMT_CHECK_ARG(d >= 4 && d % 4 == 0, "%s: d must be a positive multiple of 4", what);
  IMT_CHECK_ARG(d <= IMT_POOL_MAX_D, "%s: d above %d is not taken", what, IMT_POOL_MAX_D);
  IMT_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "%s: dropout_p outside [0, 1)", what);
  p->keep = pool_small_bytes(S, d) + pool_x_bytes(dtype, S, d) <= IMT_POOL_LDS_BYTES;
  p->lds = (size_t)(pool_small_bytes(S, d) + (p->keep ? pool_x_bytes(dtype, S, d) : 0));
  p->thresh = dropout_thresh(dropout_p);
  p->inv_keep = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  p->x_bytes = (double)rows * pool_x_bytes(dtype, S, d);
  return IMT_OK;
}

template <int KIND>
int pool_fwd(const char* what, int dtype, const void* x, const void* w, const void* b, const uint8_t* mask, void* out, float* probs,
             float* norm, int64_t rows, int S, int d, float dropout_p, uint64_t dropout_seed, void* stream) {
  PoolPlan p;
  const int rc = pool_validate(what, dtype, rows, S, d, dropout_p, &p);
  if (rc != IMT_OK) return rc;
  if (rows == 0) return IMT_OK;
  IMT_CHECK_ARG(x && w && b && out && probs && (norm || KIND != POOL_UNIT), "%s: null pointer", what);
  hipStream_t st = (hipStream_t)stream;
  ImtProfScope prof(what, 2.0 * rows * S * d * 2, (p.keep ? 1.0 : 2.0) * p.x_bytes, st);
  return imt_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((pool_fwd_kernel<T, KIND>), dim3((unsigned)rows), dim3(POOL_THREADS), p.lds, st, (const T*)x, (const T*)w, (const T*)b,
                       mask, (pool_out_t<T, KIND>*)out, probs, norm, S, d, p.keep, p.thresh, p.inv_keep, dropout_seed);
    IMT_CHECK_LAUNCH();
    return IMT_OK;
  });
}

// dout: du (fp32) | dv (compute dtype); u, norm, du_scale: unit vectors only.  ws: dw_part [rows, d] | db_part [rows]
template <int KIND>
int pool_bwd(const char* what, int dtype, const void* x, const void* w, const uint8_t* mask, const float* probs, const void* dout,
             const float* u, const float* norm, const float* du_scale, void* dx, float* dw, float* db, float* ws, int64_t rows, int S,
             int d, float dropout_p, uint64_t dropout_seed, void* stream) {
  PoolPlan p;
  const int rc = pool_validate(what, dtype, rows, S, d, dropout_p, &p);
  if (rc != IMT_OK) return rc;
  if (rows == 0) return IMT_OK;
  IMT_CHECK_ARG(x && w && probs && dout && dx && dw && db && ws && ((u && norm) || KIND != POOL_UNIT), "%s: null pointer", what);
  hipStream_t st = (hipStream_t)stream;
  float* dw_part = ws;
  float* db_part = ws + rows * d;
  ImtProfScope prof(what, 2.0 * rows * S * d * 3, (p.keep ? 2.0 : 3.0) * p.x_bytes, st);
  const int rc2 = imt_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((pool_bwd_kernel<T, KIND>), dim3((unsigned)rows), dim3(POOL_THREADS), p.lds, st, (const T*)x, (const T*)w, mask, probs,
                       (const pool_out_t<T, KIND>*)dout, u, norm, du_scale, (T*)dx, dw_part, db_part, S, d, p.keep, p.thresh, p.inv_keep,
                       dropout_seed);
    IMT_CHECK_LAUNCH();
    return IMT_OK;
  });
  if (rc2 != IMT_OK) return rc2;
  hipLaunchKernelGGL(attn_pool_fold_kernel, dim3(imt_cdiv(d + 1, 256)), dim3(256), 0, st, dw_part, db_part, dw, db, rows, d);
  IMT_CHECK_LAUNCH();
  return IMT_OK;
}

}  // namespace

extern "C" int imt_attn_pool_plan(int dtype, int S, int d) {
  PoolPlan p;
  const int rc = pool_validate("attn_pool_plan", dtype, 0, S, d, 0.f, &p);
  if (rc != IMT_OK) return rc;
  return p.keep ? 1 : 2;
}

extern "C" int imt_attn_pool_fwd(int dtype, const void* x, const void* w, const void* b, const uint8_t* mask, float* u, float* probs,
                                 float* norm, int64_t rows, int S, int d, void* stream) {
  return pool_fwd<POOL_UNIT>("attn_pool_fwd", dtype, x, w, b, mask, u, probs, norm, rows, S, d, 0.f, 0, stream);
}

extern "C" int imt_attn_pool_bwd(int dtype, const void* x, const void* w, const uint8_t* mask, const float* u, const float* probs,
                                 const float* norm, const float* du, const float* du_scale, void* dx, float* dw, float* db, float* ws,
                                 int64_t rows, int S, int d, void* stream) {
  return pool_bwd<POOL_UNIT>("attn_pool_bwd", dtype, x, w, mask, probs, du, u, norm, du_scale, dx, dw, db, ws, rows, S, d, 0.f, 0, stream);
}

extern "C" int imt_sent_pool_fwd(int dtype, const void* x, const void* w, const void* b, const uint8_t* mask, void* v, float* probs,
                                 int64_t rows, int S, int d, float dropout_p, uint64_t dropout_seed, void* stream) {
  return pool_fwd<POOL_SENT>("sent_pool_fwd", dtype, x, w, b, mask, v, probs, nullptr, rows, S, d, dropout_p, dropout_seed, stream);
}

extern "C" int imt_sent_pool_bwd(int dtype, const void* x, const void* w, const uint8_t* mask, const float* probs, const void* dv, void* dx,
                                 float* dw, float* db, float* ws, int64_t rows, int S, int d, float dropout_p, uint64_t dropout_seed,
                                 void* stream) {
  return pool_bwd<POOL_SENT>("sent_pool_bwd", dtype, x, w, mask, probs, dv, nullptr, nullptr, nullptr, dx, dw, db, ws, rows, S, d, dropout_p,
                             dropout_seed, stream);
}

extern "C" int imt_contrastive(const float* img, const float* txt, float* loss, float* d_img, float* d_txt, float* ws, int B, int N,
                               int d, void* stream) {
  IMT_CHECK_ARG(B >= 1, "contrastive: B must be at least 1");
  IMT_CHECK_ARG(N >= B, "contrastive: fewer text vectors than images (the first B belong to the images)");
  IMT_CHECK_ARG(N <= IMT_CONTRASTIVE_MAX_N, "contrastive: more than %d text vectors are not taken", IMT_CONTRASTIVE_MAX_N);
  IMT_CHECK_ARG(d >= 4 && d % 4 == 0, "contrastive: d must be a positive multiple of 4");
  IMT_CHECK_ARG(d <= IMT_POOL_MAX_D, "contrastive: d above %d is not taken", IMT_POOL_MAX_D);
  IMT_CHECK_ARG(img && txt && loss && d_img && d_txt && ws, "contrastive: null pointer");
  hipStream_t st = (hipStream_t)stream;
  float* dc = ws;                       // [B, N]
  float* row_loss = ws + (int64_t)B * N;  // [B]
  ImtProfScope prof("contrastive", 6.0 * B * N * d, 4.0 * ((double)B * d + (double)N * d) * 3, st);
  hipLaunchKernelGGL(contrastive_rows_kernel, dim3(B), dim3(POOL_THREADS), 0, st, img, txt, row_loss, dc, d_img, B, N, d);
  IMT_CHECK_LAUNCH();
  hipLaunchKernelGGL(contrastive_cols_kernel, dim3(N), dim3(POOL_THREADS), 0, st, img, dc, row_loss, d_txt, loss, B, N, d);
  IMT_CHECK_LAUNCH();
  return IMT_OK;
}

extern "C" int imt_sensim_loss(const float* scat, const float* tcat, float* loss, float* d_scat, float* d_tcat, float* ws, int B, int Ns,
                               int Nt, int d, void* stream) {
  IMT_CHECK_ARG(B >= 1, "sensim_loss: B must be at least 1");
  IMT_CHECK_ARG(Ns >= B && Nt >= B, "sensim_loss: fewer vectors on a side than pairs (the last B of each side are the pairs)");
  IMT_CHECK_ARG(Ns <= IMT_CONTRASTIVE_MAX_N && Nt <= IMT_CONTRASTIVE_MAX_N, "sensim_loss: more than %d vectors on a side are not taken",
                IMT_CONTRASTIVE_MAX_N);
  IMT_CHECK_ARG(d >= 4 && d % 4 == 0, "sensim_loss: d must be a positive multiple of 4");
  IMT_CHECK_ARG(d <= IMT_POOL_MAX_D, "sensim_loss: d above %d is not taken", IMT_POOL_MAX_D);
  IMT_CHECK_ARG(scat && tcat && loss && d_scat && d_tcat && ws, "sensim_loss: null pointer");
  hipStream_t st = (hipStream_t)stream;
  float* da = ws;                          // [B, Nt]
  float* dm = da + (int64_t)B * Nt;        // [B, Ns]
  float* row_s = dm + (int64_t)B * Ns;     // [B, d]
  float* row_t = row_s + (int64_t)B * d;   // [B, d]
  float* row_loss = row_t + (int64_t)B * d;  // [B]
  ImtProfScope prof("sensim_loss", 6.0 * B * ((double)Ns + Nt) * d, 4.0 * ((double)Ns + Nt) * d * 3, st);
  hipLaunchKernelGGL(sensim_rows_kernel, dim3(B), dim3(POOL_THREADS), 0, st, scat, tcat, row_loss, da, dm, row_s, row_t, B, Ns, Nt, d);
  IMT_CHECK_LAUNCH();
  hipLaunchKernelGGL(sensim_cols_kernel, dim3(Ns + Nt), dim3(POOL_THREADS), 0, st, scat, tcat, da, dm, row_s, row_t, row_loss, d_scat,
                     d_tcat, loss, B, Ns, Nt, d);
  IMT_CHECK_LAUNCH();
  return IMT_OK;
}

extern "C" int imt_pair_dot(const float* a, const float* b, float* out, int64_t rows, int d, void* stream) {
  const int rc = pair_dot_validate("pair_dot", rows, d);
  if (rc != IMT_OK) return rc;
  if (rows == 0) return IMT_OK;
  IMT_CHECK_ARG(a && b && out, "pair_dot: null pointer");
  hipStream_t st = (hipStream_t)stream;
  ImtProfScope prof("pair_dot", 2.0 * rows * d, 8.0 * rows * d, st);
  hipLaunchKernelGGL(pair_dot_kernel, dim3((unsigned)imt_cdiv(rows, POOL_THREADS / 64)), dim3(POOL_THREADS), 0, st, a, b, out, rows, d);
  IMT_CHECK_LAUNCH();
  return IMT_OK;
}

extern "C" int imt_pair_dot_bwd(const float* a, const float* b, const float* g, float* da, float* db, int64_t rows, int d, void* stream) {
  const int rc = pair_dot_validate("pair_dot_bwd", rows, d);
  if (rc != IMT_OK) return rc;
  if (rows == 0) return IMT_OK;
  IMT_CHECK_ARG(a && b && g && da && db, "pair_dot_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t n4 = rows * (d >> 2);
  const int64_t wgs = (n4 + 255) / 256;
  ImtProfScope prof("pair_dot_bwd", 2.0 * rows * d, 16.0 * rows * d, st);
  hipLaunchKernelGGL(pair_dot_bwd_kernel, dim3((unsigned)(wgs < 2048 ? wgs : 2048)), dim3(256), 0, st, a, b, g, da, db, n4, d >> 2);
  IMT_CHECK_LAUNCH();
  return IMT_OK;
}

extern "C" int imt_l2_dist(int dtype, const void* pred, const void* target, float* loss, void* dpred, float* ws, int B, int64_t n,
                           void* stream) {
  IMT_CHECK_ARG(imt_ok_dtype(dtype), "l2_dist: bad dtype");
  IMT_CHECK_ARG(B >= 1, "l2_dist: B must be at least 1");
  IMT_CHECK_ARG(n >= 4 && n % 4 == 0, "l2_dist: n must be a positive multiple of 4");
  IMT_CHECK_ARG(n <= ((int64_t)1 << 40) / B, "l2_dist: more than 2^40 elements are not taken");
  IMT_CHECK_ARG(pred && target && loss && dpred && ws, "l2_dist: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t n4 = (int64_t)B * n / 4;
  const int64_t wgs = (n4 + 255) / 256;
  const int nparts = (int)(wgs < IMT_L2_DIST_PARTS ? wgs : IMT_L2_DIST_PARTS);
  const int grid2 = (int)(wgs < 2048 ? wgs : 2048);
  const float inv_b = 1.0f / (float)B;
  ImtProfScope prof("l2_dist", 3.0 * B * n, (double)B * n * imt_dtype_bytes(dtype) * 5, st);
  return imt_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(l2_partial_kernel<T>, dim3(nparts), dim3(256), 0, st, (const T*)pred, (const T*)target, ws, n4);
    IMT_CHECK_LAUNCH();
    hipLaunchKernelGGL(l2_scale_kernel<T>, dim3(grid2), dim3(256), 0, st, (const T*)pred, (const T*)target, ws, nparts, loss, (T*)dpred, n4,
                       inv_b);
    IMT_CHECK_LAUNCH();
    return IMT_OK;
  });
}
