// Object stream of ImageCaptioning from pre-extracted detector features (src/image_model.py:44-82, :357-366):
// operand staging of the object head (object rows, K-padded copy of object_feat_fc.weight), ReLU + dropout and its
// backward, the weight / embedding gradient folds, and the backward of the sigmoid-gated mix of the two decoder streams.
// The product itself is imt_gemm on the padded operands.  Every reduction here runs in a fixed order: two identical
// calls give bit-identical gradients.
#include "common.hpp"

namespace {

constexpr int ROWS_PER_BLOCK = 4;  // one 64-lane wave per row, 4 consecutive columns per lane

// ------------------------------------------------------------------------------------------- forward staging
// Row r of X: [object_embedding[label] (d) | feature (1024) | locs (7) | zeros up to Kp]; a label-0 row is zero whole
// (src/image_model.py:74-76), an out-of-range label too (and flags *status).  locs = x1/800, x2/800, y1/800, y2/800, w, h,
// w*h with w = x2/800 - x1/800, h = y2/800 - y1/800 (:61-69); boxes are (x1, y1, x2, y2).
// Blocks past the object rows write the K-padded copy of object_feat_fc.weight ([d, K] -> [d, Kp], zero pad columns).
template <typename TF, typename T>
__global__ __launch_bounds__(256) void obj_rows_kernel(const int64_t* __restrict__ labels, const TF* __restrict__ feats,
                                                       const float* __restrict__ boxes, const T* __restrict__ emb,
                                                       const T* __restrict__ w, T* __restrict__ x_out, T* __restrict__ w_out,
                                                       int64_t R, int d, int Kp, int row_blocks, int* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int K = d + IMT_OBJ_FEAT_DIM + 7;
  if ((int)blockIdx.x >= row_blocks) {  // weight copy: one wave per output row of W
    const int64_t n = (int64_t)(blockIdx.x - row_blocks) * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (n >= d) return;
    const T* wr = w + n * K;  // K is odd: rows of the flat slice are not vector aligned -> element loads
    T* orow = w_out + n * Kp;
    for (int c = lane * 4; c < Kp; c += 256) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (c + e < K) ? to_f32<T>(wr[c + e]) : 0.f;
      Vec4<T>::store(orow + c, v);
    }
    return;
  }
  const int64_t r = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (r >= R) return;
  const int64_t lab = labels[r];
  const bool bad = lab < 0 || lab >= IMT_OBJ_LABELS;
  if (bad && lane == 0 && status) atomicOr(status, 1);
  const bool zero = bad || lab == 0;
  T* orow = x_out + r * Kp;
  float loc[8];
  {
    const float x1 = boxes[r * 4 + 0] / 800.f, y1 = boxes[r * 4 + 1] / 800.f;
    const float x2 = boxes[r * 4 + 2] / 800.f, y2 = boxes[r * 4 + 3] / 800.f;
    const float wd = x2 - x1, ht = y2 - y1;
    loc[0] = x1; loc[1] = x2; loc[2] = y1; loc[3] = y2; loc[4] = wd; loc[5] = ht; loc[6] = ht * wd; loc[7] = 0.f;
  }
  const T* er = emb + (zero ? 0 : lab) * d;
  const TF* fr = feats + r * IMT_OBJ_FEAT_DIM;
  for (int c = lane * 4; c < Kp; c += 256) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!zero) {
      if (c < d) v = Vec4<T>::load(er + c);                                            // d % 4 == 0: no straddle
      else if (c < d + IMT_OBJ_FEAT_DIM) v = Vec4<TF>::load(fr + (c - d));
      else if (c < d + IMT_OBJ_FEAT_DIM + 8) {
        const int j = c - d - IMT_OBJ_FEAT_DIM;                                         // 0 or 4
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = j == 0 ? loc[e] : loc[4 + e];
      }
    }
    Vec4<T>::store(orow + c, v);
  }
}

// y <- dropout(relu(y)) in place; element index r * d + c as at the other dropout sites (keep(seed, m * N + n))
template <typename T>
__global__ __launch_bounds__(256) void relu_dropout_kernel(T* __restrict__ y, int64_t rows, int d, uint32_t thresh,
                                                           float inv_keep, uint64_t seed) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (r >= rows) return;
  for (int c = lane * 4; c < d; c += 256) {
    f32x4 v = Vec4<T>::load(y + r * d + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
    if (thresh) dropout_apply4(v, seed, (uint64_t)r * d + c, thresh, inv_keep);
    Vec4<T>::store(y + r * d + c, v);
  }
}

// dz = dy * relu'(z) * keep / (1 - p): the mask is regenerated from the seed, relu'(z) read off the saved output (y > 0 exactly
// where z > 0 for a kept element; a dropped element has keep = 0 whatever y holds)
template <typename T>
__global__ __launch_bounds__(256) void relu_dropout_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y, T* __restrict__ dz,
                                                               int64_t rows, int d, uint32_t thresh, float inv_keep, uint64_t seed) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (r >= rows) return;
  for (int c = lane * 4; c < d; c += 256) {
    f32x4 g = Vec4<T>::load(dy + r * d + c);
    const f32x4 v = Vec4<T>::load(y + r * d + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = v[e] > 0.f ? g[e] : 0.f;
    if (thresh) dropout_apply4(g, seed, (uint64_t)r * d + c, thresh, inv_keep);
    Vec4<T>::store(dz + r * d + c, g);
  }
}

// grad[n, k] += dw_pad[n, k] for k < K (the first K columns of the fp32 [d, Kp] product)
__global__ __launch_bounds__(256) void obj_fold_w_kernel(const float* __restrict__ dw_pad, float* __restrict__ grad, int d, int K,
                                                        int Kp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)d * K) return;
  const int64_t n = i / K, k = i - n * K;
  grad[i] += dw_pad[n * Kp + k];
}

// grad[l, :] += sum over rows r with labels[r] == l (in row order) of dx[r, :], l = 1 .. IMT_OBJ_LABELS - 1.  One workgroup per
// label owns its gradient row: no atomics, a fixed summation order.  Rows are scanned in chunks of 256: one label load per
// thread, a ballot per wave, then every thread walks the (few) matching rows of the chunk in order.
template <typename T>
__global__ __launch_bounds__(256) void obj_embed_grad_kernel(const int64_t* __restrict__ labels, const T* __restrict__ dx, int64_t ldx,
                                                             float* __restrict__ grad, int64_t R, int d) {
  __shared__ unsigned long long match[4];
  const int l = blockIdx.x + 1;
  const int t = threadIdx.x, wave = t >> 6;
  constexpr int MAXC = 4;  // d <= 4096
  f32x4 acc[MAXC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t base = 0; base < R; base += 256) {
    const int64_t r = base + t;
    const bool m = r < R && labels[r] == (int64_t)l;
    const unsigned long long bal = __ballot(m);
    if ((t & 63) == 0) match[wave] = bal;
    __syncthreads();
    for (int w = 0; w < 4; ++w) {
      unsigned long long bits = match[w];
      while (bits) {
        const int b = __builtin_ctzll(bits);
        bits &= bits - 1;
        const T* row = dx + (base + w * 64 + b) * ldx;
#pragma unroll
        for (int i = 0; i < MAXC; ++i) {
          const int c = t * 4 + i * 1024;
          if (c < d) acc[i] += Vec4<T>::load(row + c);
        }
      }
    }
    __syncthreads();
  }
  float* g = grad + (int64_t)l * d;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = t * 4 + i * 1024;
    if (c < d) {
      f32x4 v = Vec4<float>::load(g + c);
      v += acc[i];
      Vec4<float>::store(g + c, v);
    }
  }
}

// gated mix backward, stage 1: part p of IMT_GATED_MIX_BWD_PARTS owns a contiguous range of rows; da, db per element and the
// part's column sums of dy * (a - b) * s * (1 - s) in row order -> partial[p, :]
template <typename T>
__global__ __launch_bounds__(256) void gated_mix_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ a, const T* __restrict__ b,
                                                            const T* __restrict__ gate, T* __restrict__ da, T* __restrict__ db,
                                                            float* __restrict__ partial, int64_t rows, int d, int64_t rows_per_part) {
  const int p = blockIdx.x;
  const int64_t r0 = (int64_t)p * rows_per_part;
  const int64_t r1 = min(rows, r0 + rows_per_part);
  for (int c = threadIdx.x * 4; c < d; c += 1024) {
    const f32x4 gv = Vec4<T>::load(gate + c);
    f32x4 s, ds;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s[e] = 1.0f / (1.0f + __expf(-(gv[e] + 1e-7f)));
      ds[e] = s[e] * (1.0f - s[e]);
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int64_t r = r0; r < r1; ++r) {
      const f32x4 g = Vec4<T>::load(dy + r * d + c), av = Vec4<T>::load(a + r * d + c), bv = Vec4<T>::load(b + r * d + c);
      f32x4 oa, ob;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        oa[e] = s[e] * g[e];
        ob[e] = (1.0f - s[e]) * g[e];
        acc[e] += g[e] * (av[e] - bv[e]) * ds[e];
      }
      Vec4<T>::store(da + r * d + c, oa);
      Vec4<T>::store(db + r * d + c, ob);
    }
    Vec4<float>::store(partial + (int64_t)p * d + c, acc);
  }
}

// stage 2: dgate[c] += sum over the parts in order
__global__ __launch_bounds__(256) void gated_mix_bwd_fold_kernel(const float* __restrict__ partial, float* __restrict__ dgate, int d) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d) return;
  float s = 0.f;
  for (int p = 0; p < IMT_GATED_MIX_BWD_PARTS; ++p) s += partial[(int64_t)p * d + c];
  dgate[c] += s;
}

}  // namespace

extern "C" int imt_obj_rows(int feat_dtype, int dtype, const int64_t* labels, const void* feats, const float* boxes,
                            const void* emb, const void* w, void* x_out, void* w_out, int64_t R, int d, int Kp, int* status,
                            void* stream) {
  IMT_CHECK_ARG(imt_ok_dtype(feat_dtype) && imt_ok_dtype(dtype), "obj_rows: bad dtype");
  IMT_CHECK_ARG(d > 0 && d % 4 == 0 && d <= 4096, "obj_rows: d must be a positive multiple of 4 (at most 4096)");
  IMT_CHECK_ARG(Kp >= d + IMT_OBJ_FEAT_DIM + 7 && Kp % 8 == 0, "obj_rows: Kp must be >= d + 1031 and a multiple of 8");
  IMT_CHECK_ARG(R >= 0, "obj_rows: negative row count");
  IMT_CHECK_ARG(!w_out || w, "obj_rows: w_out without w");
  IMT_CHECK_ARG(R == 0 || (labels && feats && boxes && emb && x_out), "obj_rows: null pointer");
  if (R == 0 && !w_out) return IMT_OK;
  hipStream_t st = (hipStream_t)stream;
  const int row_blocks = imt_cdiv(R, ROWS_PER_BLOCK);
  const int w_blocks = w_out ? imt_cdiv(d, ROWS_PER_BLOCK) : 0;
  const int T_bytes = imt_dtype_bytes(dtype);
  ImtProfScope prof("obj_rows", 0.0, (double)R * Kp * T_bytes + (double)R * IMT_OBJ_FEAT_DIM * imt_dtype_bytes(feat_dtype) +
                                      (w_out ? 2.0 * d * Kp * T_bytes : 0.0), st);
  const dim3 grid(row_blocks + w_blocks);
  return imt_by_dtype(feat_dtype, [&](auto feat_tag) {
    return imt_by_dtype(dtype, [&](auto tag) {
      using TF = typename decltype(feat_tag)::type;
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL((obj_rows_kernel<TF, T>), grid, dim3(256), 0, st, labels, (const TF*)feats, boxes, (const T*)emb, (const T*)w,
                         (T*)x_out, (T*)w_out, R, d, Kp, row_blocks, status);
      IMT_CHECK_LAUNCH();
      return IMT_OK;
    });
  });
}

extern "C" int imt_relu_dropout(int dtype, void* y, int64_t rows, int d, float dropout_p, uint64_t dropout_seed, void* stream) {
  IMT_CHECK_ARG(imt_ok_dtype(dtype), "relu_dropout: bad dtype");
  IMT_CHECK_ARG(d > 0 && d % 4 == 0, "relu_dropout: d must be a multiple of 4");
  IMT_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "relu_dropout: dropout_p outside [0, 1)");
  if (rows <= 0) return IMT_OK;
  IMT_CHECK_ARG(y, "relu_dropout: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(imt_cdiv(rows, ROWS_PER_BLOCK));
  const uint32_t th = dropout_thresh(dropout_p);
  const float ik = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  ImtProfScope prof("relu_dropout", 0.0, 2.0 * rows * d * imt_dtype_bytes(dtype), st);
  return imt_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(relu_dropout_kernel<T>, grid, dim3(256), 0, st, (T*)y, rows, d, th, ik, dropout_seed);
    IMT_CHECK_LAUNCH();
    return IMT_OK;
  });
}

extern "C" int imt_relu_dropout_bwd(int dtype, const void* dy, const void* y, void* dz, int64_t rows, int d, float dropout_p,
                                    uint64_t dropout_seed, void* stream) {
  IMT_CHECK_ARG(imt_ok_dtype(dtype), "relu_dropout_bwd: bad dtype");
  IMT_CHECK_ARG(d > 0 && d % 4 == 0, "relu_dropout_bwd: d must be a multiple of 4");
  IMT_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "relu_dropout_bwd: dropout_p outside [0, 1)");
  if (rows <= 0) return IMT_OK;
  IMT_CHECK_ARG(dy && y && dz, "relu_dropout_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(imt_cdiv(rows, ROWS_PER_BLOCK));
  const uint32_t th = dropout_thresh(dropout_p);
  const float ik = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  ImtProfScope prof("relu_dropout_bwd", 0.0, 3.0 * rows * d * imt_dtype_bytes(dtype), st);
  return imt_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(relu_dropout_bwd_kernel<T>, grid, dim3(256), 0, st, (const T*)dy, (const T*)y, (T*)dz, rows, d, th, ik, dropout_seed);
    IMT_CHECK_LAUNCH();
    return IMT_OK;
  });
}

extern "C" int imt_obj_fold_w(const float* dw_pad, float* grad, int d, int Kp, void* stream) {
  IMT_CHECK_ARG(d > 0 && d % 4 == 0, "obj_fold_w: d must be a positive multiple of 4");
  IMT_CHECK_ARG(Kp >= d + IMT_OBJ_FEAT_DIM + 7, "obj_fold_w: Kp must be >= d + 1031");
  IMT_CHECK_ARG(dw_pad && grad, "obj_fold_w: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int K = d + IMT_OBJ_FEAT_DIM + 7;
  ImtProfScope prof("obj_fold_w", 0.0, 12.0 * d * K, st);
  hipLaunchKernelGGL(obj_fold_w_kernel, dim3(imt_cdiv((int64_t)d * K, 256)), dim3(256), 0, st, dw_pad, grad, d, K, Kp);
  IMT_CHECK_LAUNCH();
  return IMT_OK;
}

extern "C" int imt_obj_embed_grad(int dtype, const int64_t* labels, const void* dx, int64_t ldx, float* grad, int64_t R, int d,
                                  void* stream) {
  IMT_CHECK_ARG(imt_ok_dtype(dtype), "obj_embed_grad: bad dtype");
  IMT_CHECK_ARG(d > 0 && d % 4 == 0 && d <= 4096, "obj_embed_grad: d must be a positive multiple of 4 (at most 4096)");
  IMT_CHECK_ARG(ldx >= d && ldx % 4 == 0, "obj_embed_grad: ldx must be >= d and a multiple of 4");
  if (R <= 0) return IMT_OK;
  IMT_CHECK_ARG(labels && dx && grad, "obj_embed_grad: null pointer");
  hipStream_t st = (hipStream_t)stream;
  ImtProfScope prof("obj_embed_grad", 0.0, 8.0 * R * (IMT_OBJ_LABELS - 1) + (double)R * d * imt_dtype_bytes(dtype), st);
  const dim3 grid(IMT_OBJ_LABELS - 1);
  return imt_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(obj_embed_grad_kernel<T>, grid, dim3(256), 0, st, labels, (const T*)dx, ldx, grad, R, d);
    IMT_CHECK_LAUNCH();
    return IMT_OK;
  });
}

extern "C" int imt_gated_mix_bwd(int dtype, const void* dy, const void* a, const void* b, const void* gate, void* da, void* db,
                                 float* dgate, float* partial_ws, int64_t rows, int d, void* stream) {
  IMT_CHECK_ARG(imt_ok_dtype(dtype), "gated_mix_bwd: bad dtype");
  IMT_CHECK_ARG(d > 0 && d % 4 == 0, "gated_mix_bwd: d must be a multiple of 4");
  if (rows <= 0) return IMT_OK;
  IMT_CHECK_ARG(dy && a && b && gate && da && db && dgate && partial_ws, "gated_mix_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int64_t rpp = (rows + IMT_GATED_MIX_BWD_PARTS - 1) / IMT_GATED_MIX_BWD_PARTS;
  ImtProfScope prof("gated_mix_bwd", 0.0, 5.0 * rows * d * imt_dtype_bytes(dtype), st);
  // parts past the last row write zero partial sums (their row range is empty)
  const int rc = imt_by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(gated_mix_bwd_kernel<T>, dim3(IMT_GATED_MIX_BWD_PARTS), dim3(256), 0, st, (const T*)dy, (const T*)a, (const T*)b,
                       (const T*)gate, (T*)da, (T*)db, partial_ws, rows, d, rpp);
    IMT_CHECK_LAUNCH();
    return IMT_OK;
  });
  if (rc != IMT_OK) return rc;
  hipLaunchKernelGGL(gated_mix_bwd_fold_kernel, dim3(imt_cdiv(d, 256)), dim3(256), 0, st, partial_ws, dgate, d);
  IMT_CHECK_LAUNCH();
  return IMT_OK;
}
