// The frozen ResNet trunk's kernels (see include/imt_hip.h): imt_conv2d, an NHWC convolution as an implicit GEMM on MFMA with the
// folded BatchNorm / residual / ReLU epilogue; imt_maxpool2d_3x3s2, the stem's max pool; imt_image_nhwc, uint8 pixels to the
// normalised 8-channel network input.
//
// imt_conv2d.  GEMM view: M = B Ho Wo output pixels, N = Cout, K = KH KW Cin ordered (kh, kw, c).  Cin is a multiple of 8, so
// a 16-byte chunk of K (8 bf16 / 4 fp32) lies inside ONE tap of one output pixel: it is one aligned 16-byte load of x, or zeros
// when the tap falls in the padding -- the predicate is taken per (output row, tap), no address outside x is ever formed into
// a load.  The im2col matrix is never stored.
// One workgroup (4 waves, 2 x 2) owns a 128 x BN tile of y, BN = 128 or 64 (conv_wide_tiles picks; same bits either way: one
// writer per element, the whole K in ascending order).  K loop in steps of 128 bytes, register-staged over two swizzled LDS
// stages with one barrier per step (the loop of align.hip): thread t owns chunk t & 7 of rows (t >> 3) + 32 u of both tiles; its
// rows' (b, ho, wo) are fixed for the whole loop, a step costs it one division of the chunk's k by Cin and KW.  Wave (wm, wn)
// multiplies pixels 64 wm .. + 63 by channels (BN / 2) wn .. : acc[mt][nt] is D[channel 16 nt + 4 g + e][pixel 16 mt + r] of
// mma.hpp's lane (r, g), so a lane ends with 4 consecutive channels of one pixel -- one 8- or 16-byte NHWC store where Cout is
// a multiple of 4, scalar stores otherwise.
#include <math.h>
#include "mma.hpp"

namespace {

constexpr int CV_BM = 128;       // output pixels per tile
constexpr int CV_RB = 128;       // bytes of K per staged step (one swizzled LDS row)
constexpr int CV_THREADS = 256;
constexpr int CV_CUS = 256;      // wide tiles from one per CU on

struct ConvP {
  const void* x; const void* w; void* y;
  const float* scale; const float* shift; const void* residual;
  int H, W, Cin, Cout, KW, stride, pad_h, pad_w, Ho, Wo, relu;
  int M, K, tiles_n;
};

template <typename T, int BN>
__global__ __launch_bounds__(CV_THREADS) void conv2d_kernel(ConvP p) {
  constexpr int EPC = 16 / sizeof(T), KC = CV_RB / sizeof(T);
  constexpr int UA = CV_BM / 32, UB = BN / 32;  // 16-byte chunks per thread and step of the pixel / weight tile
  constexpr int NT = BN / 32;                   // 16-channel MFMA tiles per wave
  __shared__ __attribute__((aligned(16))) char sx[2][CV_BM * CV_RB];
  __shared__ __attribute__((aligned(16))) char sw[2][BN * CV_RB];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int wm = wave & 1, wn = wave >> 1;
  // channel tiles of one pixel tile are neighbours in launch order: the gathered pixels are read from L2 by all of them
  const int tile = imt_xcd_block(blockIdx.x, gridDim.x);
  const int m0 = (tile / p.tiles_n) * CV_BM, n0 = (tile % p.tiles_n) * BN;
  const T* X = reinterpret_cast<const T*>(p.x);
  const T* Wt = reinterpret_cast<const T*>(p.w);

  // this thread's part of a staged step: chunk sc of tile rows sr + 32 u
  const int sr = tid >> 3, sc = tid & 7;
  int hb[UA], wb[UA];      // first tap's input row / column of the output pixel (may be negative: padding)
  int64_t pix0[UA];        // b * H * W, or -1 for a row past M
#pragma unroll
  for (int u = 0; u < UA; ++u) {
    const int m = m0 + sr + 32 * u;
    const int wo = m % p.Wo, t = m / p.Wo, ho = t % p.Ho, b = t / p.Ho;
    hb[u] = ho * p.stride - p.pad_h;
    wb[u] = wo * p.stride - p.pad_w;
    pix0[u] = m < p.M ? (int64_t)b * p.H * p.W : -1;
  }

  u32x4 rx[UA], rw[UB];
  auto fetch = [&](int t) {
    const int kk = t * KC + sc * EPC;  // first k of this thread's chunk; the chunk is whole or absent (K % EPC == 0)
    const bool k_ok = kk < p.K;
    const int tap = kk / p.Cin, c = kk - tap * p.Cin, kh = tap / p.KW, kw = tap - kh * p.KW;
#pragma unroll
    for (int u = 0; u < UA; ++u) {
      const int h = hb[u] + kh, w = wb[u] + kw;
      rx[u] = u32x4{0u, 0u, 0u, 0u};
      if (k_ok && pix0[u] >= 0 && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W)
        rx[u] = *reinterpret_cast<const u32x4*>(X + (pix0[u] + (int64_t)h * p.W + w) * p.Cin + c);
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int n = n0 + sr + 32 * u;
      rw[u] = u32x4{0u, 0u, 0u, 0u};
      if (k_ok && n < p.Cout) rw[u] = *reinterpret_cast<const u32x4*>(Wt + (int64_t)n * p.K + kk);
    }
  };

  f32x4 acc[4][NT];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (p.K + KC - 1) / KC;
  fetch(0);
  for (int t = 0; t < nk; ++t) {
    char* ax = sx[t & 1];
    char* aw = sw[t & 1];
#pragma unroll
    for (int u = 0; u < UA; ++u) *reinterpret_cast<u32x4*>(ax + tile_off<CV_RB>(sr + 32 * u, sc)) = rx[u];
#pragma unroll
    for (int u = 0; u < UB; ++u) *reinterpret_cast<u32x4*>(aw + tile_off<CV_RB>(sr + 32 * u, sc)) = rw[u];
    // one barrier per step: stage t & 1 was last read in step t - 2, which every wave left before the barrier of t - 1
    __syncthreads();
    if (t + 1 < nk) fetch(t + 1);
#pragma unroll
    for (int ks = 0; ks < CV_RB / 64; ++ks) {
      typename Frag<T>::type xf[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) xf[mt] = lds_frag_kcontig<T, CV_RB>(ax, 64 * wm + 16 * mt, 4 * ks);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const typename Frag<T>::type wf = lds_frag_kcontig<T, CV_RB>(aw, (BN / 2) * wn + 16 * nt, 4 * ks);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) mma16(acc[mt][nt], wf, xf[mt]);
      }
    }
  }

  // epilogue on the fp32 accumulator: * scale + shift, + residual, ReLU, store
  T* Y = reinterpret_cast<T*>(p.y);
  const T* R = reinterpret_cast<const T*>(p.residual);
  const bool vec = (p.Cout & 3) == 0;  // then a lane's 4 channels are all inside Cout or all outside, and aligned
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = n0 + (BN / 2) * wn + 16 * nt + 4 * g;
    if (n >= p.Cout) continue;
    float sc4[4], sh4[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool ok = n + e < p.Cout;
      sc4[e] = (p.scale && ok) ? p.scale[n + e] : 1.f;
      sh4[e] = (p.shift && ok) ? p.shift[n + e] : 0.f;
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int m = m0 + 64 * wm + 16 * mt + r;
      if (m >= p.M) continue;
      const int64_t o = (int64_t)m * p.Cout + n;
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaf(acc[mt][nt][e], sc4[e], sh4[e]);
      if (vec) {
        if (R) v += Vec4<T>::load(R + o);
        if (p.relu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        Vec4<T>::store(Y + o, v);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (n + e >= p.Cout) continue;
          float s = v[e];
          if (R) s += to_f32<T>(R[o + e]);
          if (p.relu) s = fmaxf(s, 0.f);
          Y[o + e] = from_f32<T>(s);
        }
      }
    }
  }
}

// 128-channel tiles where they still give every CU a workgroup; 64-channel tiles otherwise (and always for Cout <= 64)
bool conv_wide_tiles(int64_t M, int Cout) {
  return Cout > 64 && (int64_t)imt_cdiv(M, CV_BM) * imt_cdiv(Cout, 128) >= CV_CUS;
}

// ---------------------------------------------------------------- max pool 3 x 3, stride 2, padding 1 (NHWC)
// One thread per (output pixel, 16-byte chunk of channels); a tap in the padding is skipped (-inf), never read.
template <typename T> IMT_DEVICE void max16(f32x4 (&m)[2], u32x4 v);
template <> IMT_DEVICE void max16<float>(f32x4 (&m)[2], u32x4 v) {
  const f32x4 f = __builtin_bit_cast(f32x4, v);
#pragma unroll
  for (int j = 0; j < 4; ++j) m[0][j] = fmaxf(m[0][j], f[j]);
}
template <> IMT_DEVICE void max16<bf16_t>(f32x4 (&m)[2], u32x4 v) {
  const bf16x8 h = __builtin_bit_cast(bf16x8, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) m[j >> 2][j & 3] = fmaxf(m[j >> 2][j & 3], (float)h[j]);
}
template <typename T> IMT_DEVICE u32x4 pack16(const f32x4 (&m)[2]);
template <> IMT_DEVICE u32x4 pack16<float>(const f32x4 (&m)[2]) { return __builtin_bit_cast(u32x4, m[0]); }
template <> IMT_DEVICE u32x4 pack16<bf16_t>(const f32x4 (&m)[2]) {
  bf16x8 h;
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = (bf16_t)m[j >> 2][j & 3];  // exact: every maximum is one of the bf16 inputs
  return __builtin_bit_cast(u32x4, h);
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool_kernel(const T* __restrict__ x, T* __restrict__ y, int H, int W, int C, int Ho, int Wo,
                                                      int64_t total) {
  constexpr int EPC = 16 / sizeof(T);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int cpr = C / EPC;
  const int ch = (int)(i % cpr);
  const int64_t pix = i / cpr;
  const int wo = (int)(pix % Wo);
  const int64_t t = pix / Wo;
  const int ho = (int)(t % Ho);
  const int64_t b = t / Ho;
  f32x4 m[2] = {f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY}, f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY}};
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int h = 2 * ho - 1 + kh;
    if ((unsigned)h >= (unsigned)H) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int w = 2 * wo - 1 + kw;
      if ((unsigned)w >= (unsigned)W) continue;
      max16<T>(m, *reinterpret_cast<const u32x4*>(x + ((b * H + h) * W + w) * C + ch * EPC));
    }
  }
  *reinterpret_cast<u32x4*>(y + pix * C + ch * EPC) = pack16<T>(m);
}

// ---------------------------------------------------------------- uint8 [B, H, W, 3] -> normalised [B, H, W, 8]
// One thread per pixel.  (v / 255 - mean) / std is evaluated in fp64 and rounded once to fp32 (then to bf16): v / 255 next to
// the mean cancels, and an fp32 evaluation would carry the quotient's rounding error into the difference.
struct ImageP { double mean[3], std[3]; };
template <typename T>
__global__ __launch_bounds__(256) void image_kernel(const uint8_t* __restrict__ img, T* __restrict__ out, int64_t pixels, ImageP q) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  f32x4 lo = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 3; ++c) lo[c] = (float)(((double)img[3 * i + c] / 255.0 - q.mean[c]) / q.std[c]);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  Vec4<T>::store(out + 8 * i, lo);
  Vec4<T>::store(out + 8 * i + 4, zero);
}

bool mul_fits(int64_t a, int64_t b, int64_t* out) { return !__builtin_mul_overflow(a, b, out); }

}  // namespace

extern "C" int imt_conv2d_supported(int dtype, int Cin, int KH, int KW, int stride) {
  return imt_ok_dtype(dtype) && Cin > 0 && Cin % 8 == 0 && KH > 0 && KW > 0 && (stride == 1 || stride == 2) &&
         (int64_t)KH * KW * Cin <= INT32_MAX;
}

extern "C" int imt_conv2d(const imt_conv_args* a, void* stream) {
  IMT_CHECK_ARG(a != nullptr, "conv2d: null args");
  IMT_CHECK_ARG(imt_ok_dtype(a->dtype), "conv2d: bad dtype %d", a->dtype);
  IMT_CHECK_ARG(a->x != nullptr, "conv2d: x is null");
  IMT_CHECK_ARG(a->w != nullptr, "conv2d: w is null");
  IMT_CHECK_ARG(a->y != nullptr, "conv2d: y is null");
  IMT_CHECK_ARG(a->B > 0 && a->H > 0 && a->W > 0 && a->Cin > 0 && a->Cout > 0 && a->KH > 0 && a->KW > 0,
                "conv2d: sizes must be positive (B %d, H %d, W %d, Cin %d, Cout %d, KH %d, KW %d)", a->B, a->H, a->W, a->Cin, a->Cout, a->KH,
                a->KW);
  IMT_CHECK_ARG(a->stride == 1 || a->stride == 2, "conv2d: stride = %d outside {1, 2}", a->stride);
  IMT_CHECK_ARG(a->pad_h >= 0 && a->pad_w >= 0, "conv2d: negative padding (%d, %d)", a->pad_h, a->pad_w);
  IMT_CHECK_ARG(a->Cin % 8 == 0, "conv2d: Cin = %d must be a multiple of 8", a->Cin);
  IMT_CHECK_ARG(imt_conv2d_supported(a->dtype, a->Cin, a->KH, a->KW, a->stride), "conv2d: K = KH KW Cin does not fit in 31 bits");
  // floored division of a possibly negative numerator: refuse before dividing
  const int64_t nh = (int64_t)a->H + 2 * (int64_t)a->pad_h - a->KH, nw = (int64_t)a->W + 2 * (int64_t)a->pad_w - a->KW;
  IMT_CHECK_ARG(nh >= 0 && nw >= 0, "conv2d: the %d x %d kernel does not fit the padded %d x %d input (Ho or Wo <= 0)", a->KH, a->KW, a->H, a->W);
  const int64_t Ho = nh / a->stride + 1, Wo = nw / a->stride + 1;
  const int es = imt_dtype_bytes(a->dtype);
  // the kernel indexes pixels (b, h, w) and output rows with 32-bit integers and forms byte offsets in 64 bits
  int64_t in_pix, out_pix, xb, wb, yb;
  IMT_CHECK_ARG(mul_fits((int64_t)a->B * a->H, a->W, &in_pix) && in_pix <= INT32_MAX && mul_fits((int64_t)a->B * Ho, Wo, &out_pix) &&
                    out_pix <= INT32_MAX - CV_BM,
                "conv2d: B H W or B Ho Wo does not fit the kernel's 32-bit pixel index");
  IMT_CHECK_ARG(mul_fits(in_pix, (int64_t)a->Cin * es, &xb) && mul_fits((int64_t)a->Cout * a->KH * a->KW, (int64_t)a->Cin * es, &wb) &&
                    mul_fits(out_pix, (int64_t)a->Cout * es, &yb),
                "conv2d: an operand's byte size does not fit the kernel's 64-bit offsets");
  IMT_CHECK_ARG((uintptr_t)a->x % 16 == 0 && (uintptr_t)a->w % 16 == 0 && (uintptr_t)a->y % 16 == 0, "conv2d: x, w and y must be 16-byte aligned");
  IMT_CHECK_ARG(a->residual == nullptr || (uintptr_t)a->residual % 16 == 0, "conv2d: residual must be 16-byte aligned");
  IMT_CHECK_ARG((a->scale == nullptr || (uintptr_t)a->scale % 4 == 0) && (a->shift == nullptr || (uintptr_t)a->shift % 4 == 0),
                "conv2d: scale / shift must be 4-byte aligned");
  ConvP p;
  p.x = a->x; p.w = a->w; p.y = a->y;
  p.scale = a->scale; p.shift = a->shift; p.residual = a->residual;
  p.H = a->H; p.W = a->W; p.Cin = a->Cin; p.Cout = a->Cout; p.KW = a->KW; p.stride = a->stride;
  p.pad_h = a->pad_h; p.pad_w = a->pad_w; p.Ho = (int)Ho; p.Wo = (int)Wo; p.relu = a->relu;
  p.M = (int)out_pix; p.K = a->KH * a->KW * a->Cin;
  const bool wide = conv_wide_tiles(p.M, p.Cout);
  p.tiles_n = imt_cdiv(p.Cout, wide ? 128 : 64);
  const int64_t tiles = (int64_t)imt_cdiv(p.M, CV_BM) * p.tiles_n;
  IMT_CHECK_ARG(tiles <= INT32_MAX, "conv2d: %lld output tiles exceed the grid", (long long)tiles);
  hipStream_t st = (hipStream_t)stream;
  return imt_by_dtype(a->dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    ImtProfScope prof(sizeof(T) == 2 ? "conv_bf16" : "conv_f32", 2.0 * p.M * p.Cout * p.K,
                      (double)xb + (double)wb + (double)yb * (a->residual ? 2.0 : 1.0), st);
    if (wide) hipLaunchKernelGGL((conv2d_kernel<T, 128>), dim3((unsigned)tiles), dim3(CV_THREADS), 0, st, p);
    else hipLaunchKernelGGL((conv2d_kernel<T, 64>), dim3((unsigned)tiles), dim3(CV_THREADS), 0, st, p);
    IMT_CHECK_LAUNCH();
    return (int)IMT_OK;
  });
}

extern "C" int imt_maxpool2d_3x3s2(int dtype, const void* x, void* y, int B, int H, int W, int C, void* stream) {
  IMT_CHECK_ARG(imt_ok_dtype(dtype), "maxpool2d: bad dtype %d", dtype);
  IMT_CHECK_ARG(x != nullptr && y != nullptr, "maxpool2d: null tensor");
  IMT_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0, "maxpool2d: sizes must be positive (B %d, H %d, W %d, C %d)", B, H, W, C);
  IMT_CHECK_ARG(C % 8 == 0, "maxpool2d: C = %d must be a multiple of 8", C);
  IMT_CHECK_ARG((uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0, "maxpool2d: x and y must be 16-byte aligned");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, es = imt_dtype_bytes(dtype);
  int64_t xb, total;
  IMT_CHECK_ARG(mul_fits((int64_t)B * H, (int64_t)W * C, &xb) && mul_fits(xb, es, &xb), "maxpool2d: x does not fit 64-bit byte offsets");
  total = (int64_t)B * Ho * Wo * (C / (16 / es));
  const int64_t blocks = (total + 255) / 256;
  IMT_CHECK_ARG(blocks <= INT32_MAX, "maxpool2d: %lld blocks exceed the grid", (long long)blocks);
  hipStream_t st = (hipStream_t)stream;
  return imt_by_dtype(dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    ImtProfScope prof(sizeof(T) == 2 ? "maxpool_bf16" : "maxpool_f32", 0.0, (double)xb + (double)B * Ho * Wo * C * es, st);
    hipLaunchKernelGGL(maxpool_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<const T*>(x), reinterpret_cast<T*>(y), H, W,
                       C, Ho, Wo, total);
    IMT_CHECK_LAUNCH();
    return (int)IMT_OK;
  });
}

extern "C" int imt_image_nhwc(int dtype, const uint8_t* img, void* out, int B, int H, int W, const float* host_mean, const float* host_std,
                              void* stream) {
  IMT_CHECK_ARG(imt_ok_dtype(dtype), "image_nhwc: bad dtype %d", dtype);
  IMT_CHECK_ARG(img != nullptr && out != nullptr, "image_nhwc: null tensor");
  IMT_CHECK_ARG(host_mean != nullptr && host_std != nullptr, "image_nhwc: null mean / std");
  IMT_CHECK_ARG(B > 0 && H > 0 && W > 0, "image_nhwc: sizes must be positive (B %d, H %d, W %d)", B, H, W);
  IMT_CHECK_ARG((uintptr_t)out % 16 == 0, "image_nhwc: out must be 16-byte aligned");
  ImageP q;
  for (int c = 0; c < 3; ++c) {
    IMT_CHECK_ARG(host_std[c] > 0.f && isfinite(host_std[c]) && isfinite(host_mean[c]), "image_nhwc: std[%d] must be positive and finite", c);
    q.mean[c] = host_mean[c];
    q.std[c] = host_std[c];
  }
  int64_t pixels, ob;
  IMT_CHECK_ARG(mul_fits((int64_t)B * H, W, &pixels) && mul_fits(pixels, 8 * imt_dtype_bytes(dtype), &ob), "image_nhwc: out does not fit 64-bit byte offsets");
  const int64_t blocks = (pixels + 255) / 256;
  IMT_CHECK_ARG(blocks <= INT32_MAX, "image_nhwc: %lld blocks exceed the grid", (long long)blocks);
  hipStream_t st = (hipStream_t)stream;
  return imt_by_dtype(dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    ImtProfScope prof(sizeof(T) == 2 ? "image_bf16" : "image_f32", 0.0, 3.0 * pixels + (double)ob, st);
    hipLaunchKernelGGL(image_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, img, reinterpret_cast<T*>(out), pixels, q);
    IMT_CHECK_LAUNCH();
    return (int)IMT_OK;
  });
}
