// The sampling step: imt_sample_step, the counterpart of imt_beam_step (decode.hip) for drawing from the model.
// One workgroup per OUTPUT hypothesis row; the row's logits (120 KB at V = 30000) are swept from L2 a fixed number of
// times whatever `topk` is:
//   pass A        online max / sum-exp (the score is the model's own log-probability) and, with a top-k filter, the
//                 histogram of the most significant digit of the first select round;
//   select        (top-k only) radix select of the k-th largest logit on its order-preserving 32-bit key: four 8-bit
//                 rounds, each one LDS histogram (integer atomics) + a suffix scan of its 256 bins by wave 0; the first
//                 round's histogram comes from pass A, so three more sweeps;
//   ties          (only if the k-th place is shared by more equal logits than fit) one sweep in index order that finds the
//                 last index kept among the equal ones;
//   draw          Gumbel-max over the kept set: argmax of x / T - log(-log(u)) by (value desc, index asc).
// 2 sweeps without a filter, 5 with one (6 with ties at the k-th place).  No floating-point atomics, no prefix sums over
// probabilities, nothing crosses workgroups but the integer eos_count: the same input gives the same bits.
#include "common.hpp"

namespace {

constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;
constexpr int MAX_SAMPLES = 32;  // MAX_BEAM of decode.hip: one search state serves both steps
constexpr int NS = 4;            // sweeps of the row requested together (decode.hip: beam_row_topk_fast_kernel)

// larger float <=> larger key; -0 is folded into +0 first (they compare equal and must share a key)
IMT_DEVICE uint32_t order_key(float x) {
  const uint32_t b = __float_as_uint(x + 0.0f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// f(value, index, valid) for every index of [0, V) exactly once over the workgroup, in increasing index order per thread, from
// wave-uniform control flow (`valid` is false on the clamped re-reads past the end).  VEC: 16-byte loads (row 16-byte aligned).
template <bool VEC, typename F>
IMT_DEVICE void sweep_row(const float* __restrict__ x, int V, int tid, F&& f) {
  if (VEC) {
    const int V4 = V & ~3;
    for (int base = 0; base < V4; base += NS * SAMPLE_THREADS * 4) {
      f32x4 qs[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) qs[s] = *reinterpret_cast<const f32x4*>(x + min(base + (s * SAMPLE_THREADS + tid) * 4, V4 - 4));
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int v = base + (s * SAMPLE_THREADS + tid) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) f(qs[s][e], v + e, v < V4);
      }
    }
    if (V4 < V) {  // up to three elements
      const int v = V4 + tid;
      f(x[min(v, V - 1)], v, v < V);
    }
  } else {
    for (int base = 0; base < V; base += NS * SAMPLE_THREADS) {
      float qs[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) qs[s] = x[min(base + s * SAMPLE_THREADS + tid, V - 1)];
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int v = base + s * SAMPLE_THREADS + tid;
        f(qs[s], v, v < V);
      }
    }
  }
}

// hist[digit] += 1 for every lane with `active`.  The leading digit of logits is shared by most of a wave (sign and exponent), and
// 64 lanes adding to one LDS word serialise: two rounds in which the first active lane adds the count of all lanes that hold ITS
// digit take those off; what is left goes one by one.  Call from wave-uniform control flow.
IMT_DEVICE void hist_add(uint32_t* hist, bool active, uint32_t digit, int lane) {
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const unsigned long long act = __ballot(active);
    if (act == 0) return;
    const int leader = __ffsll((long long)act) - 1;
    const uint32_t d0 = (uint32_t)__shfl((int)digit, leader, 64);
    const bool same = active && digit == d0;
    const unsigned long long m = __ballot(same);
    if (lane == leader) atomicAdd(&hist[d0], (uint32_t)__popcll(m));
    active = active && !same;
  }
  if (active) atomicAdd(&hist[digit], 1u);
}

template <bool VEC>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_step_kernel(imt_sample_args a) {
  __shared__ float red_f[SAMPLE_WAVES];
  __shared__ float red_g[SAMPLE_WAVES];
  __shared__ int red_i[SAMPLE_WAVES];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_digit, s_remaining, s_count;
  __shared__ int s_cutoff;
  const int orow = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = orow / a.n, k = orow - b * a.n;
  const int prow = b * a.rep + (a.rep == 1 ? 0 : k);
  const float* x = a.logits + (int64_t)prow * a.ld;
  const int V = a.V;
  const bool masked = a.eos_in[prow] || (a.step > 1 && a.max_lens[b] < (int64_t)a.step + 1);
  const bool select = a.topk > 0 && a.topk < V;

  int64_t token = a.pad_idx;
  float score = a.scores_in[prow];
  if (!masked) {  // (block-uniform)
    // ---- pass A: online max / sum-exp; the first select round's histogram
    if (select) {
      for (int i = tid; i < 256; i += SAMPLE_THREADS) hist[i] = 0;
      __syncthreads();
    }
    float m = -INFINITY, l = 0.f;
    sweep_row<VEC>(x, V, tid, [&](float q, int v, bool ok) {
      if (ok) {
        if (q > m) { l *= __expf(m - q); m = q; }
        l += __expf(q - m);
      }
      if (select) hist_add(hist, ok, order_key(q) >> 24, lane);
    });
    float mx = wave_max(m);
    if (lane == 0) red_f[wv] = mx;
    __syncthreads();
    mx = red_f[0];
#pragma unroll
    for (int w = 1; w < SAMPLE_WAVES; ++w) mx = fmaxf(mx, red_f[w]);
    const float part = wave_sum(m == -INFINITY ? 0.f : l * __expf(m - mx));
    if (lane == 0) red_g[wv] = part;
    __syncthreads();
    float tot = red_g[0];
#pragma unroll
    for (int w = 1; w < SAMPLE_WAVES; ++w) tot += red_g[w];
    const float lse = mx + logf(tot);

    // ---- select: the key of the topk-th largest logit, and how many of the logits equal to it are kept
    uint32_t thr = 0;          // kept: key > thr, or key == thr and index <= cutoff
    int cutoff = 0x7fffffff;
    if (select) {
      uint32_t prefix = 0, remaining = (uint32_t)a.topk, count_eq = 0;
      for (int shift = 24; shift >= 0; shift -= 8) {
        if (shift < 24) {
          for (int i = tid; i < 256; i += SAMPLE_THREADS) hist[i] = 0;
          __syncthreads();
          sweep_row<VEC>(x, V, tid, [&](float q, int v, bool ok) {
            const uint32_t key = order_key(q);
            hist_add(hist, ok && (key >> (shift + 8)) == prefix, (key >> shift) & 255u, lane);
          });
        }
        __syncthreads();
        // the bin d with |{digit > d}| < remaining <= |{digit >= d}|: lane j of wave 0 owns bins 4j .. 4j + 3
        if (wv == 0) {
          uint32_t c[4], mine = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) { c[j] = hist[4 * lane + j]; mine += c[j]; }
          uint32_t incl = mine;  // sum over lanes >= this one
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_down((int)incl, o, 64);
            if (lane + o < 64) incl += t;
          }
          uint32_t above = incl - mine;
#pragma unroll
          for (int j = 3; j >= 0; --j) {
            if (above < remaining && above + c[j] >= remaining) { s_digit = 4u * lane + j; s_remaining = remaining - above; s_count = c[j]; }
            above += c[j];
          }
        }
        __syncthreads();
        prefix = (prefix << 8) | s_digit;
        remaining = s_remaining;
        count_eq = s_count;
      }
      thr = prefix;
      if (count_eq > remaining) {
        // ---- ties at the k-th place: the index of the `remaining`-th of the equal logits in index order.  Wave w walks the w-th
        // contiguous sixteenth of the row 64 indices at a time, so a ballot is in index order; count, then the one wave that holds
        // the wanted rank walks its part again.
        if (tid == 0) s_cutoff = 0x7fffffff;
        const int seg = (V + SAMPLE_WAVES - 1) / SAMPLE_WAVES;
        const int lo = min(wv * seg, V), hi = min(lo + seg, V);
        int cnt = 0;
        for (int j0 = lo; j0 < hi; j0 += 64) {
          const int v = j0 + lane;
          const bool eq = v < hi && order_key(x[min(v, V - 1)]) == thr;
          cnt += __popcll(__ballot(eq));
        }
        if (lane == 0) red_i[wv] = cnt;
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wv; ++w) before += red_i[w];
        const int want = (int)remaining - 1 - before;  // rank inside this wave's part
        if (want >= 0 && want < cnt) {
          int seen = 0;
          for (int j0 = lo; j0 < hi; j0 += 64) {
            const int v = j0 + lane;
            const bool eq = v < hi && order_key(x[min(v, V - 1)]) == thr;
            const unsigned long long mm = __ballot(eq);
            const int c = __popcll(mm);
            if (seen + c > want) {
              if (eq && seen + __popcll(mm & ((1ull << lane) - 1ull)) == want) s_cutoff = v;
              break;
            }
            seen += c;
          }
        }
        __syncthreads();
        cutoff = s_cutoff;
      }
    }

    // ---- draw: Gumbel-max over the kept set
    const uint32_t idx0 = (uint32_t)orow * (uint32_t)V;  // host: B*n*V < 2^32
    float bs = -INFINITY; int bi = 0x7fffffff;
    sweep_row<VEC>(x, V, tid, [&](float q, int v, bool ok) {
      if (ok && select) {
        const uint32_t key = order_key(q);
        ok = key > thr || (key == thr && v <= cutoff);
      }
      if (ok) {
        const float u = fmaxf(counter_uniform(a.seed, (uint32_t)a.step, idx0 + (uint32_t)v), 2.9802322387695312e-08f);  // 2^-25
        const float val = q / a.temperature - logf(-logf(u));
        if (better(val, v, bs, bi)) { bs = val; bi = v; }
      }
    });
    wave_best(bs, bi);
    __syncthreads();  // red_f / red_i reads above are done
    if (lane == 0) { red_f[wv] = bs; red_i[wv] = bi; }
    __syncthreads();
    bs = red_f[0]; bi = red_i[0];
#pragma unroll
    for (int w = 1; w < SAMPLE_WAVES; ++w)
      if (better(red_f[w], red_i[w], bs, bi)) { bs = red_f[w]; bi = red_i[w]; }
    if ((unsigned)bi >= (unsigned)V) bi = 0;  // no comparable value (NaN logits): a valid index, the hypothesis is garbage either way
    token = bi;
    score += x[bi] - lse;
  }

  // ---- bookkeeping, as beam_merge_kernel
  if (tid == 0) {
    const bool has_eos = masked ? (a.eos_in[prow] != 0) : (a.eos_in[prow] || token == a.eos);
    a.scores_out[orow] = score;
    a.eos_out[orow] = has_eos ? 1 : 0;
    a.parent_out[orow] = prow;
    a.tokens_out[orow] = token;
    a.hist_out[(int64_t)orow * a.t_max + a.step] = token;
    if (a.slots_out) a.slots_out[(int64_t)orow * a.t_max + a.step] = orow;  // step < t_max (host)
    if (a.eos_count && has_eos) atomicAdd(a.eos_count + a.step, 1);
  }
  for (int j = tid; j < a.step; j += SAMPLE_THREADS) {
    a.hist_out[(int64_t)orow * a.t_max + j] = a.hist_in[(int64_t)prow * a.t_max + j];
    if (a.slots_out) a.slots_out[(int64_t)orow * a.t_max + j] = a.slots_in[(int64_t)prow * a.t_max + j];
  }
}

}  // namespace

extern "C" int imt_sample_step(const imt_sample_args* a, void* stream) {
  IMT_CHECK_ARG(a, "sample_step: null args");
  IMT_CHECK_ARG(a->B > 0 && a->V > 0 && a->V <= (1 << 30), "sample_step: bad sizes (B %d, V %d)", a->B, a->V);
  IMT_CHECK_ARG(a->n > 0 && a->n <= MAX_SAMPLES, "sample_step: n %d out of range (1..%d)", a->n, MAX_SAMPLES);
  IMT_CHECK_ARG(a->rep == 1 || a->rep == a->n, "sample_step: rep must be 1 (first step) or n");
  IMT_CHECK_ARG(a->step >= 1 && a->step < a->t_max, "sample_step: step %d outside [1, t_max=%d)", a->step, a->t_max);
  IMT_CHECK_ARG(a->step == 1 || a->rep == a->n, "sample_step: only the first step may have rep == 1");
  IMT_CHECK_ARG(a->temperature > 0.f && a->temperature <= 3.402823466e+38f, "sample_step: temperature must be positive and finite");
  IMT_CHECK_ARG((int64_t)a->B * a->n * a->V < (1ll << 32), "sample_step: B*n*V must stay below 2^32 (the noise index is 32 bits)");
  IMT_CHECK_ARG(a->ld >= a->V, "sample_step: ld smaller than V");
  IMT_CHECK_ARG(a->pad_idx >= 0 && a->eos >= 0, "sample_step: pad_idx / eos negative");
  IMT_CHECK_ARG(a->logits && a->scores_in && a->eos_in && a->max_lens && a->hist_in, "sample_step: null input");
  IMT_CHECK_ARG(a->scores_out && a->eos_out && a->hist_out && a->parent_out && a->tokens_out, "sample_step: null output");
  IMT_CHECK_ARG((a->slots_in == nullptr) == (a->slots_out == nullptr), "sample_step: slots_in/slots_out must both be given or both NULL");
  hipStream_t st = (hipStream_t)stream;
  const int rows = a->B * a->n;
  const bool select = a->topk > 0 && a->topk < a->V;
  ImtProfScope prof("sample_step", 0, (double)rows * a->V * 4 * (select ? 5 : 2), st);
  const bool vec_ok = (a->ld % 4 == 0) && (((uintptr_t)a->logits & 15) == 0);
  if (vec_ok) hipLaunchKernelGGL(sample_step_kernel<true>, dim3(rows), dim3(SAMPLE_THREADS), 0, st, *a);
  else hipLaunchKernelGGL(sample_step_kernel<false>, dim3(rows), dim3(SAMPLE_THREADS), 0, st, *a);
  IMT_CHECK_LAUNCH();
  return IMT_OK;
}
