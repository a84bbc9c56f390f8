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
#include "search_step.hpp"

namespace {

constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;

// larger float <=> larger key; -0 is folded into +0 first (they compare equal and must share a key)
IMT_DEVICE uint32_t order_key(float x) {
  const uint32_t b = __float_as_uint(x + 0.0f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// hist[digit] += 1 for every lane with `active`.  The leading digit of logits is shared by most of a wave (sign and exponent), and
// 64 lanes adding to one LDS word serialise: two rounds in which the first active lane adds the count of all lanes that hold ITS
// digit take those off; what is left goes one by one.  Lanes that are not in the call count as inactive.
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
  const bool masked = row_finished(a, prow, b);
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
    sweep_row<SAMPLE_THREADS, VEC>(x, V, tid, [&](float q, int v, bool ok) {
      if (ok) {
        if (q > m) { l *= __expf(m - q); m = q; }
        l += __expf(q - m);
      }
      if (select) hist_add(hist, ok, order_key(q) >> 24, lane);
    });
    const float lse = block_lse<SAMPLE_WAVES>(m, l, red_f, red_g, lane, wv);

    // ---- select: the key of the topk-th largest logit, and how many of the logits equal to it are kept
    uint32_t thr = 0;          // kept: key > thr, or key == thr and index <= cutoff
    int cutoff = 0x7fffffff;
    if (select) {
      uint32_t prefix = 0, remaining = (uint32_t)a.topk, count_eq = 0;
      for (int shift = 24; shift >= 0; shift -= 8) {
        if (shift < 24) {
          for (int i = tid; i < 256; i += SAMPLE_THREADS) hist[i] = 0;
          __syncthreads();
          sweep_row<SAMPLE_THREADS, VEC>(x, V, tid, [&](float q, int v, bool ok) {
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
    sweep_row<SAMPLE_THREADS, VEC>(x, V, tid, [&](float q, int v, bool ok) {
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
    block_best<SAMPLE_WAVES>(bs, bi, red_f, red_i, lane, wv);
    if ((unsigned)bi >= (unsigned)V) bi = 0;  // no comparable value (NaN logits): a valid index, the hypothesis is garbage either way
    token = bi;
    score += x[bi] - lse;
  }

  if (tid == 0) commit_hypothesis(a, orow, prow, token, score, masked ? (a.eos_in[prow] != 0) : (a.eos_in[prow] || token == a.eos));
  copy_history(a, orow, prow, tid, SAMPLE_THREADS);
}

}  // namespace

extern "C" int imt_sample_step(const imt_sample_args* a, void* stream) {
  IMT_CHECK_ARG(a, "sample_step: null args");
  IMT_CHECK_ARG(a->B > 0 && a->V > 0 && a->V <= (1 << 30), "sample_step: bad sizes (B %d, V %d)", a->B, a->V);
  IMT_CHECK_ARG(a->n > 0 && a->n <= MAX_HYPS, "sample_step: n %d out of range (1..%d)", a->n, MAX_HYPS);
  if (const int err = check_search_args(a, "sample_step", a->n, "n")) return err;
  IMT_CHECK_ARG(a->temperature > 0.f && a->temperature <= 3.402823466e+38f, "sample_step: temperature must be positive and finite");
  IMT_CHECK_ARG((int64_t)a->B * a->n * a->V < (1ll << 32), "sample_step: B*n*V must stay below 2^32 (the noise index is 32 bits)");
  IMT_CHECK_ARG(a->ld >= a->V, "sample_step: ld smaller than V");
  IMT_CHECK_ARG(a->pad_idx >= 0 && a->eos >= 0, "sample_step: pad_idx / eos negative");
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
