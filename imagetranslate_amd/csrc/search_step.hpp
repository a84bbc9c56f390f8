// What imt_beam_step (decode.hip) and imt_sample_step (sample.hip) share: the sweep of a vocabulary row, the block reductions
// over per-thread partial results, the pick from per-lane sorted lists, the bookkeeping of a chosen hypothesis (the reference's
// src/seq_gen.py:214-227) and the host checks of the arguments both steps take.  Templates over the args type: imt_beam_args
// and imt_sample_args name every shared field alike.
#pragma once
#include "common.hpp"

constexpr int MAX_HYPS = 32;  // hypotheses per sentence (beam width, samples): one search state serves both steps
constexpr int SWEEP_NS = 4;   // sweeps of the row requested together

// ------------------------------------------------------------------------------------------------ row sweep
// quad(q, v, valid) for the four elements from index v, elem(x, v, valid) for single ones: every index of [0, V) exactly once
// over the workgroup, in increasing index order per thread.  A thread's trips end with its last valid index, so the first call
// of a trip is always valid -- its load is then consumed unconditionally and stays ahead of the trip with the others; `valid` is
// false on the clamped re-reads past the end later in that trip.  The lanes of a wave may leave the loop at different trips: a
// functor that votes across the wave sees only the lanes still there (to it, the others hold nothing valid).
// VEC: 16-byte loads (row 16-byte aligned), the up to three elements past V & ~3 go to threads 0..2.
// SWEEP_NS sweeps are REQUESTED together before the first is consumed: one sweep per loop trip was a chain of ~8 exposed load
// latencies per pass -- 41 us per row where the row's 120 KB take ~1 us to stream.
template <int THREADS, bool VEC, typename FQ, typename FE>
IMT_DEVICE void sweep_row(const float* __restrict__ x, int V, int tid, FQ&& quad, FE&& elem) {
  if (VEC) {
    const int V4 = V & ~3;
    for (int v0 = tid * 4; v0 < V4; v0 += SWEEP_NS * THREADS * 4) {
      f32x4 qs[SWEEP_NS];
#pragma unroll
      for (int s = 0; s < SWEEP_NS; ++s) qs[s] = *reinterpret_cast<const f32x4*>(x + min(v0 + s * THREADS * 4, V4 - 4));
#pragma unroll
      for (int s = 0; s < SWEEP_NS; ++s) {
        const int v = v0 + s * THREADS * 4;
        quad(qs[s], v, v < V4);
      }
    }
    if (V4 < V) {
      const int v = V4 + tid;
      elem(x[min(v, V - 1)], v, v < V);
    }
  } else {
    for (int v0 = tid; v0 < V; v0 += SWEEP_NS * THREADS) {
      float qs[SWEEP_NS];
#pragma unroll
      for (int s = 0; s < SWEEP_NS; ++s) qs[s] = x[min(v0 + s * THREADS, V - 1)];
#pragma unroll
      for (int s = 0; s < SWEEP_NS; ++s) {
        const int v = v0 + s * THREADS;
        elem(qs[s], v, v < V);
      }
    }
  }
}
// element by element: a quad is its four elements in index order
template <int THREADS, bool VEC, typename F>
IMT_DEVICE void sweep_row(const float* __restrict__ x, int V, int tid, F&& f) {
  sweep_row<THREADS, VEC>(x, V, tid, [&](f32x4 q, int v, bool ok) {
#pragma unroll
    for (int e = 0; e < 4; ++e) f(q[e], v + e, ok);
  }, f);
}

// ------------------------------------------------------------------------------------------------ block reductions
// Every thread gets the result; `red`: WAVES words of LDS that no thread still reads (each function ends after its reads of
// `red`, so two calls in a row need different arrays or a barrier between them).
template <int WAVES>
IMT_DEVICE float block_max(float v, float* red, int lane, int wv) {
  v = wave_max(v);
  if (lane == 0) red[wv] = v;
  __syncthreads();
  v = red[0];
#pragma unroll
  for (int k = 1; k < WAVES; ++k) v = fmaxf(v, red[k]);
  return v;
}
template <int WAVES>
IMT_DEVICE float block_sum(float v, float* red, int lane, int wv) {  // waves added in order 0, 1, ...
  v = wave_sum(v);
  if (lane == 0) red[wv] = v;
  __syncthreads();
  v = red[0];
#pragma unroll
  for (int k = 1; k < WAVES; ++k) v += red[k];
  return v;
}
// the row's log-sum-exp from the threads' online (max, sum of exp(x - max)) pairs
template <int WAVES>
IMT_DEVICE float block_lse(float m, float l, float* red_f, float* red_g, int lane, int wv) {
  const float mx = block_max<WAVES>(m, red_f, lane, wv);
  return mx + logf(block_sum<WAVES>(m == -INFINITY ? 0.f : l * __expf(m - mx), red_g, lane, wv));
}
// (s, i) <- the block's best pair under better(); the first barrier protects the previous call's reads of red_f / red_i
template <int WAVES>
IMT_DEVICE void block_best(float& s, int& i, float* red_f, int* red_i, int lane, int wv) {
  wave_best(s, i);
  __syncthreads();
  if (lane == 0) { red_f[wv] = s; red_i[wv] = i; }
  __syncthreads();
  s = red_f[0]; i = red_i[0];
#pragma unroll
  for (int k = 1; k < WAVES; ++k)
    if (better(red_f[k], red_i[k], s, i)) { s = red_f[k]; i = red_i[k]; }
}

// The best n (<= K) entries, in order, of the 64 sorted lists that a wave's lanes hold (ls desc, li asc among equal scores, unique
// indices, empty places (-inf, 0x7fffffff)): n rounds of a butterfly arg-best over the list heads; the lane that owned the winner
// pops it and lane 0 calls record(t, score, index).
template <int K, typename R>
IMT_DEVICE void wave_pop_best(float (&ls)[K], int (&li)[K], int n, int lane, R&& record) {
#pragma unroll
  for (int t = 0; t < K; ++t) {
    if (t < n) {
      float bs = ls[0]; int bi = li[0];
      wave_best(bs, bi);
      if (li[0] == bi && bi != 0x7fffffff) {
#pragma unroll
        for (int k = 0; k < K - 1; ++k) { ls[k] = ls[k + 1]; li[k] = li[k + 1]; }
        ls[K - 1] = -INFINITY; li[K - 1] = 0x7fffffff;
      }
      if (lane == 0) record(t, bs, bi);
    }
  }
}

// ------------------------------------------------------------------------------------------------ bookkeeping
// input row `row` of sentence b takes no new token: it holds EOS already, or (after the first step) the sentence is at its limit
template <typename Args>
IMT_DEVICE bool row_finished(const Args& a, int row, int b) {
  return a.eos_in[row] || (a.step > 1 && a.max_lens[b] < (int64_t)a.step + 1);
}
// Output row `orow` extends input row `prow` by `token` (one thread per output row).  The slot write needs step < t_max: both
// entry points refuse anything else (check_search_args), so it is not tested again here.
template <typename Args>
IMT_DEVICE void commit_hypothesis(const Args& a, int orow, int prow, int64_t token, float score, bool has_eos) {
  a.scores_out[orow] = score;
  a.eos_out[orow] = has_eos ? 1 : 0;
  a.parent_out[orow] = prow;
  a.tokens_out[orow] = token;
  a.hist_out[(int64_t)orow * a.t_max + a.step] = token;
  if (a.slots_out) a.slots_out[(int64_t)orow * a.t_max + a.step] = orow;
  if (a.eos_count && has_eos) atomicAdd(a.eos_count + a.step, 1);
}
// columns [0, step) of the parent's history and slot rows, by the threads first, first + stride, ...
template <typename Args>
IMT_DEVICE void copy_history(const Args& a, int orow, int prow, int first, int stride) {
  for (int j = first; j < a.step; j += stride) {
    a.hist_out[(int64_t)orow * a.t_max + j] = a.hist_in[(int64_t)prow * a.t_max + j];
    if (a.slots_out) a.slots_out[(int64_t)orow * a.t_max + j] = a.slots_in[(int64_t)prow * a.t_max + j];
  }
}

// ------------------------------------------------------------------------------------------------ host
// The checks both entry points make (`what`: "beam_step" / "sample_step"; `width`, `width_name`: a->beam, "beam" / a->n, "n").
template <typename Args>
static int check_search_args(const Args* a, const char* what, int width, const char* width_name) {
  IMT_CHECK_ARG(a->rep == 1 || a->rep == width, "%s: rep must be 1 (first step) or %s", what, width_name);
  IMT_CHECK_ARG(a->step >= 1 && a->step < a->t_max, "%s: step %d outside [1, t_max=%d)", what, a->step, a->t_max);
  IMT_CHECK_ARG(a->step == 1 || a->rep == width, "%s: only the first step may have rep == 1", what);
  IMT_CHECK_ARG(a->logits && a->scores_in && a->eos_in && a->max_lens && a->hist_in, "%s: null input", what);
  IMT_CHECK_ARG(a->scores_out && a->eos_out && a->hist_out && a->parent_out && a->tokens_out, "%s: null output", what);
  IMT_CHECK_ARG((a->slots_in == nullptr) == (a->slots_out == nullptr), "%s: slots_in/slots_out must both be given or both NULL", what);
  return IMT_OK;
}
