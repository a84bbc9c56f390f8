// On-device batch construction for MASS (src/utils.py:41-82): span selection, the shifted
// decoder input with its original positions, compaction of the hidden tokens and the 80/10/10 replacement -- integer
// work, one workgroup per sentence, so a MASS step needs no per-token host loop and no host->device copy of masks.
// Randomness is counter-based (counter_uniform of common.hpp: mix32 of (seed, stream, index)), restated bit for bit by oracle/batch_oracle.py;
// the span starts (streams 0, 1) are drawn on the host by utils.mass_span_starts, the 80/10/10 replacement (streams 2, 3) here.
#include "common.hpp"

namespace {

__global__ __launch_bounds__(256) void mass_mask_kernel(imt_mass_args a) {
  const int row = blockIdx.x;
  int64_t* text = a.src_text + (int64_t)row * a.width;
  // The span start is the caller's draw (imt_hip.h): row_offsets, recover_width and the size of `targets` follow from the
  // span CLIPPED at the row's end, so the start that sized them and the start that writes must be one number.  The two
  // clamps and the clip below are restated once on the host, in utils.mass_span_sizes: change them together.
  const int64_t f64 = a.first[row];
  const int first = (int)(f64 < 1 ? 1 : (f64 > a.width ? a.width : f64));
  const int64_t len64 = a.pad_indices[row] / 2;
  const int len = (int)(len64 < 0 ? 0 : (len64 > a.width ? a.width : len64));
  const int last = min(first + len, a.width);  // python slice semantics
  const int64_t off = a.row_offsets[row];
  // span mask
  for (int c = threadIdx.x; c < a.width; c += 256) a.src_mask[(int64_t)row * a.width + c] = (c >= first && c < last) ? 1 : 0;
  // decoder input = tokens first-1 .. last-1 with their original positions (read BEFORE the replacement below)
  for (int k = threadIdx.x; k < a.recover_width; k += 256) {
    const int c = first - 1 + k;
    const bool in = (c >= 0 && c < last && k <= last - first);
    a.to_recover[(int64_t)row * a.recover_width + k] = in ? text[c] : a.pad_id;
    a.positions[(int64_t)row * a.recover_width + k] = in ? (int64_t)c : (int64_t)(a.width - 1);
  }
  __syncthreads();
  // hidden tokens: compacted originals (== prediction targets) and the 80/10/10 replacement, in place
  for (int k = threadIdx.x; k < last - first; k += 256) {
    const int c = first + k;
    const int64_t orig = text[c];
    a.targets[off + k] = orig;
    const uint32_t idx = (uint32_t)(row * a.width + c);
    const float u = counter_uniform(a.seed, 2u, idx);
    int64_t repl = orig;
    if (u < 0.8f) repl = a.mask_id;
    else if (u < 0.9f) {
      const int span = a.vocab - a.n_special;
      int r = (int)(counter_uniform(a.seed, 3u, idx) * (float)span);
      if (r >= span) r = span - 1;
      repl = a.n_special + r;
    }
    text[c] = repl;
  }
}

__global__ __launch_bounds__(256) void mass_unmask_kernel(int64_t* text, const uint8_t* mask, const int64_t* originals,
                                                          const int64_t* row_offsets, int width) {
  __shared__ int s_first;
  const int row = blockIdx.x;
  if (threadIdx.x == 0) s_first = width;
  __syncthreads();
  int mine = width;
  for (int c = threadIdx.x; c < width; c += 256)
    if (mask[(int64_t)row * width + c]) { mine = c; break; }
  atomicMin(&s_first, mine);
  __syncthreads();
  const int first = s_first;
  for (int c = first + threadIdx.x; c < width; c += 256)
    if (mask[(int64_t)row * width + c]) text[(int64_t)row * width + c] = originals[row_offsets[row] + (c - first)];
}

// Non-pad target selection (src/seq2seq.py:175-177, train_image_mt.py:253-256): flat positions p = b*T1 + t of the
// positions whose mask[b, col0 + t] is set, in order, plus the target ids at those positions and their count.  One
// workgroup walks the B*T1 flags in chunks of 1024 with a running offset (ballot + popcount scan per wave, 16 wave
// totals through LDS): ~5 us at 8128 positions instead of ~90 us of nonzero / boolean-index kernels.
// One workgroup, ordered compaction.  Thread t owns the SEL_ITEMS consecutive positions of chunk-local index t; all its
// mask bytes and ids are requested together, unconditionally (clamped), so a chunk of 16384 positions costs two memory
// round trips and one block-wide exclusive scan (the first version walked 1024 positions per trip with three barriers
// each: 60 us for the 8128 positions of a C1 batch, on the critical path in front of the encoder; this one ~6 us).
constexpr int SEL_ITEMS = 16;
__global__ __launch_bounds__(1024) void select_plan_kernel(const uint8_t* __restrict__ mask, int64_t ld_mask,
                                                           const int64_t* __restrict__ ids, int64_t ld_ids, int B, int T1, int col0,
                                                           int32_t* __restrict__ idx, int64_t* __restrict__ targets,
                                                           int32_t* __restrict__ count) {
  __shared__ int wave_tot[16];
  __shared__ int s_base;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = B * T1;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int p0 = 0; p0 < n; p0 += 1024 * SEL_ITEMS) {
    uint8_t mk[SEL_ITEMS];
    int64_t tok[SEL_ITEMS];
    const int first = p0 + tid * SEL_ITEMS;
#pragma unroll
    for (int k = 0; k < SEL_ITEMS; ++k) {
      const int p = min(first + k, n - 1);
      const int b = p / T1, t = p - b * T1;
      mk[k] = mask[(int64_t)b * ld_mask + col0 + t];
      tok[k] = ids[(int64_t)b * ld_ids + col0 + t];
    }
    int mine = 0;
#pragma unroll
    for (int k = 0; k < SEL_ITEMS; ++k) mine += (first + k < n && mk[k] != 0) ? 1 : 0;
    // exclusive scan of `mine` over the workgroup: inclusive wave scan by shuffles, wave totals through LDS
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    int off = s_base + incl - mine;
    for (int k = 0; k < wv; ++k) off += wave_tot[k];
#pragma unroll
    for (int k = 0; k < SEL_ITEMS; ++k) {
      if (first + k < n && mk[k] != 0) {
        idx[off] = first + k;
        targets[off] = tok[k];
        ++off;
      }
    }
    __syncthreads();
    if (tid == 0) {
      int tot = s_base;
      for (int k = 0; k < 16; ++k) tot += wave_tot[k];
      s_base = tot;
    }
    __syncthreads();
  }
  if (tid == 0) count[0] = s_base;
}

// BERT masking for the masked language model (src/utils.py:19-38, include/imt_hip.h): the Bernoulli draw per token, the
// 80/10/10 replacement in place and the ordered compaction of the masked positions (the reference's texts[mask]) in one
// launch, shaped like select_plan_kernel above: one workgroup, chunks of 1024 x SEL_ITEMS positions, every id and pad byte
// of a thread requested together (clamped), one block-wide exclusive scan per chunk.  A thread reads its own positions
// before it writes them and the positions of two threads are disjoint, so the in-place update needs no barrier of its own.
__global__ __launch_bounds__(1024) void mlm_mask_kernel(imt_mlm_args a) {
  __shared__ int wave_tot[16];
  __shared__ int s_base;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = a.n_rows * a.width;
  const int span = a.vocab - a.n_special;
  if (tid == 0) s_base = 0;
  __syncthreads();
  // 64-bit walk: n may be anything below 2^31, so p0 + 16384 and a thread's positions past the end need not fit an int
  for (int64_t p0 = 0; p0 < n; p0 += 1024 * SEL_ITEMS) {
    uint8_t pd[SEL_ITEMS];
    int64_t tok[SEL_ITEMS];
    const int64_t first = p0 + tid * SEL_ITEMS;
#pragma unroll
    for (int k = 0; k < SEL_ITEMS; ++k) {
      const int p = (int)min(first + k, (int64_t)n - 1);
      const int b = p / a.width, t = p - b * a.width;
      pd[k] = a.pads[(int64_t)b * a.ld_pads + t];
      tok[k] = a.texts[p];
    }
    uint32_t sel = 0;
#pragma unroll
    for (int k = 0; k < SEL_ITEMS; ++k) {
      const bool s = first + k < n && pd[k] != 0 && (a.mask_eos || tok[k] != a.eos_id) &&
                     counter_uniform(a.seed, 4u, (uint32_t)(first + k)) < a.mask_prob;
      sel |= (s ? 1u : 0u) << k;
    }
    const int mine = __popc(sel);
    // exclusive scan of `mine` over the workgroup: inclusive wave scan by shuffles, wave totals through LDS
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    int off = s_base + incl - mine;
    for (int k = 0; k < wv; ++k) off += wave_tot[k];
#pragma unroll
    for (int k = 0; k < SEL_ITEMS; ++k) {
      const int64_t p = first + k;
      if (p < n) a.mask[p] = (uint8_t)((sel >> k) & 1u);
      if ((sel >> k) & 1u) {
        a.idx[off] = (int32_t)p;
        a.targets[off] = tok[k];
        ++off;
        const float u = counter_uniform(a.seed, 5u, (uint32_t)p);
        if (u < 0.8f) a.texts[p] = a.mask_id;
        else if (u < 0.9f) {
          int r = (int)(counter_uniform(a.seed, 6u, (uint32_t)p) * (float)span);
          if (r >= span) r = span - 1;
          a.texts[p] = (int64_t)(a.n_special + r);
        }
      }
    }
    __syncthreads();
    if (tid == 0) {
      int tot = s_base;
      for (int k = 0; k < 16; ++k) tot += wave_tot[k];
      s_base = tot;
    }
    __syncthreads();
  }
  if (tid == 0) a.count[0] = s_base;
}

}  // namespace

extern "C" int imt_mlm_mask(const imt_mlm_args* a, void* stream) {
  IMT_CHECK_ARG(a, "mlm_mask: null args");
  IMT_CHECK_ARG(a->n_rows > 0 && a->width > 0, "mlm_mask: bad sizes");
  IMT_CHECK_ARG((int64_t)a->n_rows * a->width < (1ll << 31), "mlm_mask: too many positions");
  IMT_CHECK_ARG(a->mask_prob > 0.f && a->mask_prob < 1.f, "mlm_mask: mask_prob must be in (0, 1)");
  IMT_CHECK_ARG(a->vocab > a->n_special && a->n_special >= 0, "mlm_mask: vocabulary smaller than the special-token block");
  IMT_CHECK_ARG(a->texts && a->pads && a->mask && a->idx && a->targets && a->count, "mlm_mask: null tensor");
  IMT_CHECK_ARG(a->ld_pads >= a->width, "mlm_mask: pad rows overlap");
  hipStream_t st = (hipStream_t)stream;
  ImtProfScope prof("mlm_mask", 0, (double)a->n_rows * a->width * 18, st);
  hipLaunchKernelGGL(mlm_mask_kernel, dim3(1), dim3(1024), 0, st, *a);
  IMT_CHECK_LAUNCH();
  return IMT_OK;
}

extern "C" int imt_select_plan(const uint8_t* mask, int64_t ld_mask, const int64_t* ids, int64_t ld_ids, int B, int T1, int col0,
                               int32_t* idx, int64_t* targets, int32_t* count, void* stream) {
  IMT_CHECK_ARG(mask && ids && idx && targets && count && B > 0 && T1 >= 0 && col0 >= 0, "select_plan: bad args");
  IMT_CHECK_ARG((int64_t)B * T1 < (1ll << 31), "select_plan: too many positions");
  hipLaunchKernelGGL(select_plan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, mask, ld_mask, ids, ld_ids, B, T1, col0, idx,
                     targets, count);
  IMT_CHECK_LAUNCH();
  return IMT_OK;
}

extern "C" int imt_mass_mask(const imt_mass_args* a, void* stream) {
  IMT_CHECK_ARG(a, "mass_mask: null args");
  IMT_CHECK_ARG(a->n_rows > 0 && a->width > 1 && a->recover_width > 0, "mass_mask: bad sizes");
  IMT_CHECK_ARG(a->mask_prob > 0.f && a->mask_prob < 1.f, "mass_mask: mask_prob must be in (0, 1)");
  IMT_CHECK_ARG(a->vocab > a->n_special && a->n_special >= 0, "mass_mask: vocabulary smaller than the special-token block");
  IMT_CHECK_ARG(a->src_text && a->pad_indices && a->row_offsets && a->first && a->src_mask && a->to_recover && a->positions && a->targets,
                "mass_mask: null tensor");
  hipStream_t st = (hipStream_t)stream;
  ImtProfScope prof("mass_mask", 0, (double)a->n_rows * a->width * 17, st);
  hipLaunchKernelGGL(mass_mask_kernel, dim3(a->n_rows), dim3(256), 0, st, *a);
  IMT_CHECK_LAUNCH();
  return IMT_OK;
}

extern "C" int imt_mass_unmask(int64_t* src_text, const uint8_t* src_mask, const int64_t* originals, const int64_t* row_offsets,
                               int n_rows, int width, void* stream) {
  IMT_CHECK_ARG(src_text && src_mask && originals && row_offsets && n_rows > 0 && width > 0, "mass_unmask: bad args");
  hipLaunchKernelGGL(mass_unmask_kernel, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, src_text, src_mask, originals, row_offsets, width);
  IMT_CHECK_LAUNCH();
  return IMT_OK;
}
