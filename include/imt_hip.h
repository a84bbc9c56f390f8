/*
 * imt_hip.h -- C ABI of libimt_hip.so: the MI355X (gfx950) implementation of ImageTranslate's
 * transformer encoder-decoder train-step hot path.
 *
 * The reference (rasoolims/ImageTranslate) has NO native/FFI layer: its hot path is Python nn.Modules on
 * stock PyTorch + HuggingFace transformers==2.9.0.  Each entry point below therefore cites the reference
 * Python (or restated HF-BERT 2.9.0) computation it replaces; the Python classes of the same names in
 * imagetranslate_amd/ bind these through ctypes.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is a DEVICE pointer unless named host_*.
 *   - `stream` is a hipStream_t passed as void*; the library never allocates/frees device memory and
 *     never synchronises the device; every result is complete in `stream` order when the call returns to
 *     the host.  One exception to "no global state": a whole-stack imt_stack_backward forks each layer's
 *     weight-gradient launch onto ONE library-owned non-blocking side stream (created on first use) and
 *     joins it back into `stream` with events before it returns -- so a stack backward is not capturable
 *     into a hipGraph on a single stream unless IMT_DW_SIDE_STREAM=0, and one process drives one GPU from
 *     one thread (the deployment model of this library).  The tuning aids IMT_TRACE / IMT_PROF do allocate
 *     and synchronise; they are off unless their environment variable is set.
 *   - return 0 on success, a negative IMT_ERR_* otherwise; imt_last_error() gives a thread-local message.
 *   - dtype: IMT_F32 (parity mode, exact fp32 MFMA/VALU) or IMT_BF16 (bf16 storage, fp32 accumulate).
 *     "T" below means the element type selected by `dtype`.  Gradients of PARAMETERS are always fp32
 *     and are ACCUMULATED (+=) into the caller's flat gradient buffer.
 *   - leading dimensions are in elements; rows must be 16-byte aligned (ld % 8 == 0 for bf16, % 4 for f32).
 */
#ifndef IMT_HIP_H
#define IMT_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define IMT_OK 0
#define IMT_ERR_BAD_ARG (-1)
#define IMT_ERR_UNSUPPORTED (-2)
#define IMT_ERR_LAUNCH (-3)

#define IMT_F32 0
#define IMT_BF16 1

int imt_version(void);
const char* imt_last_error(void);

/* Optional per-launch profiler used by bench.py for the roofline object: when enabled, every kernel launch is
 * bracketed by two hipEvents recorded on the launch stream.  imt_prof_report waits for the recorded events
 * (host-side), aggregates per kernel kind and clears the log.  flops/bytes are the ALGORITHMIC figures of the
 * launches (2*M*N*K per GEMM; minimal operand traffic for the HBM-bound kernels).  Off by default. */
/* sizeof() of the argument structures below as THIS library was compiled, by name ("imt_gemm_args", "imt_attn_args",
 * "imt_prof_row", "imt_attn_block", "imt_layer_desc", "imt_stack_desc", "imt_stack_io", "imt_attn_decode_args",
 * "imt_decode_io", "imt_beam_args", "imt_mass_args", "imt_score_args", "imt_sample_args", "imt_conv_args"); -1 for an unknown name.  A binding checks its own layout against it
 * once at load time (imagetranslate_amd/_lib.py does): a stale binding then fails loudly instead of passing shifted fields. */
int imt_abi_sizeof(const char* struct_name);

typedef struct imt_prof_row {
  char kind[48];
  int64_t launches;
  double total_ms;
  double flops;
  double bytes;
} imt_prof_row;
/* test utility: `blocks` workgroups of `threads` threads holding `lds_bytes` of LDS each spin for ~`cycles` shader clocks
 * (a stand-in for a long-running communication kernel when measuring the step under CU pressure). */
int imt_debug_spin(int blocks, int threads, int lds_bytes, int64_t cycles, void* stream);
int imt_prof_enable(int on);
int imt_prof_report(imt_prof_row* rows, int max_kinds);

/* ------------------------------------------------------------------ GEMM (all nn.Linear fwd/bwd on the path)
 * layout IMT_NT: C[M,N] = A[M,K] * B[N,K]^T   (y = x W^T : BertSelfAttention.query/key/value, *.dense,
 *                                              BertOutputLayer.layer -- src/bert_seq2seq.py:6-12)
 *        IMT_NN: C[M,N] = A[M,K] * B[K,N]     (dx = dy W)
 *        IMT_TN: C[M,N] = A[K,M]^T * B[K,N]   (dW = dy^T x)
 * epilogue, applied in this order to v = alpha * acc:
 *   bias     : v += bias[n]                                   (T)
 *   aux_mode : IMT_AUX_GELU_FWD  aux[m,n] = v ; v = gelu_erf(v)     (BertIntermediate, src/lm_config.py:7)
 *              IMT_AUX_DGELU     v *= gelu_erf'(aux[m,n])
 *   dropout  : v = keep(seed, m*N+n) ? v/(1-p) : 0            (hidden_dropout_prob, src/lm_config.py:8)
 *   resid    : v += resid[m,n]                                (T)   (BertSelfOutput / BertOutput residual)
 *   accumulate: v += C[m,n]
 *   store as c_dtype (T or IMT_F32).  split_k > 1: fp32 atomicAdd of the raw partial products into C
 *   (c_dtype must be IMT_F32; no other epilogue; C pre-initialised by the caller).
 * Views: every matrix is a view with its own leading dimension (lda / ldb multiples of a 16-byte chunk, ldc a multiple of 4);
 * a contiguous extent of A or B that is not a whole number of chunks (NN / TN only) needs a leading dimension that covers
 * the rounded-up extent.  Results do not depend on memory outside the views: pad elements may hold anything, NaN included,
 * and nothing outside the views of C, aux (IMT_AUX_GELU_FWD) and a_colsum is written.
 */
#define IMT_NT 0
#define IMT_NN 1
#define IMT_TN 2
#define IMT_AUX_NONE 0
#define IMT_AUX_GELU_FWD 1
#define IMT_AUX_DGELU 2
#define IMT_AUX_SPLITK_WS 3 /* aux = fp32 WORKSPACE of split_k * M * N floats: NT / NN product as split_k K-ranges of 256 x 256-tile
                               workgroups, each into its own slab, then one reduce launch into C (C += with accumulate; plain
                               epilogue only: alpha / alpha_dev).  For few output tiles and a very long K (dX through the
                               vocabulary); fixed summation order, no atomics.  split_k = 2..16. */

typedef struct imt_gemm_args {
  int32_t dtype, layout;
  int32_t M, N, K;
  const void* A; int64_t lda;
  const void* B; int64_t ldb;
  void* C; int64_t ldc;
  int32_t c_dtype;
  int32_t accumulate;
  const void* bias;
  const void* resid; int64_t ldr;
  void* aux; int64_t ldaux;
  int32_t aux_mode;
  int32_t split_k;
  float alpha;
  float dropout_p;
  uint64_t dropout_seed;
  const float* alpha_dev; /* nullable device scalar multiplied into alpha (upstream loss gradient, no host sync) */
  float* a_colsum;        /* IMT_TN only, nullable: a_colsum[m] += alpha * sum_k A[k,m]  (bias gradient of the same
                             nn.Linear, fused into its weight-gradient GEMM: dy is read once) */
  int32_t force_general;  /* tests / tuning: kernel variant, 0 = auto, 1 = register-staged double buffer (2 blocks/CU),
                             2 / 4: retired, run as 1, 3 = single LDS buffer + register prefetch (3 blocks/CU),
                             5 = persistent wave-specialised (LDS-DMA producer waves, K a whole number of tiles),
                             6 = 256 x 256 tiles (NT / NN, K a whole number of tiles); any other value is refused
                             (IMT_ERR_BAD_ARG) */
  /* LayerNorm of the finished rows of C, in the same call (HF BertSelfOutput / BertOutput, src/bert_seq2seq.py:84-90,
   * 139-143: LayerNorm(dropout(dense(x)) + input) with the bias / dropout / residual epilogue above).  ln_out != NULL:
   * ln_out[M,N] (ld_ln, type c_dtype) = LayerNorm(C rows; ln_gamma, ln_beta, ln_eps), ln_mean / ln_rstd fp32 [M] (what
   * imt_layernorm_bwd takes).  C still receives the LayerNorm INPUT.  imt_layernorm_fwd runs behind the GEMM (C and ln_out
   * contiguous), or the split-K epilogue launch (splitk_ws below) normalises its rows itself.  (Three reserved
   * fields of the retired ring GEMM and ticket LayerNorm left this struct with library version 101.) */
  const void* ln_gamma; const void* ln_beta;
  void* ln_out; int64_t ld_ln;
  float* ln_mean; float* ln_rstd;
  float ln_eps;
  /* Few output tiles and a long K (the reference's inference and captioning callers: src/seq_gen.py:164-194 decodes
   * batch x beam = 320 rows per step, src/train_captioning.py:51-72 trains on 32 x 31 caption tokens; 128-row tiles then
   * occupy 12-52 of the 256 CUs and each walks the whole K alone).  With a caller-owned fp32 workspace here, imt_gemm may run
   * such a product (NT / NN, K >= 16 tiles) as 2..8 K-ranges per output tile on the persistent kernel, each range into its own
   * fp32 slab, followed by ONE launch that sums the slabs in a fixed order and applies the whole epilogue (bias, GELU /
   * GELU' with aux, dropout, residual, accumulate, C of either type): no atomics, bit-reproducible.  NULL / too small: never
   * taken.  imt_gemm_splitk_ws_bytes() is enough for every product whose 128 x 128 tiles times splits stay <= 256. */
  void* splitk_ws; int64_t splitk_ws_bytes;
} imt_gemm_args;
int64_t imt_gemm_splitk_ws_bytes(void);
int imt_gemm(const imt_gemm_args* a, void* stream);
/* All weight-gradient GEMMs (IMT_TN, fp32 C += alpha * A^T B, optional a_colsum) of one transformer layer in ONE
 * launch (HOST array of `count` descriptors), or of two layers (up to 16 problems).  128 x 128 output tiles; 256 x 128 when
 * every M is a multiple of 256 and those tiles still give three quarters of the CUs one each (same bits either way: one
 * writer per tile, the whole K in ascending order).  Problems that cannot be grouped fall back to imt_gemm each. */
int imt_gemm_grouped_tn(const imt_gemm_args* list, int count, void* stream);
/* The tile order of that launch, evaluated on the host (no GPU needed): for a group of `count` (1..16) problems with
 * tile_rows[i] x tile_cols[i] output tiles, order[3w .. 3w+2] = {problem, tile row, tile column} of hardware workgroup w,
 * w < order_tiles == the group's tile count (at most 640).  Workgroup w runs on XCD w % 8.  plain != 0: the order under
 * IMT_GROUPED_PLAIN_ORDER. */
int imt_gemm_grouped_tile_order(const int* tile_rows, const int* tile_cols, int count, int plain, int* order, int order_tiles);

/* Dense + bias + dropout + residual + LayerNorm in ONE launch -- HF BertSelfOutput / BertOutput as instantiated by
 * src/bert_seq2seq.py:84-90,139-143: out = LayerNorm(dropout(x W^T + bias) + resid; eps), row-complete 32 x N tiles
 * (imagetranslate_amd/csrc/gemm_ln.hip).  x [M,K] (ldx), w [N,K] (ldw), bias / gamma / beta [N], resid [M,N] (ldr, may be
 * NULL), all of `dtype`; pre_ln [M,N] (may be NULL) receives the LayerNorm INPUT (what imt_layernorm_bwd reads as x), out
 * [M,N] its output (both with leading dimension ldo); mean / rstd fp32 [M] (may be NULL).  Dropout uses the element index
 * m * N + n like imt_gemm's epilogue, so imt_layernorm_bwd(dx_dropout_seed = dropout_seed) regenerates the mask.
 * Supported: N in {128, 256, 384, 512}, K a whole number of 128-byte tiles (imt_gemm_bias_residual_ln_supported). */
int imt_gemm_bias_residual_ln_supported(int dtype, int N, int K);
int imt_gemm_bias_residual_ln(int dtype, const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias,
                              const void* resid, int64_t ldr, const void* gamma, const void* beta, void* pre_ln, void* out,
                              int64_t ldo, float* mean, float* rstd, int M, int N, int K, float eps, float dropout_p,
                              uint64_t dropout_seed, void* stream);

/* column sums: out[n] += scale * sum_m X[m,n]  -> bias gradients (fp32, accumulated); scale_dev nullable. */
int imt_colsum(int dtype, const void* X, int64_t ldx, int M, int N, float* out, const float* scale_dev, void* stream);

/* ------------------------------------------------------------------ LayerNorm (torch.nn.LayerNorm, eps 1e-12)
 * fwd: y = (x - mean) * rstd * gamma + beta ; saves mean/rstd (fp32, [rows]) for backward.
 *      optional dropout on y (BertEmbeddings: dropout(LN(.))).
 * bwd: dx = LN'(dy) ; dgamma/dbeta accumulated (fp32 atomics) ; optional second output
 *      dx_drop = dropout-masked dx (grad w.r.t. the dense output that was dropped before the residual add).
 */
int imt_layernorm_fwd(int dtype, const void* x, const void* gamma, const void* beta, void* y, float* mean,
                      float* rstd, int rows, int d, float eps, float dropout_p, uint64_t dropout_seed,
                      void* stream);
/* y = dropout(LayerNorm(x + resid)), sum_out = x + resid (what imt_layernorm_bwd reads as its x): the residual add of
 * BertSelfOutput / BertOutput (src/bert_seq2seq.py:84-90) for callers whose dense layer did not fuse it. */
int imt_add_layernorm_fwd(int dtype, const void* x, const void* resid, const void* gamma, const void* beta, void* sum_out,
                          void* y, float* mean, float* rstd, int rows, int d, float eps, float dropout_p,
                          uint64_t dropout_seed, void* stream);
int imt_layernorm_bwd(int dtype, const void* dy, const void* x, const void* gamma, const float* mean,
                      const float* rstd, void* dx, float* dgamma, float* dbeta, int rows, int d,
                      float y_dropout_p, uint64_t y_dropout_seed, void* dx_drop, float dx_dropout_p,
                      uint64_t dx_dropout_seed, float* partial_ws, void* stream);
/* partial_ws: NULL, or an [IMT_LN_PARTIAL_COPIES][2][d] fp32 buffer ZEROED by the caller (IMT_LN_BWD_WS_FLOATS(d) floats).  When given, the
 * per-workgroup column sums are added to copy (workgroup % copies) of it INSTEAD of dgamma / dbeta: 256 workgroups adding
 * into the same d addresses serialise at the memory side (~6 us per launch at rows=8192, d=512), separate copies
 * (each XCD has its own) do not.  imt_ln_partial_reduce then folds any number of such buffers into the gradients in ONE launch:
 * grads[dgamma_off[i] + c] += sum_k partials[i][k][0][c], likewise dbeta (offsets are HOST arrays of element offsets
 * into `grads`, a negative dgamma offset skips that buffer; at most 224 buffers per call, laid out back to back).  (Also measured, slower: a same-launch "last
 * workgroup of a group sums its group" reduction -- its device-scope release fence writes back the XCD's L2.) */
#define IMT_LN_PARTIAL_COPIES 32   /* a multiple of the 8 XCDs: workgroup b -> copy b % 32 stays on XCD b % 8 */
#define IMT_LN_BWD_WS_FLOATS(d) (IMT_LN_PARTIAL_COPIES * 2 * (int64_t)(d))
int imt_ln_partial_reduce(const float* partials, int n_sites, int d, const int64_t* host_dgamma_off,
                          const int64_t* host_dbeta_off, float* grads, void* stream);

/* ------------------------------------------------------------------ embeddings (HF BertEmbeddings)
 * fwd: out[n,:] = word[ids[n]] + pos[pos_ids ? pos_ids[n] : n % seq_len] + type[type_ids[n]]   (pre-LN sum)
 * bwd: scatter-add d(sum) into the three fp32 gradient tables; word rows with id == pad_id get no gradient
 *      (nn.Embedding padding_idx).
 */
int imt_embed_fwd(int dtype, const int64_t* ids, const int64_t* pos_ids, const int64_t* type_ids,
                  const void* word, const void* pos, const void* type, void* out, int n_tokens, int seq_len,
                  int d, int vocab, int max_pos, int n_types, void* stream);
int imt_embed_bwd(int dtype, const int64_t* ids, const int64_t* pos_ids, const int64_t* type_ids,
                  const void* dsum, float* dword, float* dpos, float* dtype_tab, int n_tokens, int seq_len, int d,
                  int64_t pad_id, void* stream);
/* BertEmbeddings in ONE launch: sum_out[n,:] = word[ids[n]] + pos[...] + type[...] (kept for the backward),
 * y = dropout(LayerNorm(sum_out)) -- imt_embed_fwd + imt_layernorm_fwd without the round trip of the sum. */
int imt_embed_ln_fwd(int dtype, const int64_t* ids, const int64_t* pos_ids, const int64_t* type_ids, const void* word,
                     const void* pos, const void* type, const void* gamma, const void* beta, void* sum_out, void* y,
                     float* mean, float* rstd, int n_tokens, int seq_len, int d, int vocab, int max_pos, int n_types, float eps,
                     float dropout_p, uint64_t dropout_seed, void* stream);

/* ------------------------------------------------------------------ attention (HF BertSelfAttention)
 * scores = Q K^T * scale + additive mask ; P = softmax ; [dropout(P)] ; O = P V, heads merged in the output.
 * Q/K/V are strided views: element (b, t, h, e) at base[(b*T + t)*ld + h*head_dim + e]
 * mask semantics == (1 - m) * -10000.0 added to the scaled scores (src/bert_seq2seq.py:25-38, HF
 * get_extended_attention_mask), m = AND of:
 *   key_mask[b, j]   (uint8, nullable)  -- encoder pad mask / encoder_attention_mask
 *   causal: j <= i   (flag)             -- future_mask / is_decoder 2-D mask
 *   query_mask[b, i] (uint8, nullable)  -- the tgt_mask.unsqueeze(-1) factor of future_mask (src/seq2seq.py:14-17)
 *   mask3d[b, i, j]  (uint8, nullable)  -- arbitrary 3-D tgt_attention_mask
 * lse[b,h,i] (fp32) = log-sum-exp of the masked scaled scores, saved for backward.
 * Backward kernels (bf16): Tq, Tk <= 128 one fused single-workgroup kernel per (batch, head); 129..256 (MASS, BASELINE
 * configs[4]: src/mass_seq2seq.py:32-60 runs the encoder over 256 tokens) its 256-key sibling; longer sequences and fp32 the
 * dQ + dK/dV kernel pair.  All are free of cross-workgroup sums: bit-reproducible.
 */
typedef struct imt_attn_args {
  int32_t dtype;
  int32_t B, H, Tq, Tk, head_dim;
  const void* Q; int64_t ldq;
  const void* K; int64_t ldk;
  const void* V; int64_t ldv;
  void* O; int64_t ldo;
  float* lse;
  const uint8_t* key_mask;
  const uint8_t* query_mask;
  const uint8_t* mask3d;
  int32_t causal;
  float scale;
  float dropout_p;
  uint64_t dropout_seed;
  /* backward only */
  const void* dO; int64_t lddo;
  void* dQ; int64_t lddq;
  void* dK; int64_t lddk;
  void* dV; int64_t lddv;
  float* delta; /* workspace [B,H,Tq] fp32: rowsum(dO * O) */
} imt_attn_args;
int imt_attention_fwd(const imt_attn_args* a, void* stream);
int imt_attention_bwd(const imt_attn_args* a, void* stream);
/* The backward of an attention whose output went through BertSelfOutput's projection y = ctx W_o^T: dO = dy W_o is formed
 * INSIDE the attention backward (bf16, head_dim 64, Tq and Tk <= 128, d_model = 64 H, no 3-D mask; one workgroup per (batch,
 * head) multiplies its 64 columns of it) instead of by an NN imt_gemm into a buffer that imt_attention_bwd reads back.  a: as
 * for imt_attention_bwd, except that a->dO may be NULL (dO is never stored) or an OUTPUT [B*Tq, >= d_model] (lddo).  dy
 * [B*Tq, d_model] (lddy), w_o [d_model, d_model] row-major (ldw); both 16-byte aligned with leading dimensions that are
 * multiples of 8.  Bit-identical to imt_gemm (NN, alpha 1) + imt_attention_bwd.  _supported() == 0: the caller keeps the pair. */
int imt_attention_bwd_proj_supported(int dtype, int head_dim, int H, int Tq, int Tk, int d_model, int has_mask3d);
int imt_attention_bwd_proj(const imt_attn_args* a, const void* dy, int64_t lddy, const void* w_o, int64_t ldw, int d_model,
                           void* stream);

/* ------------------------------------------------------------------ row select (src/seq2seq.py:175-177)
 * gather: out[r,:] = x[idx[r],:] ; scatter (its backward): dx[idx[r],:] = dout[r,:] (dx pre-zeroed by caller
 * or zero_rest=1 to have the kernel write zeros to unselected rows given the inverse map).
 */
int imt_gather_rows(int dtype, const void* x, int64_t ldx, const int32_t* idx, void* out, int64_t ldo, int n_sel,
                    int d, void* stream);
int imt_scatter_rows(int dtype, const void* dout, int64_t ldo, const int32_t* idx, void* dx, int64_t ldx, int n_sel,
                     int d, void* stream);

/* ------------------------------------------------------------------ log-softmax + label-smoothed NLL
 * (F.log_softmax src/seq2seq.py:179-180 ; SmoothedNLLLoss src/loss.py:10-27 ; .mean() train_image_mt.py:282)
 * imt_log_softmax_fwd : lp = logits - logsumexp(logits) rowwise  (fp32 out, [N,V]); lse saved.
 * imt_smoothed_nll_fwd: loss[r] = (1-eps)*(-lp[r,t]) + (eps/V)*(-sum_v lp[r,v]) ; 0 where t == ignore_index.
 * imt_xent_fused_fwd_bwd: from raw logits (T, [N,V], in place): per-row loss and
 *      dlogits = grad_scale * (softmax - ((1-eps)*onehot + eps/V)), 0 on ignored rows, written over logits.
 */
int imt_log_softmax_fwd(int dtype, const void* logits, int64_t ld, float* lp, int64_t ldlp, float* lse, int N, int V,
                        void* stream);
int imt_log_softmax_bwd(const float* dlp, int64_t lddlp, const float* lp, int64_t ldlp, int out_dtype, void* dlogits,
                        int64_t ld, int N, int V, void* stream);
int imt_smoothed_nll_fwd(const float* lp, int64_t ldlp, const int64_t* target, float* loss, int N, int V,
                         float epsilon, int64_t ignore_index, void* stream);
int imt_smoothed_nll_bwd(const float* dloss, const int64_t* target, float* dlp, int64_t lddlp, int N, int V,
                         float epsilon, int64_t ignore_index, void* stream);
int imt_xent_fused_fwd_bwd(int dtype, void* logits, int64_t ld, const int64_t* target, float* loss_rows, int N,
                           int V, float epsilon, int64_t ignore_index, float grad_scale, void* stream);

/* ------------------------------------------------------------------ scoring of given targets (src/score_pairs.py:116-127)
 * The reference scores a translation candidate with the teacher-forced decoder: output layer (BertOutputLayer.layer,
 * src/bert_seq2seq.py:6-12), F.log_softmax, gather of the target ids, per-sentence sum / mean.  imt_score_rows does the
 * tail of that in two launches and never stores the [N, V] logits:
 *   logit[r, v] = sum_k x[r, k] w[v, k] + bias[v]          (fp32 accumulate; never rounded to T)
 *   lse[r]      = log sum_v exp(logit[r, v])
 *   logprob[r]  = logit[r, target[r]] - lse[r]             (0 where target[r] is outside [0, V): the row is ignored)
 *   seg_score[s] = sum of logprob over rows [seg_offsets[s], seg_offsets[s+1]), divided by the number of non-ignored rows of
 *                  the segment when normalize != 0 (a segment with none scores 0).
 * Launch 1 (profiling kind score_xl_bf16 / score_xl_f32) is imt_gemm's 256 x 256-tile NT main loop with an epilogue that
 * reduces each tile to one (max, sum exp) pair per row and picks out the target's logit; launch 2 (score_combine) merges
 * the column tiles of a row in tile order and sums the rows of a segment in a fixed order.  No atomics: two calls on the
 * same input give the same bits.  ws: caller-owned scratch of imt_score_ws_bytes(N, V) bytes = the [N] target logits
 * (rounded up to 256 bytes) + ceil(V / 256) x N float2 partials; contents are undefined afterwards.
 * imt_score_supported: 1 where the fused kernel takes (dtype, V, K): K a whole number of 128-byte K tiles (64 bf16 / 32
 * fp32 elements) and a weight below 2 GiB.  imt_score_rows returns IMT_ERR_BAD_ARG before any launch otherwise, and on a bad
 * dtype, null x / w / target / logprob, N, V, K <= 0 or a workspace that is too small.  ldx / ldw in elements, rows 16-byte
 * aligned. */
typedef struct imt_score_args {
  int32_t dtype;                 /* IMT_F32 / IMT_BF16: type of x, w, bias */
  int32_t N, V, K;               /* rows, vocabulary, hidden size */
  const void* x; int64_t ldx;    /* [N, K] decoder output rows */
  const void* w; int64_t ldw;    /* [V, K] BertOutputLayer.layer.weight */
  const void* bias;              /* [V], nullable */
  const int64_t* target;         /* [N]; a target outside [0, V) marks the row as ignored */
  float* logprob;                /* [N] out: logit[target] - lse; 0 for ignored rows */
  float* lse;                    /* [N] out, nullable */
  const int64_t* seg_offsets;    /* [n_seg + 1] device, nullable: rows [off[s], off[s+1]) form sentence s */
  int32_t n_seg, normalize;      /* normalize != 0: divide by the number of non-ignored rows of the segment */
  float* seg_score;              /* [n_seg] out (with seg_offsets) */
  void* ws; int64_t ws_bytes;    /* caller-owned workspace, >= imt_score_ws_bytes(N, V) */
} imt_score_args;
int64_t imt_score_ws_bytes(int N, int V);
int imt_score_supported(int dtype, int V, int K);
int imt_score_rows(const imt_score_args* a, void* stream);
/* ------------------------------------------------------------------ k nearest neighbours by inner product (sentence mining)
 * For queries x [N, K] and keys y [M, K] of one dtype: s[r, c] = sum_k x[r, k] y[c, k] (fp32 accumulate, imt_gemm's K order).
 *   val [N, k] fp32, idx [N, k] int32: row r holds the k largest s[r, .], ordered by value descending, then index ascending;
 *   ties at any place, the k-th included, go to the lowest indices.  idx stores c + index_base (key chunks report global
 *   indices).  Places j >= M hold val = -inf, idx = -1.
 * Launch 1 (profiling kind knn_xl_bf16 / knn_xl_f32) is imt_gemm's 256 x 256-tile NT main loop; one workgroup walks the column
 * tiles of one of `splits` column ranges of a 256-row block and keeps the rows' running lists in LDS; launch 2 (knn_combine)
 * merges the ranges of a row in column order.  The [N, M] similarities are never stored.  No atomics: two calls on the same
 * input give the same bits, and so do calls with different `splits`.  splits = 0 lets the host choose (enough workgroups for
 * the chip when N is small).  ws: caller-owned scratch of imt_knn_ws_bytes(N, M, k, splits) bytes = N x splits x k floats
 * (rounded up to 256 bytes) + as many int32; contents are undefined afterwards.
 * imt_knn_supported: 1 where K is a whole number of 128-byte K tiles (64 bf16 / 32 fp32 elements).
 * Refused before any launch with IMT_ERR_BAD_ARG: null args or tensors, a bad dtype, N, M or K <= 0, k outside
 * 1..IMT_KNN_MAX_K, splits outside 0..IMT_KNN_MAX_SPLITS, an unsupported K, ldx / ldy (in elements) below K or rows not 16-byte
 * aligned, (rows + 256) * ld * element size >= 2^31 for either operand (32-bit DMA offsets), a workspace that is misaligned
 * or too small, index_base < 0 or index_base + M above 2^31 - 1. */
#define IMT_KNN_MAX_K 8
#define IMT_KNN_MAX_SPLITS 256
typedef struct imt_knn_args {
  int32_t dtype;                 /* IMT_F32 / IMT_BF16: type of x and y */
  int32_t N, M, K, k;            /* queries, keys, vector length, neighbours per query */
  const void* x; int64_t ldx;    /* [N, K] queries */
  const void* y; int64_t ldy;    /* [M, K] keys */
  int32_t index_base;            /* added to every stored index */
  int32_t splits;                /* 0: host's choice; else 1..IMT_KNN_MAX_SPLITS column ranges */
  float* val;                    /* [N, k] out */
  int32_t* idx;                  /* [N, k] out */
  void* ws; int64_t ws_bytes;    /* caller-owned workspace, >= imt_knn_ws_bytes(N, M, k, splits) */
} imt_knn_args;
int64_t imt_knn_ws_bytes(int N, int M, int k, int splits);
int imt_knn_supported(int dtype, int K);
int imt_knn_rows(const imt_knn_args* a, void* stream);
/* ------------------------------------------------------------------ word alignment of sentence pairs (argmax / intersection)
 * B independent problems: x [B, S, d] and y [B, T, d] of one dtype, token ranges xr [B, 2] / yr [B, 2] (begin, end) int32 on the
 * device.  For i in xr[b], j in yr[b]:
 *   sim[b, i, j] = (x[b, i] . y[b, j]) / (max(|x[b, i]|, 1e-12) max(|y[b, j]|, 1e-12))     products and norms in fp32
 *   fwd_idx[b, i] = the LOWEST j in range of maximal sim, fwd_val[b, i] that value; bwd_idx[b, j] / bwd_val[b, j] likewise over i
 *   link[b, i]    = fwd_idx[b, i] if bwd_idx[b, fwd_idx[b, i]] == i and fwd_val[b, i] >= min_sim, else -1
 * Positions outside their range, and all positions of a pair whose other range is empty, hold -1 / -inf.  The kernel clamps
 * the ranges to [0, S] / [0, T] (end below begin: empty); rows outside them never reach a result, whatever they hold.
 * One launch (profiling kind align_bf16 / align_f32), one workgroup per pair: it walks 64 x 64 tiles of the pair's ranges
 * (MFMA, 128 bytes of d per step), takes the norms from the staged operands, keeps the running maxima of both directions in
 * LDS and finishes with the mutual test.  Neither the similarities nor normalised rows are stored; no workspace; no atomics:
 * two calls give the same bits, and a pair's outputs do not depend on B or on the other pairs.
 * imt_align_supported: 1 where d is a whole number of 128-byte steps (64 bf16 / 32 fp32 elements).
 * Refused before any launch with IMT_ERR_BAD_ARG: null args or tensors, a bad dtype, B <= 0, S or T outside
 * 1..IMT_ALIGN_MAX_LEN, an unsupported d, row strides (elements) below d, batch strides below (rows - 1) * ld + d, bases or
 * strides that leave rows off 16-byte boundaries, an operand whose last byte offset does not fit in 63 bits. */
#define IMT_ALIGN_MAX_LEN 512
typedef struct imt_align_args {
  int32_t dtype;                          /* IMT_F32 / IMT_BF16: type of x and y */
  int32_t B, S, T, d;                     /* pairs, source / target positions, vector length */
  const void* x; int64_t ldx, bsx;        /* [B, S, d]: row and batch stride in elements */
  const void* y; int64_t ldy, bsy;        /* [B, T, d] */
  const int32_t* xr;                      /* [B, 2] (begin, end) of the source tokens to align */
  const int32_t* yr;                      /* [B, 2] of the target tokens */
  float min_sim; int32_t reserved;        /* links below min_sim are dropped (-inf: keep all) */
  int32_t* link;                          /* [B, S] out */
  int32_t* fwd_idx; float* fwd_val;       /* [B, S] out */
  int32_t* bwd_idx; float* bwd_val;       /* [B, T] out */
} imt_align_args;
int imt_align_supported(int dtype, int d);
int imt_align_pairs(const imt_align_args* a, void* stream);
/* out[0] = scale * sum(x[0..n)), fixed summation order: the `.mean()` of the per-row losses (train_image_mt.py:282). */
int imt_scaled_sum(const float* x, int n, float scale, float* out, void* stream);

/* ------------------------------------------------------------------ frozen ResNet trunk: pixels -> region features
 * ModifiedResnet up to x8.view().permute() (src/image_model.py:24-36; init_net :85-97 picks the depth): conv1 / bn1 / relu /
 * maxpool / layer1..4 of a torchvision ResNet in inference mode.  Forward only; BatchNorm arrives folded into a per-channel
 * scale and shift.  Activations are NHWC, so the last layer's [B, H/32, W/32, C] IS the reference's
 * view(B, C, -1).permute(0, 2, 1).
 *
 * imt_conv2d: 2-D convolution as an implicit GEMM on MFMA.  x [B, H, W, Cin], w [Cout, KH, KW, Cin], y [B, Ho, Wo, Cout], all of
 *   `dtype`, Ho = (H + 2 pad_h - KH) / stride + 1 (floored), Wo likewise; stride 1 or 2, symmetric zero padding, dilation 1,
 *   groups 1.  GEMM view M = B Ho Wo, N = Cout, K = KH KW Cin in (kh, kw, c) order; fp32 accumulation, K ascending (imt_gemm's
 *   rule; IMT_F32 is the exact fp32 MFMA chain).  Epilogue on the fp32 accumulator, in this order:
 *     v = acc * scale[c] + shift[c]      (fp32 [Cout], each nullable: 1 / 0)
 *     v += residual[b, ho, wo, c]        (T, nullable)
 *     v = max(v, 0) when relu != 0
 *   then one store as T.  Cin must be a multiple of 8 (a tap is whole 16-byte chunks; the stem's 3 channels are padded to 8 by
 *   imt_image_nhwc and zero weights); M, Cout and K need not be whole tiles and H, W may be odd.  A tap in the padding contributes
 *   zeros by predicate: no byte outside x's B H W Cin elements is read and none outside y is written, whatever surrounds them.
 *   One launch (profiling kind conv_bf16 / conv_f32), one writer per output element, no atomics, no workspace: two calls give
 *   the same bits.
 *   Refused before any launch with IMT_ERR_BAD_ARG: null args, x, w or y; a bad dtype; a non-positive size; stride outside
 *   {1, 2}; negative padding; Cin % 8 != 0; Ho or Wo <= 0; x, w, y or residual off a 16-byte boundary; B H W or B Ho Wo beyond
 *   the kernel's 32-bit pixel index, K beyond 31 bits, or an operand whose byte size overflows its 64-bit offsets.
 *   imt_conv2d_supported: 1 for a (dtype, Cin, KH, KW, stride) the kernel takes.
 * imt_maxpool2d_3x3s2: NHWC max pool, kernel 3, stride 2, padding 1 (the stem's nn.MaxPool2d): y [B, (H - 1) / 2 + 1,
 *   (W - 1) / 2 + 1, C].  Padding counts as -inf, so an all-negative window keeps its negative maximum.  C % 8 == 0 (16-byte
 *   loads over channels).  Profiling kind maxpool_bf16 / maxpool_f32.
 * imt_image_nhwc: decoded images uint8 [B, H, W, 3] (what PIL hands over; transforms.ToTensor + Normalize of
 *   src/dataset.py:283-289) -> out [B, H, W, 8] of `dtype`: channels 0-2 = (v / 255 - mean[c]) / std[c], evaluated in fp64 and
 *   rounded once to fp32 (then to bf16); channels 3-7 = 0.  host_mean / host_std: 3 HOST floats each.  Profiling kind image_*. */
typedef struct imt_conv_args {
  int32_t dtype;                          /* IMT_F32 / IMT_BF16: type of x, w, y and residual */
  int32_t B, H, W, Cin, Cout, KH, KW;
  int32_t stride, pad_h, pad_w;
  int32_t relu;
  const void* x; const void* w; void* y;
  const float* scale; const float* shift; /* fp32 [Cout], nullable */
  const void* residual;                   /* [B, Ho, Wo, Cout], nullable */
} imt_conv_args;
int imt_conv2d_supported(int dtype, int Cin, int KH, int KW, int stride);
int imt_conv2d(const imt_conv_args* a, void* stream);
int imt_maxpool2d_3x3s2(int dtype, const void* x, void* y, int B, int H, int W, int C, void* stream);
int imt_image_nhwc(int dtype, const uint8_t* img, void* out, int B, int H, int W, const float* host_mean, const float* host_std,
                   void* stream);

/* ------------------------------------------------------------------ data-parallel gradient exchange (RCCL over xGMI)
 * Replaces torch DistributedDataParallel's NCCL all-reduce of src/train_image_mt.py:72-76 (bootstrap src/utils.py:93-97):
 * one process per GPU, one communicator per process.  Rank 0 calls imt_comm_get_unique_id and hands the
 * imt_comm_unique_id_bytes() (= 128) HOST bytes to every rank out of band; every rank then calls imt_comm_init with the
 * same id.  imt_comm_allreduce: in-place SUM of `count` elements over the ranks, asynchronous in `stream` (issue one call
 * per gradient bucket as the backward finalises it; fold 1 / world_size into imt_clip_adam's grad_scale);
 * imt_comm_broadcast: rank `root`'s buffer to all (the parameter broadcast of DDP's constructor).  librccl is opened at
 * first use (no load-time dependency); every function returns IMT_ERR_* with a message on RCCL errors. */
int imt_comm_unique_id_bytes(void);
int imt_comm_get_unique_id(void* host_id_out);
int imt_comm_init(const void* host_unique_id, int world_size, int rank, void** comm_out);
int imt_comm_allreduce(void* comm, void* buf, int64_t count, int dtype, void* stream);
int imt_comm_broadcast(void* comm, void* buf, int64_t count, int dtype, int root, void* stream);
int imt_comm_destroy(void* comm);

/* GEMM selection policy for data-parallel runs: share_cus != 0 makes the one-tile-per-CU products with K < 1024 take the
 * three-workgroups-per-CU kernel instead of the persistent one-workgroup-per-CU kernel, which needs a whole second round
 * as soon as a collective's resident kernels hold a few CUs.  Returns the previous setting.
 * The environment variable IMT_GEMM_SHARE_CUS (0 / 1), when set, overrides this call. */
int imt_set_gemm_share_cus(int share_cus);
/* Tests / tuning: the fewest 256 x 128 tiles with which imt_gemm_grouped_tn takes them (and the stack's backward launches
 * the weight gradients of two layers at once) where every row count allows; 0 = the default, three quarters of the CUs.
 * Returns the previous setting. */
int imt_set_gemm_grouped_tall_min_tiles(int min_tiles);

/* ------------------------------------------------------------------ optimizer
 * (clip_grad_norm_ train_image_mt.py:291 ; AdamInverseSqrtWithWarmup src/utils.py:105-156)
 * imt_sumsq       : out[0] += sum(g^2) over n fp32 elements (out pre-zeroed by caller); DETERMINISTIC (fixed
 *                   reduction order: data-parallel replicas holding identical gradients get identical norms);
 *                   partial_ws = IMT_SUMSQ_WS_FLOATS floats of scratch.
 * imt_clip_adam   : clip_coef = min(1, max_norm / (sqrt(sumsq[0]) + 1e-6)) ; g *= clip_coef ;
 *                   Adam(beta1, beta2, eps, no weight decay, bias-corrected) on fp32 master params ;
 *                   optionally writes the bf16 shadow copy ; optionally zeroes g.
 *                   lr and step are read from the host args (one launch per step).
 * imt_clip_scale  : g *= grad_scale * min(1, max_norm / (grad_scale * sqrt(sumsq[0]) + 1e-6)) in place: the clip of a
 *                   gradient-accumulation micro-step that does not end in an optimizer step (train_image_mt.py:291-295:
 *                   clip after every backward, step every `accum`).
 */
#define IMT_SUMSQ_WS_FLOATS 1024
int imt_sumsq(const float* g, int64_t n, float* out, float* partial_ws, void* stream);
int imt_clip_adam(float* p, float* g, float* m, float* v, void* p_bf16, int64_t n, const float* sumsq,
                  float max_norm, float grad_scale, float lr, float beta1, float beta2, float eps, int64_t step,
                  int zero_grad, void* stream);
int imt_clip_scale(float* g, int64_t n, const float* sumsq, float max_norm, float grad_scale, void* stream);
int imt_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
int imt_gated_mix(int dtype, const void* a, const void* b, const void* gate, void* out, int64_t rows, int d,
                  void* stream);
/* Image head glue (ModifiedResnet head, src/image_model.py:37-41,77-78: dropout -> fc -> + location_embedding -> dropout;
 * the fc itself is imt_gemm): out[r, :] = dropout(x[r, :] + add[r % period, :]), x of in_dtype, out / add of out_dtype,
 * add may be NULL (plain dropout; with the forward's seed this is also the dropout's backward). */
int imt_add_rows_dropout(int in_dtype, const void* x, int out_dtype, void* out, const void* add, int64_t rows, int d,
                         int period, float dropout_p, uint64_t dropout_seed, void* stream);

/* ------------------------------------------------------------------ object stream of ImageCaptioning
 * Pre-extracted detector output (box features [R, 1024], boxes [R, 4] = x1 y1 x2 y2, labels [R] int64, 0 = padding) enters the
 * object head of src/image_model.py:58-78: row = [object_embedding[label] (d) | feature (1024) | locs (7)], locs = x1/800,
 * x2/800, y1/800, y2/800, w, h, w*h (w = x2/800 - x1/800, h likewise); a label-0 row is zeroed whole; then
 * relu(object_feat_fc(row)) (no bias) and dropout.  K = d + 1031 is odd, so the product runs on K-padded operands:
 * imt_obj_rows   : X [R, Kp] in `dtype` (Kp >= d + 1031, Kp % 8 == 0, pad columns zero) from labels / feats (`feat_dtype`) /
 *                  boxes (fp32) / emb ([91, d], `dtype`); with w_out != NULL the same launch writes W_pad [d, Kp] from the
 *                  [d, d + 1031] weight w.  Labels must lie in [0, 91) (caller's contract); an out-of-range label gives a zero
 *                  row and, when status != NULL, sets *status |= 1 on the device.
 * imt_relu_dropout     : y <- dropout(relu(y)) in place, [rows, d] contiguous, element index r * d + c (the other dropout sites' hash).
 * imt_relu_dropout_bwd : dz = dy * (y > 0) * keep(seed, r * d + c) / (1 - p); y is the forward's output.
 * imt_obj_fold_w       : grad[n, k] += dw_pad[n, k] for k < d + 1031 (dw_pad = fp32 [d, Kp] TN product dz^T X).
 * imt_obj_embed_grad   : grad[l, :] += sum over rows with labels[r] == l of dx[r, :], l = 1 .. 90, in row order (deterministic,
 *                        no atomics); dx = [R, >= d] with leading dimension ldx (dz W_pad[:, :d]); label 0 gets nothing.
 * imt_gated_mix_bwd    : backward of imt_gated_mix (s = sigmoid(gate + 1e-7), out = s a + (1 - s) b; src/image_model.py:362-366,
 *                        src/seq_gen.py:177-180): da = s dy, db = (1 - s) dy, dgate[c] += sum_r dy (a - b) s (1 - s) into fp32.
 *                        Two stages in a fixed order: IMT_GATED_MIX_BWD_PARTS row ranges -> partial_ws [PARTS, d] fp32, then
 *                        one fold; two identical calls give bit-identical dgate. */
#define IMT_OBJ_FEAT_DIM 1024
#define IMT_OBJ_LABELS 91
#define IMT_GATED_MIX_BWD_PARTS 64
int imt_obj_rows(int feat_dtype, int dtype, const int64_t* labels, const void* feats, const float* boxes, const void* emb,
                 const void* w, void* x_out, void* w_out, int64_t R, int d, int Kp, int* status, void* stream);
int imt_relu_dropout(int dtype, void* y, int64_t rows, int d, float dropout_p, uint64_t dropout_seed, void* stream);
int imt_relu_dropout_bwd(int dtype, const void* dy, const void* y, void* dz, int64_t rows, int d, float dropout_p,
                         uint64_t dropout_seed, void* stream);
int imt_obj_fold_w(const float* dw_pad, float* grad, int d, int Kp, void* stream);
int imt_obj_embed_grad(int dtype, const int64_t* labels, const void* dx, int64_t ldx, float* grad, int64_t R, int d,
                       void* stream);
int imt_gated_mix_bwd(int dtype, const void* dy, const void* a, const void* b, const void* gate, void* da, void* db,
                      float* dgate, float* partial_ws, int64_t rows, int d, void* stream);

/* ------------------------------------------------------------------ contrastive tail of ImageMassSeq2Seq
 * src/image_model.py:240-263.  Three tensors (caption states, negative-sample states, image regions) are pooled to unit vectors
 * by a learned one-vector attention, then the images are scored against every text vector.
 * imt_attn_pool_fwd (:240-243 / :245-248 / :252-253 and the normalisation :255-258), one workgroup per sentence of
 *   x [rows, S, d] (`dtype`, contiguous): score_s = x_s . w + b (w [d], b [1] in `dtype`); where mask ([rows, S] bytes, NULL = no
 *   mask) is 0 the score is set to exactly -10000 (masked_fill: an all-masked sentence pools to the plain average);
 *   p = softmax_s(score); v = sum_s p_s x_s; u = v / (|v|_2 + 1e-4).  Outputs, all fp32: u [rows, d], and for the backward
 *   probs [rows, S] and norm [rows] = |v|_2.  Softmax statistics and every sum are fp32.
 * imt_attn_pool_plan: how often a sentence is read from memory -- 1: it stays in LDS after the score pass (its S * d elements
 *   fit beside the per-position arrays in IMT_POOL_LDS_BYTES), 2: the weighted sum reads it a second time.  Never more.  The
 *   backward follows the same plan.  IMT_ERR_BAD_ARG for a shape the kernels do not take (below).
 * imt_attn_pool_bwd: du [rows, d] fp32 (times du_scale[0] when that device scalar is given) -> dx [rows, S, d] in `dtype`
 *   (OVERWRITTEN), and dw [d] / db [1] ACCUMULATED into fp32 (the flat gradient buffer).  Per-sentence partial sums go to ws
 *   (rows * d + rows floats) and a second launch adds them in sentence order: no float atomics, two identical calls give
 *   bit-identical dw / db.
 * imt_contrastive (:260-263): img [B, d], txt [N, d] fp32 unit vectors, txt row i < B belonging to image i;
 *   C = img txt^T, loss[0] = sum_i (log(sum_j exp C_ij + 1e-4) - (C_ii + 1e-4)) / B, and d loss / d img, d loss / d txt
 *   (OVERWRITTEN, fp32).  ws: B * N + B floats.  Fixed summation order throughout.
 * Refused before any launch with IMT_ERR_BAD_ARG: a NULL tensor, S < 1, S > IMT_POOL_MAX_S, d not a multiple of 4 (the vector
 * width) or above IMT_POOL_MAX_D, N < B, N > IMT_CONTRASTIVE_MAX_N. */
#define IMT_POOL_MAX_S 4096
#define IMT_POOL_MAX_D 1024
#define IMT_POOL_LDS_BYTES 65536
#define IMT_CONTRASTIVE_MAX_N 4096
int imt_attn_pool_plan(int dtype, int S, int d);
int imt_attn_pool_fwd(int dtype, const void* x, const void* w, const void* b, const uint8_t* mask, float* u, float* probs,
                      float* norm, int64_t rows, int S, int d, void* stream);
int imt_attn_pool_bwd(int dtype, const void* x, const void* w, const uint8_t* mask, const float* u, const float* probs,
                      const float* norm, const float* du, const float* du_scale, void* dx, float* dw, float* db, float* ws,
                      int64_t rows, int S, int d, void* stream);
int imt_contrastive(const float* img, const float* txt, float* loss, float* d_img, float* d_txt, float* ws, int B, int N, int d,
                    void* stream);

/* ------------------------------------------------------------------ tail of Caption2Image (src/image_model.py:430-438) and
 * its loss (src/train_txt2image.py:67).
 * imt_sent_pool_fwd, one workgroup per sentence of x [rows, S, d] (`dtype`, contiguous): xd = dropout(x), the keep decision of an
 *   element being the one imt_add_rows_dropout makes for that element of the flattened [rows * S, d] tensor under the same seed
 *   (dropout_p == 0: nothing is drawn); score_s = xd_s . w + b (w [d], b [1] in `dtype`), set to exactly -10000 where mask
 *   ([rows, S] bytes, NULL = no mask) is 0; p = softmax_s(score); v = sum_s p_s xd_s.  No normalisation.  Outputs: v [rows, d] in
 *   `dtype` (it feeds a GEMM) and probs [rows, S] fp32.  Reads x once or twice as imt_attn_pool_plan says; every sum is fp32 in a
 *   fixed order.
 * imt_sent_pool_bwd: dv [rows, d] in `dtype` and the saved probs -> dx [rows, S, d] in `dtype` (OVERWRITTEN; the dropout mask is
 *   regenerated from the seed), and dw [d] / db [1] ACCUMULATED into fp32 through ws (rows * d + rows floats) and a second launch
 *   that adds the per-sentence partials in sentence order: two identical calls give bit-identical results.
 * imt_l2_dist: pred, target [B, n] in `dtype` (contiguous); loss[0] = sqrt(sum (pred - target)^2) / B in fp32 and
 *   dpred = (pred - target) / (sqrt(sum) B) in `dtype`, all zeros when the sum is 0.  ws: IMT_L2_DIST_PARTS floats (per-workgroup
 *   partial sums, added in index order).
 * Refused before any launch with IMT_ERR_BAD_ARG: a NULL tensor, a dtype other than IMT_F32 / IMT_BF16, S < 1, S > IMT_POOL_MAX_S,
 * d not a multiple of 4 or above IMT_POOL_MAX_D, dropout_p outside [0, 1), n not a positive multiple of 4, B < 1.  rows == 0
 * returns IMT_OK without a launch. */
#define IMT_L2_DIST_PARTS 256
int imt_sent_pool_fwd(int dtype, const void* x, const void* w, const void* b, const uint8_t* mask, void* v, float* probs,
                      int64_t rows, int S, int d, float dropout_p, uint64_t dropout_seed, void* stream);
int imt_sent_pool_bwd(int dtype, const void* x, const void* w, const uint8_t* mask, const float* probs, const void* dv, void* dx,
                      float* dw, float* db, float* ws, int64_t rows, int S, int d, float dropout_p, uint64_t dropout_seed,
                      void* stream);
int imt_l2_dist(int dtype, const void* pred, const void* target, float* loss, void* dpred, float* ws, int B, int64_t n,
                void* stream);

/* ------------------------------------------------------------------ tail of SenSim (src/sen_sim.py:68-113)
 * The sentence vectors are pooled by imt_attn_pool_fwd (the same one-vector attention and the same / (norm + 1e-4)).
 * imt_sensim_loss (:94-103), the two-sided contrastive loss: scat [Ns, d] = the source negatives followed by the B sources,
 *   tcat [Nt, d] = the target negatives followed by the B targets (the reference's cat([neg, pos])), fp32 unit vectors;
 *   src_i = scat[Ns - B + i], tgt_i = tcat[Nt - B + i].  A = src tcat^T [B, Nt], M = tgt scat^T [B, Ns],
 *   D_i = sum_j exp A_ij + sum_j exp M_ij + 1e-4, loss[0] = sum_i (log D_i - (src_i . tgt_i + 1e-4)) / B.  No max is subtracted
 *   (unit vectors: every exponent lies in [-1, 1]).  The gradients come from the same call, d_scat [Ns, d] and d_tcat [Nt, d]
 *   OVERWRITTEN: with dA = exp A / (D B), dM = exp M / (D B), d_scat = dM^T tgt and its last B rows += dA tcat - tgt / B,
 *   d_tcat = dA^T src and its last B rows += dM scat - src / B.  The three multiples of tgt_i in d src_i (and of src_i in
 *   d tgt_i) nearly cancel when a pair dominates its denominator; they are added as one coefficient -R_i / (D_i B), R_i = D_i
 *   without the pair's own two terms, summed separately, so no accuracy is lost there.  Two launches: one workgroup per pair writes dA, dM and the two
 *   row sums to ws, then one workgroup per row of scat and tcat forms the column sums and adds the row sum of its pair -- one
 *   writer per output row, fixed summation order, no float atomics: two identical calls give identical bits.
 *   ws: B * (Ns + Nt) + 2 * B * d + B floats.  Without negatives the reference's loss is one-sided (:105-108): that is
 *   imt_contrastive with N = B.
 * imt_pair_dot (:112): out_r = a_r . b_r over fp32 [rows, d]; imt_pair_dot_bwd: da_r = g_r b_r, db_r = g_r a_r (OVERWRITTEN).
 * Refused before any launch with IMT_ERR_BAD_ARG: a NULL tensor, B < 1, Ns < B, Nt < B, Ns or Nt above IMT_CONTRASTIVE_MAX_N,
 * rows outside [0, 2^31), d not a positive multiple of 4 or above IMT_POOL_MAX_D.  rows == 0 returns IMT_OK without a launch. */
int imt_sensim_loss(const float* scat, const float* tcat, float* loss, float* d_scat, float* d_tcat, float* ws, int B, int Ns,
                    int Nt, int d, void* stream);
int imt_pair_dot(const float* a, const float* b, float* out, int64_t rows, int d, void* stream);
int imt_pair_dot_bwd(const float* a, const float* b, const float* g, float* da, float* db, int64_t rows, int d, void* stream);

/* ------------------------------------------------------------------ lexical proposals of Seq2Seq (src/seq2seq.py:110-144)
 * imt_proposal_attn_fwd: x [rows, d] (`dtype`, contiguous) are decoder states, row r belonging to group g = r / rows_per_group
 *   (a sentence: rows_per_group = T - 1 in training, the beam repetition in beam search); prop [G, P] int64 are the group's
 *   proposed word ids, table [vocab, d] (`dtype`) the word embeddings; gate, gamma, beta [d] fp32.
 *   e_j = table[prop[g, j]] (pad entries take part: the reference's -10000 fill is a no-op); s_j = <x_r, e_j>; p = softmax_j(s);
 *   c = sum_j p_j e_j, or 1e-8 in every element when all of prop[g, :] == pad_idx; sg = sigmoid(gate + 1e-8);
 *   y_r = LayerNorm(sg x_r + (1 - sg) c; gamma, beta, eps), written in `dtype`.  An id outside [0, vocab) reads row 0.
 *   Saved for the backward: scores [rows, P] fp32 (the raw s) and stats [rows, 4] fp32 (softmax max and sum, LayerNorm mean and rstd).
 *   All statistics and sums are fp32; no buffer of rows * P * d elements exists in either direction.
 * imt_proposal_attn_bwd: dy [rows, d] in `dtype` -> dx [rows, d] in `dtype` (OVERWRITTEN); dgate, dgamma, dbeta [d] and
 *   dtable [vocab, d] ACCUMULATED into fp32 (the flat gradient buffer).  A table row gets the sum over every entry of prop that
 *   names it, duplicates within a group and across groups included, of sum over the group's rows of (p_j dc + ds_j x_r); pad_idx
 *   (and ids outside [0, vocab)) get nothing, so an all-pad group leaves dtable alone and reaches x only through sg dz.
 *   ws: caller-owned, 16-byte aligned, imt_proposal_attn_ws_bytes(rows, rows_per_group, P, d) bytes = p and ds [rows, P], dc
 *   [rows, d], per-workgroup partial sums ceil(rows_per_group / 8) * G * 3 * d, the gathered gradient [G, P, d] fp32 and two
 *   ints per entry of prop.  Partials are added in workgroup order, a group's rows in row order, the entries of one id in entry
 *   order by a single writer: no float atomics, two identical calls give identical bits.
 * Refused before any launch: IMT_ERR_BAD_ARG for a bad dtype, a NULL tensor, rows outside [0, 2^31) or no multiple of
 *   rows_per_group, rows_per_group < 1, P < 1, vocab < 1, a workspace that is too small or misaligned; IMT_ERR_UNSUPPORTED for d
 *   not a multiple of 4 in [4, IMT_PROPOSAL_MAX_D].  imt_proposal_attn_ws_bytes returns the same negative codes.  rows == 0
 *   returns IMT_OK without a launch. */
#define IMT_PROPOSAL_MAX_D 1024
int64_t imt_proposal_attn_ws_bytes(int64_t rows, int rows_per_group, int P, int d);
int imt_proposal_attn_fwd(int dtype, const void* x, const void* table, const int64_t* prop, const float* gate, const float* gamma,
                          const float* beta, void* y, float* scores, float* stats, int64_t rows, int rows_per_group, int P, int d,
                          int64_t vocab, int64_t pad_idx, float eps, void* stream);
int imt_proposal_attn_bwd(int dtype, const void* dy, const void* x, const void* table, const int64_t* prop, const float* gate,
                          const float* gamma, const float* scores, const float* stats, void* dx, float* dtable, float* dgate,
                          float* dgamma, float* dbeta, void* ws, int64_t ws_bytes, int64_t rows, int rows_per_group, int P, int d,
                          int64_t vocab, int64_t pad_idx, void* stream);


/* ------------------------------------------------------------------ whole encoder / decoder stacks
 * The host-side runtime that chains the kernels above for BertEncoderModel.forward (src/bert_seq2seq.py:103-144)
 * and BertDecoderModel.forward (src/bert_seq2seq.py:40-91) and their backward passes.  All tensors live in
 * caller-owned memory: `params` is the FLAT parameter buffer in the compute dtype (fp32 master, or its bf16
 * shadow), `grads` the FLAT fp32 gradient buffer with the same element offsets; `ws` is a caller-allocated
 * workspace of imt_stack_workspace_bytes() bytes that carries the saved activations from forward to backward.
 * Offsets are in ELEMENTS; -1 = absent.  q|k|v weights (and biases) of one attention block are contiguous
 * ([3d,d]) so the three projections run as one GEMM.
 */
typedef struct imt_attn_block {
  int64_t qkv_w, qkv_b; /* self.query|key|value .weight [3d,d], .bias [3d] */
  int64_t o_w, o_b;     /* output.dense */
  int64_t ln_g, ln_b;   /* output.LayerNorm */
} imt_attn_block;

typedef struct imt_layer_desc {
  imt_attn_block self_attn;
  imt_attn_block cross_attn; /* qkv_w == -1 when the layer has no crossattention */
  int64_t ff1_w, ff1_b;      /* intermediate.dense [ff,d] */
  int64_t ff2_w, ff2_b;      /* output.dense [d,ff] */
  int64_t ln2_g, ln2_b;      /* output.LayerNorm */
  int64_t cross_kv_w, cross_kv_b; /* crossattention key|value weight [2d,d] / bias [2d] when they do NOT follow the query
                                     projection in the flat buffer (-1: they sit at cross_attn.qkv_w + d*d / qkv_b + d).
                                     When these blocks of ALL layers are contiguous in layer order ([L*2d, d], [L*2d]),
                                     the runtime projects the encoder states for every layer with ONE GEMM and forms
                                     d(encoder states) / dW of all layers with one GEMM each. */
} imt_layer_desc;

typedef struct imt_stack_desc {
  int32_t dtype;
  int32_t d, heads, ff, vocab, max_pos, n_types, n_layers;
  int32_t is_decoder;
  int32_t reserved;
  int64_t pad_id;
  float ln_eps, hidden_dropout, attn_dropout;
  float reserved_f;
  int64_t emb_word, emb_pos, emb_type, emb_ln_g, emb_ln_b;
  const imt_layer_desc* layers; /* HOST pointer, n_layers entries */
  const void* params;           /* device, compute dtype */
  float* grads;                 /* device, fp32 (may be NULL for inference) */
} imt_stack_desc;

typedef struct imt_stack_io {
  int32_t B, T;              /* batch, sequence length of this stack's own tokens */
  int32_t Tk;                /* decoder: encoder sequence length */
  int32_t training;          /* 1: apply dropout (seeded) */
  const int64_t* ids;        /* [B,T] */
  const int64_t* type_ids;   /* [B,T] or NULL (zeros) */
  const int64_t* pos_ids;    /* [B,T] or NULL (arange) */
  const uint8_t* key_mask;   /* self-attention key mask [B,T]: encoder attention_mask / decoder 2-D tgt mask, or NULL */
  const uint8_t* query_mask; /* decoder: tgt_mask factor of future_mask [B,T] or NULL */
  const uint8_t* mask3d;     /* decoder: arbitrary [B,T,T] tgt_attention_mask or NULL */
  int32_t causal;            /* decoder self-attention causal flag */
  int32_t reserved;
  const void* enc_states;    /* decoder: [B,Tk,d] (compute dtype) */
  const uint8_t* enc_mask;   /* decoder: encoder_attention_mask [B,Tk] or NULL (ones) */
  void* out;                 /* [B,T,d] final hidden states (compute dtype) */
  uint64_t dropout_seed;
  /* backward only */
  const void* d_out;         /* [B,T,d] gradient of `out` */
  void* d_enc_states;        /* decoder: [B,Tk,d] gradient w.r.t. enc_states, OVERWRITTEN */
  /* forward only, optional: HOST array of n_wait_events hipEvent_t (as void*, NULL entries allowed).  `stream` waits for
   * wait_events[0] before the embeddings are read and for wait_events[1 + l] before layer l: an optimizer step that is still
   * updating the parameters on another stream (segment by segment, in the order the forward needs them) then delays only
   * the layer it has not reached yet instead of the whole stack. */
  const void* const* wait_events;
  int32_t n_wait_events;
  int32_t reserved2;
} imt_stack_io;

int64_t imt_stack_workspace_bytes(const imt_stack_desc* m, int B, int T, int Tk);
int imt_stack_forward(const imt_stack_desc* m, const imt_stack_io* io, void* ws, int64_t ws_bytes, void* stream);
/* backward over layers [layer_lo, layer_hi) in reverse order (layer_hi == n_layers first); the embedding
 * backward runs when layer_lo == 0.  Splitting lets the caller launch gradient all-reduce buckets between
 * segments (RCCL on a side stream).  Parameter gradients are accumulated into m->grads.  A call that covers
 * the whole stack (layer_lo == 0, layer_hi == n_layers) runs the per-layer weight-gradient launches on the
 * library's side stream, concurrently with the next layer's input-gradient chain (joined before return). */
int imt_stack_backward(const imt_stack_desc* m, const imt_stack_io* io, void* ws, int64_t ws_bytes, int layer_lo,
                       int layer_hi, void* stream);
/* The decisions of that call about its weight-gradient launches, evaluated on the host (no GPU needed, no device call):
 * for a stack of n_layers, the range [layer_lo, layer_hi), the side stream on or off, and pairable[l] != 0 where the products
 * of layer l and as many again would take the 256 x 128 instance of the grouped launch (HOST array of n_layers).
 * records[3i .. 3i+2] for layer l = layer_hi - 1 - i: {wait_done, action, with_held}.  wait_done: the layer whose side-stream
 * launch must be over before layer l writes its scratch set (l + 4: same set), or -1.  action: the products of layer l are
 * held for the layer below, or launched on the main or the side stream -- together with those of layer with_held (or -1).
 * *join_done (nullable): the layer whose side-stream launch the call waits for before it returns, or -1. */
#define IMT_DW_HOLD 0
#define IMT_DW_FLUSH_MAIN 1
#define IMT_DW_FLUSH_SIDE 2
int imt_stack_dw_schedule(int n_layers, int layer_lo, int layer_hi, int side_stream, const int* pairable, int* records,
                          int* join_done);

/* ------------------------------------------------------------------ incremental decoding + beam search
 * Replaces the per-step work of BeamDecoder.forward (src/seq_gen.py:131-227).  The reference re-runs the decoder
 * on the whole prefix every step (:164-166) and re-projects the encoder states to cross K/V in every layer of
 * every step; here each step processes ONE new position per hypothesis against
 *   - a self-attention cache  [n_layers][r_max][t_max][3d]  (q|k|v of every position, written in place by the
 *     fused QKV GEMM), addressed through a slot table so that beam re-ordering never copies the cache:
 *     slots[r, j] = cache row that holds position j of hypothesis r (its ancestor at the time j was decoded);
 *   - cross-attention K/V     [n_layers][B][Tk][2d]  projected once per sentence by imt_decode_begin and shared by
 *     the `rep` hypotheses of a sentence (row r reads sentence r / rep).
 * With the causal mask of BertDecoderModel (src/bert_seq2seq.py:69-71) the cached keys/values equal the
 * recomputed ones, so the last-position hidden state is the reference's `decoder_states[:, -1, :]` (:191).
 */
typedef struct imt_attn_decode_args {
  int32_t dtype;
  int32_t R, H, head_dim; /* hypotheses, heads, 32|64 */
  int32_t n_keys;         /* keys attended (self: pos+1; cross: Tk) */
  int32_t rep;            /* hypotheses per sentence (mask row and, without slots, K/V row = r / rep) */
  const void* Q; int64_t ldq;        /* query of hypothesis r at Q + r*ldq (+ h*head_dim) */
  const void* K; const void* V;      /* element (row, j) at base + row*ld_row + j*ld_pos (+ h*head_dim) */
  int64_t ld_row, ld_pos;
  const int32_t* slots; int64_t ld_slots; /* [R, >= n_keys] or NULL (row = r / rep) */
  const uint8_t* key_mask; int64_t ld_mask; /* [R/rep, n_keys]: (1-m)*-10000 added to the scaled score; nullable */
  void* O; int64_t ldo;
  float scale;
  int32_t reserved;
} imt_attn_decode_args;
int imt_attention_decode(const imt_attn_decode_args* a, void* stream);

typedef struct imt_decode_io {
  int32_t R;               /* hypothesis rows this step (B at the first step, B*beam afterwards) */
  int32_t rep;             /* rows per source sentence */
  int32_t pos;             /* 0-based position being decoded == number of cached positions */
  int32_t Tk;              /* encoder length */
  int32_t t_max, r_max;    /* cache capacity: positions, rows */
  const int64_t* ids;      /* [R] newest token of every hypothesis */
  const int64_t* type_ids; /* [R] or NULL (zeros) */
  const int64_t* pos_ids;  /* [R] position-embedding index (normally == pos) */
  const int32_t* slots;    /* [R, t_max] slot table, slots[r, pos] == r ; NULL: every row reads its own cache row */
  const uint8_t* enc_mask; /* [R/rep, Tk] encoder_attention_mask or NULL (ones) */
  void* self_cache;        /* imt_decode_self_cache_bytes() */
  const void* cross_kv;    /* imt_decode_cross_bytes(), filled by imt_decode_begin */
  void* out;               /* [R, d] last-position hidden states (compute dtype) */
} imt_decode_io;
int64_t imt_decode_workspace_bytes(const imt_stack_desc* m, int r_max);
int64_t imt_decode_self_cache_bytes(const imt_stack_desc* m, int r_max, int t_max);
int64_t imt_decode_cross_bytes(const imt_stack_desc* m, int B, int Tk);
/* cross K|V of every decoder layer from the encoder states [B,Tk,d] (one GEMM per layer). */
int imt_decode_begin(const imt_stack_desc* m, const void* enc_states, int B, int Tk, void* cross_kv, void* stream);
int imt_decode_step(const imt_stack_desc* m, const imt_decode_io* io, void* ws, int64_t ws_bytes, void* stream);
/* bf16 stacks with hidden size 512 or 768 in heads of 64 run a step as ONE launch whose workgroups meet at grid-wide barriers with
 * bounded waits (csrc/decode_fused.hip; IMT_DECODE_FUSED=0: the launch-per-operator chain).  A wait that runs out abandons
 * the launch and sets a status word in `ws` (cleared by the step with pos == 0).  imt_decode_check synchronises `stream`
 * and returns IMT_ERR_LAUNCH if any step since then was abandoned, IMT_OK otherwise (and always for other stacks):
 * call it once when a search ends, before trusting its tokens. */
int imt_decode_check(const imt_stack_desc* m, int r_max, const void* ws, void* stream);

/* One beam-search step on device (src/seq_gen.py:193-227): log-softmax of the [B*rep, V] logits, the EOS /
 * length-limit zeroing (:194-196), length-penalised scores (:197-200, pow((len+6)/6, ratio)), top-`beam` over the
 * rep*V continuations of each sentence with ties broken by the LOWEST flat index (torch.topk leaves it unspecified),
 * the reference's PAD overwrites (:205-212, including that finished/over-limit slots take beam 0 as parent because
 * the overwritten flat index is divided by V, :216 with floor division), and the bookkeeping (:214-227): token
 * history, hypothesis sizes, scores, EOS flags, and the slot table of the self-attention cache.
 * Row r of the inputs is hypothesis (r / rep, r % rep); outputs have B*beam rows.  `step` is the reference's loop
 * index i (>= 1): inputs hold i tokens, outputs i+1.  eos_count[step] += number of output hypotheses containing EOS.
 */
typedef struct imt_beam_args {
  int32_t B, beam, rep, V;
  int32_t step, t_max;
  const float* logits; int64_t ld; /* [B*rep, V] fp32 */
  const float* scores_in;          /* [B*rep] */
  const float* sizes_in;           /* [B*rep] (ignored when beam == 1) */
  const uint8_t* eos_in;           /* [B*rep] hypothesis already contains EOS */
  const int64_t* max_lens;         /* [B] */
  const int64_t* hist_in;          /* [B*rep, t_max] */
  const int32_t* slots_in;         /* [B*rep, t_max] or NULL */
  float len_penalty_ratio;
  int32_t reserved;
  int64_t pad_idx, eos;
  float* cand_scores; int32_t* cand_idx; /* workspace [B*rep, beam] each */
  float* scores_out; float* sizes_out; uint8_t* eos_out; /* [B*beam] */
  int64_t* hist_out;               /* [B*beam, t_max] */
  int32_t* slots_out;              /* [B*beam, t_max] or NULL */
  int32_t* parent_out;             /* [B*beam] input row each output hypothesis extends */
  int64_t* tokens_out;             /* [B*beam] appended token */
  int32_t* eos_count;              /* [t_max] (pre-zeroed by the caller) or NULL */
} imt_beam_args;
int imt_beam_step(const imt_beam_args* a, void* stream);

/* One SAMPLING step on device: the counterpart of imt_beam_step for drawing from the model instead of searching it (the
 * reference has no such mode).  Output row r' = b*n + k extends input row p = b*rep + (rep == 1 ? 0 : k): every hypothesis
 * keeps its own parent, n samples per sentence run side by side.  With x = logits[p, :V]:
 *   masked rows   eos_in[p], or step > 1 and max_lens[b] < step + 1 (the rule of imt_beam_step): token pad_idx, score unchanged,
 *                 eos_out = eos_in[p];
 *   kept set K    the first `topk` indices by (x descending, index ascending) -- ties at the k-th place go to the lowest
 *                 indices -- or all of [0, V) when topk <= 0 or topk >= V;
 *   noise         u(v) = max(counter_uniform(seed, stream = step, index = r'*V + v), 2^-25) (the generator of imt_mass_mask,
 *                 indexed by the OUTPUT row: the n children of one parent at step 1 draw differently), g(v) = -log(-log(u(v)));
 *   token         argmax over v in K of x[v] / temperature + g(v) by (value descending, index ascending): Gumbel-max, an
 *                 exact draw from softmax(x / temperature) restricted to K;
 *   score         scores_in[p] + x[token] - logsumexp(x): the MODEL's log-probability (temperature 1, whole vocabulary);
 *   bookkeeping   history, eos_out, slots_out, parent_out, tokens_out, eos_count[step]: commit_hypothesis / copy_history of
 *                 csrc/search_step.hpp, the functions imt_beam_step calls.
 * Deterministic: no floating-point atomics, nothing crosses workgroups; two calls on the same input give the same bits. */
typedef struct imt_sample_args {
  int32_t B, n, rep, V;            /* n samples per sentence (1..32); rep = 1 (only at step 1) or n */
  int32_t step, t_max;
  const float* logits; int64_t ld; /* [B*rep, V] fp32, rows ld apart; columns [V, ld) are never read */
  const float* scores_in;          /* [B*rep] */
  const uint8_t* eos_in;           /* [B*rep] */
  const int64_t* max_lens;         /* [B] */
  const int64_t* hist_in;          /* [B*rep, t_max] */
  const int32_t* slots_in;         /* [B*rep, t_max] or NULL */
  float temperature;               /* > 0, finite */
  int32_t topk;                    /* <= 0 or >= V: the whole vocabulary */
  uint64_t seed;
  int64_t pad_idx, eos;
  float* scores_out; uint8_t* eos_out; /* [B*n] */
  int64_t* hist_out;               /* [B*n, t_max] */
  int32_t* slots_out;              /* [B*n, t_max] or NULL */
  int32_t* parent_out;             /* [B*n] */
  int64_t* tokens_out;             /* [B*n] */
  int32_t* eos_count;              /* [t_max] (pre-zeroed by the caller) or NULL */
} imt_sample_args;
int imt_sample_step(const imt_sample_args* a, void* stream);

/* ------------------------------------------------------------------ MASS batch construction on device
 * mass_mask / mass_unmask of src/utils.py:41-82.  Per sentence (row): a contiguous span of int(pad_index/2) tokens
 * starting at `first` is hidden from the encoder, where first = 1 (20%), the bound ceil(pad - (1-p)*pad) (20%) or
 * uniform in [2, bound] (60%) (src/utils.py:52-60); the decoder input `to_recover` is the span shifted right by one
 * with its ORIGINAL positions; hidden tokens become <mask> (80%), a random non-special id (10%) or stay (10%).
 * The random draws are counter-based on (seed, stream, index) -- NOT Python's generator: the same statistical
 * procedure, reproducible on device.  The span starts are drawn by the CALLER (streams 0 and 1 of the generator, index =
 * row; utils.mass_span_starts restates the rule on the host without a device read) and handed in as `first`, because a
 * span is clipped at the row's end like a Python slice and every size below follows from the clipped span:
 *   f[r]           = first[r] clamped to [1, width]       (a start below 1 is read as 1, one past the row as width)
 *   len[r]         = int(pad_indices[r]/2) clamped to [0, width]
 *   hidden[r]      = min(f[r] + len[r], width) - f[r]     (>= 0 after the clamps)
 *   row_offsets[r] = sum_{q<r} hidden[q]                  (exclusive prefix sum; total = number of targets)
 *   recover_width  = max_r hidden[r] + 1
 * The kernel applies the same two clamps, writes hidden[r] targets for row r and nothing else into `targets`: the sizes
 * and the writes come from the same `first` (utils.mass_span_sizes is the caller's side of this arithmetic).
 * src_text is modified in place (like the reference); imt_mass_unmask restores it from `targets`.
 */
typedef struct imt_mass_args {
  int32_t n_rows, width, recover_width;
  int32_t n_special, vocab;  /* replacement ids are drawn from [n_special, vocab) */
  float mask_prob;
  uint64_t seed;
  int64_t mask_id, pad_id;
  int64_t* src_text;            /* [n_rows, width] in/out */
  const int64_t* pad_indices;   /* [n_rows] index of the first pad token (width-1 if none) */
  const int64_t* row_offsets;   /* [n_rows] */
  const int64_t* first;         /* [n_rows] span start of every row, drawn by the caller */
  uint8_t* src_mask;            /* [n_rows, width] out: 1 on hidden positions */
  int64_t* to_recover;          /* [n_rows, recover_width] out, padded with pad_id */
  int64_t* positions;           /* [n_rows, recover_width] out, padded with width-1 */
  int64_t* targets;             /* [total] out: hidden tokens in row-major order (== the reference's mask_idx) */
} imt_mass_args;
int imt_mass_mask(const imt_mass_args* a, void* stream);
int imt_mass_unmask(int64_t* src_text, const uint8_t* src_mask, const int64_t* originals, const int64_t* row_offsets,
                    int n_rows, int width, void* stream);

/* ------------------------------------------------------------------ masked-LM batch construction on device
 * mask_text of src/utils.py:19-38 (BERT masking) in ONE launch: the Bernoulli draw per token, the 80/10/10 replacement in
 * place and the compaction of the masked positions in row-major order (the order of the reference's texts[mask]).  Nothing
 * is read back.  With p = b*width + t the flat position (uint32) and counter_uniform the generator of imt_mass_mask --
 * streams 4, 5 and 6 here, so a seed shared with imt_mass_mask never reuses its streams 0-3:
 *   selected(p) = pads[b, t] != 0 && (mask_eos || texts[p] != eos_id) && counter_uniform(seed, 4, p) < mask_prob  (float32)
 *   mask[p]     = selected(p), written at EVERY position
 *   the k-th selected position in row-major order: idx[k] = p, targets[k] = the ORIGINAL id; count[0] = how many
 *   replacement at a selected position, u = counter_uniform(seed, 5, p):
 *     u < 0.8f   <mask>
 *     u < 0.9f   n_special + min((int)(counter_uniform(seed, 6, p) * (float)(vocab - n_special)), vocab - n_special - 1)
 *     otherwise  the id stays
 * idx / targets need room for n_rows*width entries; entries at and beyond count[0] are unspecified.  n_rows*width < 2^31.
 * utils.mask_text_count restates selected(p) on the host, so a training step sizes its buffers without reading count.
 * texts is modified in place (like the reference); a scatter of targets at idx restores it.
 */
typedef struct imt_mlm_args {
  int32_t n_rows, width;
  int32_t n_special, vocab;  /* replacement ids are drawn from [n_special, vocab) */
  int32_t mask_eos;          /* 0: a token equal to eos_id is never selected */
  float mask_prob;           /* 0 < p < 1 */
  uint64_t seed;
  int64_t mask_id, eos_id;
  int64_t* texts;            /* [n_rows, width] contiguous, in/out */
  const uint8_t* pads;       /* [n_rows, width], row stride ld_pads: 1 = a real token */
  int64_t ld_pads;
  uint8_t* mask;             /* [n_rows, width] out */
  int32_t* idx;              /* [n_rows*width] out: flat positions of the selected tokens */
  int64_t* targets;          /* [n_rows*width] out: their original ids */
  int32_t* count;            /* [1] out */
} imt_mlm_args;
int imt_mlm_mask(const imt_mlm_args* a, void* stream);

/* Non-pad target selection (src/seq2seq.py:175-177 `flat[tgt_mask[:, 1:]]`, train_image_mt.py:253-256 targets):
 * idx[k] = flat position b*T1 + t of the k-th set mask[b, col0 + t] (row-major order), targets[k] = ids[b, col0 + t],
 * count[0] = number selected.  idx / targets need room for B*T1 entries. */
int imt_select_plan(const uint8_t* mask, int64_t ld_mask, const int64_t* ids, int64_t ld_ids, int B, int T1, int col0,
                    int32_t* idx, int64_t* targets, int32_t* count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMT_HIP_H */
