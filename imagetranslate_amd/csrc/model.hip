// Host-side runtime: chains the kernels for a whole BERT encoder / cross-attending decoder stack
// (BertEncoderModel.forward src/bert_seq2seq.py:103-144, BertDecoderModel.forward :40-91, with the HF-BERT
// 2.9.0 layer semantics restated in SURVEY section 8: post-LN, erf-GELU, additive -10000 masks) and their
// backward passes.  Pure enqueue: no allocation, no synchronisation; every launch goes to the caller's stream
// so the whole forward/backward is capturable in a hipGraph.  Activations needed by backward are kept in the
// caller-owned workspace, carved identically by forward and backward.
#include "common.hpp"
#include "decode_fused.hpp"

namespace {

struct Carver {
  char* base; int64_t off;
  explicit Carver(void* b) : base(reinterpret_cast<char*>(b)), off(0) {}
  void* take(int64_t bytes) { void* p = base ? base + off : nullptr; off += (bytes + 255) & ~(int64_t)255; return p; }
};

// what dense + residual + LayerNorm leaves behind: the sum [N,d] (LN input), the row statistics, the LN output [N,d]
struct LnWs { void* pre_ln; float* mean; float* rstd; void* out; };
struct AttnWs {  // one attention block (self or cross)
  void* qkv;     // self: [N,3d] ; cross: q [N,d] then kv [Nk,2d]
  void* kv;      // cross only
  int64_t kv_ld; // leading dimension of kv (2d, or L*2d when the projections of all layers are one buffer)
  void* ctx;     // [N,d]
  float* lse;    // [B,H,T]
  LnWs ln;
};
struct LayerWs {
  AttnWs self_attn, cross;
  void* z; void* h;  // [N,ff]
  LnWs ln2;          // ln2.out [N,d] is the layer's output
};
// Backward scratch of one layer.  Every dy operand of a weight-gradient GEMM keeps its own buffer until the end of the layer,
// because all dW GEMMs of a layer are deferred into ONE grouped launch (imt_gemm_grouped_tn).
struct Scratch {
  void* dpre[3]; void* ddrop[3];     // [N,d]  LN-backward outputs of the FFN / cross / self blocks (residual / dense path)
  void* d_ctx; void* d_ff; void* d_qkv;  // [N,d], [N,ff], [N,3d]
  void* d_q; void* d_kv;             // [N,d] cross-attention query gradient, [Nk,2d]
};
// It exists FOUR times (layer l uses scr[l % 4], handed down by imt_stack_backward's layer loop): the weight-gradient launch
// of the layer pair (l + 1, l) reads both layers' dy operands and may run on the side stream while layers l - 1 and l - 2
// already write their own (DwPlan).
constexpr int N_SCRATCH = 4;
struct StackWs {
  void* emb_sum; float* emb_mean; float* emb_rstd; void* x0;
  LayerWs* layers;  // host array (carved on the stack of the caller)
  void* d_run;                       // [N,d]  running gradient w.r.t. the current block output
  Scratch scr[N_SCRATCH];
  void* d_emb;                       // [N,d]  gradient w.r.t. the embedding sum (its own buffer: see imt_stack_backward)
  void* kv_all; void* d_kv_all;      // [Nk, L*2d] when the cross-attention key|value projections are batched
  float* delta;                      // [B,H,T]
  float* ln_partial;                 // [3 * layers + 1][IMT_LN_BWD_WS_FLOATS(d)]: per-XCD dgamma|dbeta partial sums of every
                                     // LayerNorm site (layer l: 3l = FFN, 3l+1 = cross, 3l+2 = self; last = embeddings)
  float* ln_site(int site, int d) const { return ln_partial + (int64_t)site * IMT_LN_BWD_WS_FLOATS(d); }
  void* splitk; int64_t splitk_bytes; // fp32 slabs of imt_gemm's split-K mode (few output tiles: captioning / short batches); one
                                     // product at a time on the main stream, the grouped weight gradients never use it
  int64_t bytes;
};

constexpr int MAX_LAYERS = 64;

// crossattention key|value weight / bias offsets of a layer (imt_layer_desc.cross_kv_*)
int64_t kv_w_off(const imt_stack_desc* m, const imt_layer_desc& p) { return p.cross_kv_w >= 0 ? p.cross_kv_w : p.cross_attn.qkv_w + (int64_t)m->d * m->d; }
int64_t kv_b_off(const imt_stack_desc* m, const imt_layer_desc& p) { return p.cross_kv_b >= 0 ? p.cross_kv_b : p.cross_attn.qkv_b + m->d; }
// all layers' key|value projections contiguous in layer order -> one [L*2d, d] weight: ONE GEMM projects the encoder
// states for every layer (forward), one forms d(encoder states) and one the weight gradients (backward)
bool cross_kv_batched(const imt_stack_desc* m) {
  if (!m->is_decoder || m->n_layers < 2) return false;
  const int64_t d = m->d;
  for (int l = 0; l < m->n_layers; ++l) {
    const imt_layer_desc& p = m->layers[l];
    if (p.cross_attn.qkv_w < 0 || p.cross_kv_w < 0 || p.cross_kv_b < 0) return false;
    if (p.cross_kv_w != m->layers[0].cross_kv_w + (int64_t)l * 2 * d * d) return false;
    if (p.cross_kv_b != m->layers[0].cross_kv_b + (int64_t)l * 2 * d) return false;
  }
  return true;
}

void carve(const imt_stack_desc* m, int B, int T, int Tk, void* ws, StackWs& w, LayerWs* layers) {
  Carver c(ws);
  const int64_t N = (int64_t)B * T, Nk = (int64_t)B * Tk, d = m->d, ff = m->ff, es = imt_dtype_bytes(m->dtype);
  w.emb_sum = c.take(N * d * es); w.emb_mean = (float*)c.take(N * 4); w.emb_rstd = (float*)c.take(N * 4);
  w.x0 = c.take(N * d * es); w.layers = layers;
  const bool batched = cross_kv_batched(m);
  const int64_t L2d = (int64_t)m->n_layers * 2 * d;
  auto take_ln = [&](LnWs& o) { o.pre_ln = c.take(N * d * es); o.mean = (float*)c.take(N * 4); o.rstd = (float*)c.take(N * 4); o.out = c.take(N * d * es); };
  w.kv_all = w.d_kv_all = nullptr;
  if (batched) { w.kv_all = c.take(Nk * L2d * es); w.d_kv_all = c.take(Nk * L2d * es); }
  for (int l = 0; l < m->n_layers; ++l) {
    LayerWs& L = layers[l]; AttnWs& s = L.self_attn;
    s.qkv = c.take(N * 3 * d * es); s.kv = nullptr; s.ctx = c.take(N * d * es);
    s.lse = (float*)c.take((int64_t)B * m->heads * T * 4);
    take_ln(s.ln);
    AttnWs& x = L.cross; memset(&x, 0, sizeof(x));
    if (m->is_decoder && m->layers[l].cross_attn.qkv_w >= 0) {
      x.qkv = c.take(N * d * es); x.ctx = c.take(N * d * es);
      if (batched) { x.kv = w.kv_all ? (void*)((char*)w.kv_all + (int64_t)l * 2 * d * es) : nullptr; x.kv_ld = L2d; }
      else { x.kv = c.take(Nk * 2 * d * es); x.kv_ld = 2 * d; }
      x.lse = (float*)c.take((int64_t)B * m->heads * T * 4);
      take_ln(x.ln);
    }
    L.z = c.take(N * ff * es); L.h = c.take(N * ff * es);
    take_ln(L.ln2);
  }
  w.d_run = c.take(N * d * es);
  for (Scratch& z : w.scr) {
    for (int i = 0; i < 3; ++i) { z.dpre[i] = c.take(N * d * es); z.ddrop[i] = c.take(N * d * es); }
    z.d_ctx = c.take(N * d * es); z.d_ff = c.take(N * ff * es); z.d_qkv = c.take(N * 3 * d * es); z.d_q = c.take(N * d * es);
    z.d_kv = c.take((Nk > 0 ? Nk : 1) * 2 * d * es);
  }
  w.d_emb = c.take(N * d * es); w.delta = (float*)c.take((int64_t)B * m->heads * T * 4);
  w.ln_partial = (float*)c.take((int64_t)(3 * m->n_layers + 1) * IMT_LN_BWD_WS_FLOATS(d) * 4);
  // split-K slabs: only batches whose products have <= 128 output tiles can take that path (imt_gemm: splitk_choice)
  w.splitk_bytes = ((N + 127) / 128) * ((d + 127) / 128) <= 128 ? imt_gemm_splitk_ws_bytes() : 0;
  w.splitk = w.splitk_bytes ? c.take(w.splitk_bytes) : nullptr;
  w.bytes = c.off;
}

struct MaskSet { const uint8_t* key; const uint8_t* query; const uint8_t* m3d; int causal; };

// What every helper below needs for one call: the stack, the stream, and (training stacks: batch()) the batch.
struct Ctx {
  const imt_stack_desc* m; hipStream_t st; int dtype; int64_t es;
  void* splitk; int64_t splitk_bytes;  // imt_gemm_args.splitk_ws of every main-stream product
  int B = 0, T = 0, Tk = 0, N = 0;     // N = B * T rows (incremental decoding: the hypotheses of the step)
  uint64_t seed = 0; float hp = 0.f, ap = 0.f;  // dropout seed; hidden / attention dropout rates of this call (0 unless training)
  MaskSet self_ms{}, cross_ms{};
  Ctx(const imt_stack_desc* m_, void* stream, void* sk = nullptr, int64_t sk_bytes = 0, const imt_stack_io* io = nullptr)
      : m(m_), st((hipStream_t)stream), dtype(m_->dtype), es(imt_dtype_bytes(m_->dtype)), splitk(sk), splitk_bytes(sk_bytes) { if (io) batch(io); }
  void batch(const imt_stack_io* io) {
    B = io->B; T = io->T; Tk = io->Tk; N = B * T; seed = io->dropout_seed;
    hp = io->training ? m->hidden_dropout : 0.f; ap = io->training ? m->attn_dropout : 0.f;
    self_ms = MaskSet{io->key_mask, io->query_mask, io->mask3d, io->causal};
    cross_ms = MaskSet{io->enc_mask, nullptr, nullptr, 0};
  }
  const char* P(int64_t off) const { return reinterpret_cast<const char*>(m->params) + off * es; }
  float* G(int64_t off) const { return m->grads + off; }
};

#define RC(x) do { int rc__ = (x); if (rc__ != IMT_OK) return rc__; } while (0)

// The one place an imt_gemm_args is zeroed and given what every product of this file shares: C[M,N] = A B in `layout`, operands
// and result in the compute dtype, no epilogue.  Callers set the rest by field name.
imt_gemm_args product(const Ctx& c, int layout, int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc) {
  imt_gemm_args a;
  memset(&a, 0, sizeof(a));
  a.dtype = c.dtype; a.layout = layout; a.M = M; a.N = N; a.K = K;
  a.A = A; a.lda = lda; a.B = B; a.ldb = ldb; a.C = C; a.ldc = ldc; a.c_dtype = c.dtype;
  a.split_k = 1; a.alpha = 1.f; a.splitk_ws = c.splitk; a.splitk_ws_bytes = c.splitk_bytes;
  return a;
}
int run(const Ctx& c, const imt_gemm_args& a) { return imt_gemm(&a, c.st); }

// y[M,N] = x[M,K] W[N,K]^T + b
imt_gemm_args linear_fwd(const Ctx& c, const void* x, int64_t ldx, int M, int K, int64_t w_off, int64_t b_off, int N, void* y, int64_t ldy) {
  imt_gemm_args a = product(c, IMT_NT, M, N, K, x, ldx, c.P(w_off), K, y, ldy);
  a.bias = b_off >= 0 ? c.P(b_off) : nullptr; a.ldaux = N; return a;
}
// dx[M,K] = dy[M,N] W[N,K]        (W stored [N,K] row-major -> NN with B = W)
imt_gemm_args linear_bwd_input(const Ctx& c, const void* dy, int64_t lddy, int M, int N, int64_t w_off, int K, void* dx, int64_t lddx) {
  imt_gemm_args a = product(c, IMT_NN, M, K, N, dy, lddy, c.P(w_off), K, dx, lddx);
  a.ldaux = K; return a;
}

// y = LayerNorm(dropout(x W^T + b) + resid)  (BertSelfOutput / BertOutput), x [c.N, K] -> [c.N, d]: imt_gemm with the residual
// epilogue + imt_layernorm_fwd, or ONE launch of the row-complete fused kernel (gemm_ln.hip).  Measured on MI355X
// (profiles/r02_gemm_ln_study.txt): the fused kernel streams the whole weight through every workgroup (32-row tiles), which
// at d = 512 costs what the LayerNorm launch saves (8192 x 512 x 512: 22.2 us against 13.8 + 8.1, C1 step 7.63 against 7.61
// ms; incremental decoding 0.92 against 0.77 ms per step: its K loop is one serial stream per workgroup) -- it wins only for
// narrow models (N <= 256: 0.5-0.7x of the pair).  IMT_GEMM_LN=0 / 1: never / whenever supported.
bool fuse_dense_ln(const Ctx& c, int N, int K) {
  static const int mode = getenv("IMT_GEMM_LN") ? atoi(getenv("IMT_GEMM_LN")) : -1;
  if (mode == 0 || !imt_gemm_bias_residual_ln_supported(c.dtype, N, K)) return false;
  if (mode == 1) return true;
  return N <= 256 && K <= 1024;
}
int dense_resid_ln(const Ctx& c, const void* x, int K, int64_t w_off, int64_t b_off, const void* resid, int64_t g_off, int64_t beta_off,
                   const LnWs& o, uint64_t seed) {
  const int M = c.N, N = c.m->d;
  const void* bias = b_off >= 0 ? c.P(b_off) : nullptr;
  if (fuse_dense_ln(c, N, K))
    return imt_gemm_bias_residual_ln(c.dtype, x, K, c.P(w_off), K, bias, resid, N, c.P(g_off), c.P(beta_off), o.pre_ln, o.out, N, o.mean,
                                     o.rstd, M, N, K, c.m->ln_eps, c.hp, seed, c.st);
  // imt_gemm with the LayerNorm of the finished rows behind it (a second launch, or the split-K epilogue launch)
  imt_gemm_args a = product(c, IMT_NT, M, N, K, x, K, c.P(w_off), K, o.pre_ln, N);
  a.bias = bias; a.resid = resid; a.ldr = N; a.dropout_p = c.hp; a.dropout_seed = seed;
  a.ln_gamma = c.P(g_off); a.ln_beta = c.P(beta_off); a.ln_out = o.out; a.ld_ln = N; a.ln_mean = o.mean; a.ln_rstd = o.rstd; a.ln_eps = c.m->ln_eps;
  return run(c, a);
}

// Weight-gradient GEMMs of one layer are collected here and issued as ONE grouped launch at the end of the layer's
// backward (dW[N,K] += dy[M,N]^T x[M,K] ; db[N] += colsum(dy), fused) -- or, where imt_gemm_grouped_tn then multiplies
// 256 x 128 tiles, those of TWO layers at the end of the second one's (hold_for_pair, DwPlan).
struct DeferredDW {
  imt_gemm_args list[16];
  int n = 0;
  // the products collected so far are one layer's: would they and the same again, the next layer's, take the 256 x 128 instance?
  bool hold_for_pair() const {
    if (n == 0 || 2 * n > 16) return false;
    imt_gemm_args two[16];
    for (int i = 0; i < n; ++i) two[i] = two[n + i] = list[i];
    return imt_gemm_grouped_tall(two, 2 * n);
  }
  void add(const Ctx& c, const void* dy, int64_t lddy, const void* x, int64_t ldx, int M, int N, int K, int64_t w_off, int64_t b_off) {
    imt_gemm_args& a = list[n++];
    a = product(c, IMT_TN, N, K, M, dy, lddy, x, ldx, c.G(w_off), K);
    a.c_dtype = IMT_F32; a.accumulate = 1;
    a.splitk_ws = nullptr; a.splitk_ws_bytes = 0;    // the slabs belong to the main-stream products
    a.a_colsum = b_off >= 0 ? c.G(b_off) : nullptr;  // dy is read once for dW and db
    // used only if the group cannot be formed (ragged token count): about one workgroup per CU via split-K
    const int tiles = imt_cdiv(N, 128) * imt_cdiv(K, 128);
    int sk = 1;
    while (sk < 8 && tiles * sk * 2 <= 256 && M / (sk * 2) >= 512) sk *= 2;
    if (M % (c.dtype == IMT_BF16 ? 64 : 32) != 0) { a.split_k = sk; a.accumulate = (sk == 1); }
  }
  int flush(hipStream_t st) { const int cnt = n; n = 0; return cnt ? imt_gemm_grouped_tn(list, cnt, st) : IMT_OK; }
};

// Side stream for the weight-gradient launches (one process drives one GPU from one thread: plain statics).
// dW of layer l only has to be complete when the stack's backward returns, and it is bound by operand traffic, while
// the dX chain of layer l-1 is a string of latency-bound launches: on two streams the hardware runs workgroups of
// both.  ready[l]: main stream has produced every dy operand of layer l.  done[l]: the side stream has finished dW(l).
struct SideQueue {
  hipStream_t st = nullptr; hipEvent_t ready[MAX_LAYERS], done[MAX_LAYERS]; bool ok = false;
  bool init() {
    if (st) return ok;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { st = (hipStream_t)1; return ok = false; }
    for (int i = 0; i < MAX_LAYERS; ++i)
      if (hipEventCreateWithFlags(&ready[i], hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&done[i], hipEventDisableTiming) != hipSuccess) return ok = false;
    return ok = true;
  }
};
SideQueue g_side;

// Where the weight-gradient launch of each layer of one imt_stack_backward call goes (layers in descending order): the
// decisions, with no HIP call, so that they can be checked without a GPU (imt_stack_dw_schedule documents the answers).
struct DwPlan {
  int lo, hi;
  bool whole, side;    // whole stack of >= 2 layers: only then layer pairs per launch and the side stream (a data-parallel run
                       // calls per layer and hands each layer's gradients to its all-reduce bucket as soon as the call returns)
  int held = -1;       // the layer whose products wait in DeferredDW for those of the layer below
  int last_side = -1;  // the call ends by waiting for done[last_side]
  DwPlan(int n_layers, int lo_, int hi_, bool side_on)
      : lo(lo_), hi(hi_), whole(lo_ == 0 && hi_ == n_layers && n_layers >= 2), side(side_on && whole) {}
  // layer l writes the scratch set layer l + 4 used: the launch that read it (done[l + 4]: that layer's own or its pair's) must
  // be over (it is, by two layers' worth of time)
  int wait_done(int l) const { return side && l + N_SCRATCH < hi ? l + N_SCRATCH : -1; }
  bool may_hold(int l) const { return whole && held < 0 && l > lo; }
  // all 4 (encoder) / 7 (decoder) products of layer l are collected (pairable: hold_for_pair()): one launch -- with those of the
  // layer above (*with_held), if this is the second layer of a pair; held back for the layer below, if it is the first of one
  int collected(int l, bool pairable, int* with_held) {
    *with_held = -1;
    if (may_hold(l) && pairable) { held = l; return IMT_DW_HOLD; }
    *with_held = held; held = -1;
    if (side) last_side = l;
    return side ? IMT_DW_FLUSH_SIDE : IMT_DW_FLUSH_MAIN;
  }
};
// ... and the half that acts on them, at three points of imt_stack_backward.  Side stream: unless IMT_DW_SIDE_STREAM=0; neither it
// nor layer pairs under the per-launch event profiler (it reports one launch per layer, and not next to a concurrent one).
struct DwSchedule {
  DwPlan plan; hipStream_t main; DeferredDW dw;
  DwSchedule(int n_layers, int lo, int hi, hipStream_t st) : plan(n_layers, lo, hi, true), main(st) {
    static const bool env = !(getenv("IMT_DW_SIDE_STREAM") && atoi(getenv("IMT_DW_SIDE_STREAM")) == 0);
    plan.side = env && !imt_prof_enabled() && plan.whole && g_side.init();
  }
  void before_scratch(int l) const { if (plan.wait_done(l) >= 0) (void)hipStreamWaitEvent(main, g_side.done[plan.wait_done(l)], 0); }
  int collected(int l) {
    int with_held;
    const int action = plan.collected(l, plan.may_hold(l) && !imt_prof_enabled() && dw.hold_for_pair(), &with_held);
    if (action != IMT_DW_FLUSH_SIDE) return action == IMT_DW_HOLD ? IMT_OK : dw.flush(main);
    (void)hipEventRecord(g_side.ready[l], main);
    (void)hipStreamWaitEvent(g_side.st, g_side.ready[l], 0);
    RC(dw.flush(g_side.st));
    (void)hipEventRecord(g_side.done[l], g_side.st);
    if (with_held >= 0) (void)hipEventRecord(g_side.done[with_held], g_side.st);
    return IMT_OK;
  }
  // the gradients are complete, in main-stream order, when the call returns (the encoder stack accumulates into the
  // self-attention weights it shares with the decoder; the optimizer / all-reduce follow on the main stream)
  void join() const { if (plan.last_side >= 0) (void)hipStreamWaitEvent(main, g_side.done[plan.last_side], 0); }
};

uint64_t site_seed(uint64_t base, int layer, int site) { return base + 0x9E3779B97F4A7C15ull * (uint64_t)(layer * 16 + site + 1); }

inline const char* offp(const void* p, int64_t elems, int64_t es) { return reinterpret_cast<const char*>(p) + elems * es; }
inline char* offp(void* p, int64_t elems, int64_t es) { return reinterpret_cast<char*>(p) + elems * es; }

// What only a cross-attention block needs; self-attention passes none (nullptr).  Its LayerNorm slot is 1 and its dropout
// sites start at 4 (self: slot 2, sites from 0).
struct Cross {
  const void* src;       // encoder states [B*Tk, d]
  int64_t kv_w, kv_b;    // key|value weight / bias offsets
  bool kv_ready;         // forward: the key|value projections of all layers were formed by one GEMM before the layer loop
  void* d_src; int accumulate;  // backward: gradient w.r.t. src (nullable), added to what the layers above left there -- or,
  void* d_kv_batched;    // batched projections: this layer's column block of d_kv_all (d(src) is formed after the layer loop)
};
Cross cross_of(const Ctx& c, const imt_stack_io* io, const StackWs& w, int l, bool batched) {
  Cross x;
  x.src = io->enc_states; x.kv_w = kv_w_off(c.m, c.m->layers[l]); x.kv_b = kv_b_off(c.m, c.m->layers[l]); x.kv_ready = batched;
  x.d_src = io->d_enc_states; x.accumulate = (l == c.m->n_layers - 1) ? 0 : 1;
  x.d_kv_batched = batched ? offp(w.d_kv_all, (int64_t)l * 2 * c.m->d, c.es) : nullptr;
  return x;
}

// what the forward and the backward of an attention block pass alike: self (cross == false): the strided q|k|v views of w.qkv;
// cross: w.qkv against the key|value projections in w.kv.  The backward adds its gradient pointers.
imt_attn_args attn_block_args(const Ctx& c, const AttnWs& w, bool cross, int layer) {
  const int d = c.m->d; const MaskSet& ms = cross ? c.cross_ms : c.self_ms;
  imt_attn_args a;
  memset(&a, 0, sizeof(a));
  a.dtype = c.dtype; a.B = c.B; a.H = c.m->heads; a.Tq = c.T; a.Tk = cross ? c.Tk : c.T; a.head_dim = d / c.m->heads;
  a.Q = w.qkv; a.ldq = cross ? d : 3 * d;
  if (cross) { a.K = w.kv; a.ldk = w.kv_ld; a.V = offp(w.kv, d, c.es); a.ldv = w.kv_ld; }
  else       { a.K = offp(w.qkv, d, c.es); a.ldk = 3 * d; a.V = offp(w.qkv, 2 * d, c.es); a.ldv = 3 * d; }
  a.O = w.ctx; a.ldo = d; a.lse = w.lse; a.key_mask = ms.key; a.query_mask = ms.query; a.mask3d = ms.m3d; a.causal = ms.causal;
  a.scale = 1.0f / sqrtf((float)a.head_dim); a.dropout_p = c.ap; a.dropout_seed = site_seed(c.seed, layer, cross ? 4 : 0);
  return a;
}

// ------------------------------------------------------------------------------------------------ forward
// attention block (BertAttention = BertSelfAttention + BertSelfOutput) on x [N,d]
int attn_block_fwd(const Ctx& c, const imt_attn_block& p, AttnWs& w, const void* x, int layer, const Cross* cross) {
  const int d = c.m->d, N = c.N;
  if (!cross) {
    RC(run(c, linear_fwd(c, x, d, N, d, p.qkv_w, p.qkv_b, 3 * d, w.qkv, 3 * d)));
  } else {
    RC(run(c, linear_fwd(c, x, d, N, d, p.qkv_w, p.qkv_b, d, w.qkv, d)));
    if (!cross->kv_ready) RC(run(c, linear_fwd(c, cross->src, d, c.B * c.Tk, d, cross->kv_w, cross->kv_b, 2 * d, w.kv, w.kv_ld)));
  }
  const imt_attn_args a = attn_block_args(c, w, cross != nullptr, layer);
  RC(imt_attention_fwd(&a, c.st));
  return dense_resid_ln(c, w.ctx, d, p.o_w, p.o_b, x, p.ln_g, p.ln_b, w.ln, site_seed(c.seed, layer, (cross ? 4 : 0) + 1));
}

// LayerNorm backward of a block output (dy) at LayerNorm slot `slot` of `layer`: s.dpre[slot] = the gradient on the residual
// path, *d_dense = the one on the dense path (s.ddrop[slot] under hidden dropout, else the same buffer)
int block_ln_bwd(const Ctx& c, StackWs& sw, Scratch& s, int layer, int slot, const void* dy, const LnWs& ln, int64_t g_off, int64_t b_off,
                 uint64_t seed, void** d_dense) {
  void* d_pre = s.dpre[slot];
  *d_dense = (c.hp > 0.f) ? s.ddrop[slot] : d_pre;
  return imt_layernorm_bwd(c.dtype, dy, ln.pre_ln, c.P(g_off), ln.mean, ln.rstd, d_pre, c.G(g_off), c.G(b_off), c.N, c.m->d, 0.f, 0,
                           (c.hp > 0.f) ? *d_dense : nullptr, c.hp, seed, sw.ln_site(3 * layer + slot, c.m->d), c.st);
}

// backward of the block: the gradient of w.ln.out is in sw.d_run, which then receives the gradient of x; cross: also
// cross->d_src, or this layer's block of d_kv_all
int attn_block_bwd(const Ctx& c, const imt_attn_block& p, AttnWs& w, StackWs& sw, Scratch& s, DeferredDW& dw, const void* x, int layer,
                   const Cross* cross) {
  const int d = c.m->d, N = c.N, slot = cross ? 1 : 2;
  void* d_dense;
  RC(block_ln_bwd(c, sw, s, layer, slot, sw.d_run, w.ln, p.ln_g, p.ln_b, site_seed(c.seed, layer, (cross ? 4 : 0) + 1), &d_dense));
  dw.add(c, d_dense, d, w.ctx, d, N, d, d, p.o_w, p.o_b);
  // short attention in bf16: d_ctx = d_dense W_o is formed inside the attention backward (bit-identical to the pair), and
  // s.d_ctx is neither written nor read
  imt_attn_args a = attn_block_args(c, w, cross != nullptr, layer);
  const bool proj = imt_attention_bwd_proj_supported(a.dtype, a.head_dim, a.H, a.Tq, a.Tk, d, a.mask3d != nullptr);
  if (!proj) RC(run(c, linear_bwd_input(c, d_dense, d, N, d, p.o_w, d, s.d_ctx, d)));
  a.dO = proj ? nullptr : s.d_ctx; a.lddo = d; a.delta = sw.delta;
  auto attn_bwd = [&]() { return proj ? imt_attention_bwd_proj(&a, d_dense, d, c.P(p.o_w), d, d, c.st) : imt_attention_bwd(&a, c.st); };
  // the gradient of x: the query (self: q|k|v) projection's, on top of the residual path's
  auto dx = [&](const void* dq, int width) {
    dw.add(c, dq, width, x, d, N, width, d, p.qkv_w, p.qkv_b);
    imt_gemm_args g = linear_bwd_input(c, dq, width, N, width, p.qkv_w, d, sw.d_run, d);
    g.resid = s.dpre[slot]; g.ldr = d;
    return run(c, g);
  };
  if (!cross) {
    a.dQ = s.d_qkv; a.lddq = 3 * d; a.dK = offp(s.d_qkv, d, c.es); a.lddk = 3 * d; a.dV = offp(s.d_qkv, 2 * d, c.es); a.lddv = 3 * d;
    RC(attn_bwd());
    return dx(s.d_qkv, 3 * d);
  }
  const int Nk = c.B * c.Tk;
  void* dkv = cross->d_kv_batched ? cross->d_kv_batched : s.d_kv;
  const int64_t lddkv = cross->d_kv_batched ? w.kv_ld : 2 * d;
  a.dQ = s.d_q; a.lddq = d; a.dK = dkv; a.lddk = lddkv; a.dV = offp(dkv, d, c.es); a.lddv = lddkv;
  RC(attn_bwd());
  RC(dx(s.d_q, d));
  // the key|value weight gradient stays in this layer's grouped launch either way (its 32 tiles fill CUs the other six
  // products of a decoder layer leave idle; as a separate batched launch it cost +0.07 ms/step)
  dw.add(c, dkv, lddkv, cross->src, d, Nk, 2 * d, d, cross->kv_w, cross->kv_b);
  if (!cross->d_kv_batched && cross->d_src) {
    imt_gemm_args g = linear_bwd_input(c, s.d_kv, 2 * d, Nk, 2 * d, cross->kv_w, d, cross->d_src, d);
    g.accumulate = cross->accumulate;
    RC(run(c, g));
  }
  return IMT_OK;
}

int ffn_fwd(const Ctx& c, const imt_layer_desc& p, LayerWs& w, const void* x, int layer) {
  const int d = c.m->d, ff = c.m->ff;
  imt_gemm_args g = linear_fwd(c, x, d, c.N, d, p.ff1_w, p.ff1_b, ff, w.h, ff);
  g.aux = w.z; g.aux_mode = IMT_AUX_GELU_FWD;
  RC(run(c, g));
  return dense_resid_ln(c, w.h, ff, p.ff2_w, p.ff2_b, x, p.ln2_g, p.ln2_b, w.ln2, site_seed(c.seed, layer, 8));
}

// dy: the gradient of w.ln2.out; writes the gradient of x into sw.d_run
int ffn_bwd(const Ctx& c, const imt_layer_desc& p, LayerWs& w, StackWs& sw, Scratch& s, DeferredDW& dw, const void* x, int layer,
            const void* dy) {
  const int d = c.m->d, ff = c.m->ff, N = c.N;
  void* d_dense;
  RC(block_ln_bwd(c, sw, s, layer, 0, dy, w.ln2, p.ln2_g, p.ln2_b, site_seed(c.seed, layer, 8), &d_dense));
  dw.add(c, d_dense, d, w.h, ff, N, d, ff, p.ff2_w, p.ff2_b);
  imt_gemm_args g = linear_bwd_input(c, d_dense, d, N, d, p.ff2_w, ff, s.d_ff, ff);  // dz
  g.aux = w.z; g.aux_mode = IMT_AUX_DGELU;
  RC(run(c, g));
  dw.add(c, s.d_ff, ff, x, d, N, ff, d, p.ff1_w, p.ff1_b);
  g = linear_bwd_input(c, s.d_ff, ff, N, ff, p.ff1_w, d, sw.d_run, d);
  g.resid = s.dpre[0]; g.ldr = d;
  return run(c, g);
}

// the descriptor checks a training stack (`decode` false) and an incremental decoder share
int check_desc(const imt_stack_desc* m, bool decode) {
  const char* who = decode ? "decode" : "stack";
  IMT_CHECK_ARG(imt_ok_dtype(m->dtype), "%s: bad dtype", who);
  if (decode) IMT_CHECK_ARG(m->is_decoder, "decode: stack is not a decoder");
  IMT_CHECK_ARG(m->n_layers >= (decode ? 1 : 0) && m->n_layers <= MAX_LAYERS && (m->n_layers == 0 || m->layers), "%s: bad layer table", who);
  IMT_CHECK_ARG(m->d > 0 && m->heads > 0 && m->d % m->heads == 0, "%s: hidden size %d not a multiple of heads %d", who, m->d, m->heads);
  const int dh = m->d / m->heads;
  IMT_CHECK_ARG(dh == 32 || dh == 64, "%s: head_dim %d unsupported (32 or 64)", who, dh);
  IMT_CHECK_ARG(m->d % 8 == 0 && m->ff % 8 == 0, "%s: d and ff must be multiples of 8", who);
  return IMT_OK;
}

int validate(const imt_stack_desc* m, const imt_stack_io* io, const void* ws, int64_t ws_bytes, StackWs& w, LayerWs* layers) {
  IMT_CHECK_ARG(m && io, "stack: null descriptor");
  RC(check_desc(m, false));
  IMT_CHECK_ARG(io->B > 0 && io->T > 0, "stack: empty batch");
  IMT_CHECK_ARG(io->T <= m->max_pos || io->pos_ids, "stack: sequence longer than max_position_embeddings");
  IMT_CHECK_ARG(m->params && io->ids && io->out, "stack: null tensor");
  if (m->is_decoder) IMT_CHECK_ARG(io->enc_states && io->Tk > 0, "stack: decoder needs encoder states");
  carve(m, io->B, io->T, m->is_decoder ? io->Tk : 0, const_cast<void*>(ws), w, layers);
  IMT_CHECK_ARG(ws && ws_bytes >= w.bytes, "stack: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)w.bytes);
  IMT_CHECK_ARG(((uintptr_t)ws & 255) == 0, "stack: workspace must be 256-B aligned");
  return IMT_OK;
}

// gamma / beta offsets of LayerNorm site 3 * l + slot (slot 0 FFN, 1 cross, 2 self) for the fold of the partial sums; -1: the
// layer has no such LayerNorm
void ln_site_offsets(const imt_stack_desc* m, int l, int slot, int64_t* g_off, int64_t* b_off) {
  const imt_layer_desc& p = m->layers[l];
  if (slot == 0) { *g_off = p.ln2_g; *b_off = p.ln2_b; }
  else if (slot == 2) { *g_off = p.self_attn.ln_g; *b_off = p.self_attn.ln_b; }
  else if (m->is_decoder && p.cross_attn.qkv_w >= 0) { *g_off = p.cross_attn.ln_g; *b_off = p.cross_attn.ln_b; }
}

}  // namespace

extern "C" int64_t imt_stack_workspace_bytes(const imt_stack_desc* m, int B, int T, int Tk) {
  if (!m || m->n_layers > MAX_LAYERS || (m->n_layers > 0 && !m->layers)) return -1;
  StackWs w; LayerWs layers[MAX_LAYERS];
  carve(m, B, T, m->is_decoder ? Tk : 0, nullptr, w, layers);
  return w.bytes;
}

extern "C" int imt_stack_forward(const imt_stack_desc* m, const imt_stack_io* io, void* ws, int64_t ws_bytes, void* stream) {
  StackWs w; LayerWs layers[MAX_LAYERS];
  RC(validate(m, io, ws, ws_bytes, w, layers));
  Ctx c(m, stream, w.splitk, w.splitk_bytes, io);
  const int d = m->d;
  void* x0 = (m->n_layers == 0) ? io->out : w.x0;
  // parameters still being written by an optimizer step on another stream: wait site by site (imt_stack_io.wait_events)
  auto wait_site = [&](int k) {
    if (io->wait_events && k < io->n_wait_events && io->wait_events[k]) (void)hipStreamWaitEvent(c.st, (hipEvent_t)const_cast<void*>(io->wait_events[k]), 0);
  };
  wait_site(0);
  // BertEmbeddings: gather + sum + LayerNorm + dropout in one launch (the sum is kept for the backward)
  RC(imt_embed_ln_fwd(c.dtype, io->ids, io->pos_ids, io->type_ids, c.P(m->emb_word), c.P(m->emb_pos), c.P(m->emb_type), c.P(m->emb_ln_g),
                      c.P(m->emb_ln_b), w.emb_sum, x0, w.emb_mean, w.emb_rstd, c.N, c.T, d, m->vocab, m->max_pos, m->n_types, m->ln_eps,
                      c.hp, site_seed(c.seed, 1000, 0), c.st));
  const void* x = x0;
  const bool batched = cross_kv_batched(m);
  if (batched)  // key|value projections of the encoder states for ALL layers: one [B*Tk, d] x [L*2d, d]^T product
    RC(run(c, linear_fwd(c, io->enc_states, d, c.B * c.Tk, d, m->layers[0].cross_kv_w, m->layers[0].cross_kv_b, m->n_layers * 2 * d,
                         w.kv_all, (int64_t)m->n_layers * 2 * d)));
  for (int l = 0; l < m->n_layers; ++l) {
    const imt_layer_desc& p = m->layers[l]; LayerWs& L = layers[l];
    wait_site(1 + l);
    RC(attn_block_fwd(c, p.self_attn, L.self_attn, x, l, nullptr));
    const void* a = L.self_attn.ln.out;
    if (m->is_decoder && p.cross_attn.qkv_w >= 0) {
      const Cross cross = cross_of(c, io, w, l, batched);
      RC(attn_block_fwd(c, p.cross_attn, L.cross, a, l, &cross));
      a = L.cross.ln.out;
    }
    if (l == m->n_layers - 1) L.ln2.out = io->out;  // last LN writes straight into the caller's output
    RC(ffn_fwd(c, p, L, a, l));
    x = L.ln2.out;
  }
  return IMT_OK;
}

extern "C" int imt_stack_backward(const imt_stack_desc* m, const imt_stack_io* io, void* ws, int64_t ws_bytes, int layer_lo,
                                  int layer_hi, void* stream) {
  StackWs w; LayerWs layers[MAX_LAYERS];
  RC(validate(m, io, ws, ws_bytes, w, layers));
  IMT_CHECK_ARG(m->grads && io->d_out, "stack_backward: grads / d_out missing");
  IMT_CHECK_ARG(0 <= layer_lo && layer_lo <= layer_hi && layer_hi <= m->n_layers, "stack_backward: bad layer range");
  Ctx c(m, stream, w.splitk, w.splitk_bytes, io);
  const int N = c.N, d = m->d;
  // The running gradient w.r.t. the current layer's output lives in w.d_run between layers (and between segment
  // calls); the first segment reads it from io->d_out.
  const void* dy = (layer_hi == m->n_layers) ? io->d_out : w.d_run;
  const bool batched = cross_kv_batched(m);
  // LayerNorm dgamma / dbeta of this call's layers go to per-XCD partial sums (zeroed here, folded into the gradients by
  // one launch at the end): 256 workgroups per LayerNorm adding straight into the same d gradient addresses cost ~6 us
  // of serialised atomics per launch
  const int64_t lnf = IMT_LN_BWD_WS_FLOATS(d);
  if (layer_hi > layer_lo) (void)hipMemsetAsync(w.ln_site(3 * layer_lo, d), 0, (size_t)(3 * (layer_hi - layer_lo)) * lnf * 4, c.st);
  if (layer_lo == 0) (void)hipMemsetAsync(w.ln_site(3 * m->n_layers, d), 0, (size_t)lnf * 4, c.st);
  DwSchedule sched(m->n_layers, layer_lo, layer_hi, c.st);
  for (int l = layer_hi - 1; l >= layer_lo; --l) {
    const imt_layer_desc& p = m->layers[l]; LayerWs& L = layers[l];
    Scratch& s = w.scr[l % N_SCRATCH];
    sched.before_scratch(l);
    if (l == m->n_layers - 1) L.ln2.out = io->out;
    const bool has_cross = m->is_decoder && p.cross_attn.qkv_w >= 0;
    const void* x_in = (l == 0) ? w.x0 : (const void*)layers[l - 1].ln2.out;
    const void* a_self = L.self_attn.ln.out;
    RC(ffn_bwd(c, p, L, w, s, sched.dw, has_cross ? L.cross.ln.out : a_self, l, dy));
    if (has_cross) {
      const Cross cross = cross_of(c, io, w, l, batched);
      RC(attn_block_bwd(c, p.cross_attn, L.cross, w, s, sched.dw, a_self, l, &cross));
    }
    RC(attn_block_bwd(c, p.self_attn, L.self_attn, w, s, sched.dw, x_in, l, nullptr));
    RC(sched.collected(l));
    dy = w.d_run;
  }
  if (layer_lo == 0 && batched && io->d_enc_states) {
    // every layer has written its dK|dV block: d(encoder states) = d_kv_all [Nk, L*2d] x W_kv [L*2d, d], one product with
    // K = L*2d instead of L accumulating ones
    const int L2d = m->n_layers * 2 * d;
    RC(run(c, linear_bwd_input(c, w.d_kv_all, L2d, c.B * c.Tk, L2d, m->layers[0].cross_kv_w, d, io->d_enc_states, d)));
  }
  if (layer_lo == 0) {
    // (w.d_emb, not a scratch buffer of the layers: dW of layers 0 / 1 may still be reading those on the side stream)
    RC(imt_layernorm_bwd(c.dtype, m->n_layers == 0 ? io->d_out : dy, w.emb_sum, c.P(m->emb_ln_g), w.emb_mean, w.emb_rstd, w.d_emb, c.G(m->emb_ln_g), c.G(m->emb_ln_b), N, d,
                         c.hp, site_seed(c.seed, 1000, 0), nullptr, 0.f, 0, w.ln_site(3 * m->n_layers, d), c.st));
    RC(imt_embed_bwd(c.dtype, io->ids, io->pos_ids, io->type_ids, w.d_emb, c.G(m->emb_word), c.G(m->emb_pos), c.G(m->emb_type), N, c.T, d,
                     m->pad_id, c.st));
  }
  // fold the partial sums of the sites this call covered: [3*layer_lo, 3*layer_hi) and, with layer 0, the embeddings
  int64_t g_off[3 * MAX_LAYERS + 1], b_off[3 * MAX_LAYERS + 1];
  const int first = 3 * layer_lo, emb = 3 * m->n_layers;
  const int last = (layer_lo == 0) ? emb + 1 : 3 * layer_hi;  // [first, last) -- sites of layers above layer_hi are skipped
  for (int sidx = first; sidx < last; ++sidx) {
    int64_t* g = &g_off[sidx - first]; int64_t* b = &b_off[sidx - first]; *g = *b = -1;
    if (sidx == emb) { *g = m->emb_ln_g; *b = m->emb_ln_b; }
    else if (sidx / 3 < layer_hi) ln_site_offsets(m, sidx / 3, sidx % 3, g, b);
  }
  if (last > first) RC(imt_ln_partial_reduce(w.ln_site(first, d), last - first, d, g_off, b_off, m->grads, c.st));
  sched.join();
  return IMT_OK;
}

extern "C" int imt_stack_dw_schedule(int n_layers, int layer_lo, int layer_hi, int side_stream, const int* pairable, int* records, int* join_done) {
  IMT_CHECK_ARG(n_layers <= MAX_LAYERS && 0 <= layer_lo && layer_lo <= layer_hi && layer_hi <= n_layers, "stack_dw_schedule: bad layer range");
  IMT_CHECK_ARG(layer_lo == layer_hi || (pairable && records), "stack_dw_schedule: null table");
  DwPlan plan(n_layers, layer_lo, layer_hi, side_stream != 0);
  for (int l = layer_hi - 1; l >= layer_lo; --l, records += 3) {
    records[0] = plan.wait_done(l);
    records[1] = plan.collected(l, pairable[l] != 0, &records[2]);
  }
  if (join_done) *join_done = plan.last_side;
  return IMT_OK;
}

// ------------------------------------------------------------------------------------------------ incremental decoding
namespace {

struct DecodeWs {
  void* emb_sum; void* x; void* ctx; void* pre_ln; void* a; void* q; void* b; void* h; void* z; float* mean; float* rstd;
  void* splitk; int64_t splitk_bytes;  // imt_gemm's split-K slabs (R rows: a handful of output tiles per product)
  char* fused; int64_t fused_layer_bytes; unsigned* fused_bar;  // one-launch step (decode_fused.hip): per-layer hand-off buffers, barrier words
  int64_t bytes;
};

void carve_decode(const imt_stack_desc* m, int r_max, void* ws, DecodeWs& w) {
  Carver c(ws);
  const int64_t R = r_max, d = m->d, ff = m->ff, es = imt_dtype_bytes(m->dtype);
  w.emb_sum = c.take(R * d * es); w.x = c.take(R * d * es); w.ctx = c.take(R * d * es); w.pre_ln = c.take(R * d * es);
  w.a = c.take(R * d * es); w.q = c.take(R * d * es); w.b = c.take(R * d * es);
  w.h = c.take(R * ff * es); w.z = c.take(R * ff * es); w.mean = (float*)c.take(R * 4); w.rstd = (float*)c.take(R * 4);
  w.splitk_bytes = imt_gemm_splitk_ws_bytes(); w.splitk = c.take(w.splitk_bytes);
  w.fused = nullptr; w.fused_layer_bytes = 0; w.fused_bar = nullptr;
  if (m->dtype == IMT_BF16 && imt_decode_fused_shape(m->d, m->heads, m->ff, m->n_layers)) {  // bf16, hidden size 512 or 768 in heads of 64
    w.fused_layer_bytes = (imt_decode_fused_layer_bytes(r_max, m->d, m->ff) + 255) & ~(int64_t)255;
    w.fused = (char*)c.take(w.fused_layer_bytes * m->n_layers);
    w.fused_bar = (unsigned*)c.take(IMT_FUSED_BAR_WORDS * sizeof(unsigned));
  }
  w.bytes = c.off;
}

int validate_decoder(const imt_stack_desc* m) {
  IMT_CHECK_ARG(m, "decode: null descriptor");
  RC(check_desc(m, true));
  IMT_CHECK_ARG(m->params, "decode: null parameter buffer");
  for (int l = 0; l < m->n_layers; ++l)
    IMT_CHECK_ARG(m->layers[l].cross_attn.qkv_w >= 0, "decode: layer %d has no crossattention block", l);
  return IMT_OK;
}

// one layer's attention of the step, self (against the cache of the layer, `kv`, with the new position's query at q) or cross
// (w.q against the per-sentence K|V of the layer, `kv`)
imt_attn_decode_args decode_attn_args(const Ctx& c, const imt_decode_io* io, const DecodeWs& w, bool cross, const void* q, const void* kv) {
  const int d = c.m->d, dh = d / c.m->heads;
  const int64_t width = cross ? 2 * d : 3 * d;                              // one position: k|v, or q|k|v
  const int64_t ld_row = (int64_t)(cross ? io->Tk : io->t_max) * width;     // one sentence / one cache row (all positions)
  imt_attn_decode_args a;
  memset(&a, 0, sizeof(a));
  a.dtype = c.dtype; a.R = io->R; a.H = c.m->heads; a.head_dim = dh; a.n_keys = cross ? io->Tk : io->pos + 1; a.rep = cross ? io->rep : 1;
  a.Q = q; a.ldq = cross ? d : ld_row;
  a.K = cross ? kv : offp(kv, d, c.es); a.V = offp(a.K, d, c.es); a.ld_row = ld_row; a.ld_pos = width;
  if (cross) { a.key_mask = io->enc_mask; a.ld_mask = io->Tk; }
  else       { a.slots = io->slots; a.ld_slots = io->t_max; }
  a.O = w.ctx; a.ldo = d; a.scale = 1.0f / sqrtf((float)dh);
  return a;
}

// arguments of the one-launch step (decode_fused.hip): parameters, caches and the hand-off buffers of every layer
void fused_step_args(const Ctx& c, const imt_decode_io* io, const DecodeWs& w, int64_t self_layer, int64_t cross_layer, ImtFusedArgs& f) {
  const imt_stack_desc* m = c.m; const int d = m->d, ff = m->ff;
  memset(&f, 0, sizeof(f));
  const bf16_t* P = reinterpret_cast<const bf16_t*>(m->params);
  for (int l = 0; l < m->n_layers; ++l) {
    const imt_layer_desc& p = m->layers[l]; ImtFusedLayer& L = f.L[l];
    const imt_attn_block &sa = p.self_attn, &ca = p.cross_attn;
    L.wqkv = P + sa.qkv_w; L.bqkv = P + sa.qkv_b; L.wo = P + sa.o_w; L.bo = P + sa.o_b; L.g1 = P + sa.ln_g; L.b1 = P + sa.ln_b;
    L.wq = P + ca.qkv_w; L.bq = P + ca.qkv_b; L.wo2 = P + ca.o_w; L.bo2 = P + ca.o_b; L.g2 = P + ca.ln_g; L.b2 = P + ca.ln_b;
    L.w1 = P + p.ff1_w; L.bf1 = P + p.ff1_b; L.w2 = P + p.ff2_w; L.bf2 = P + p.ff2_b; L.g3 = P + p.ln2_g; L.b3 = P + p.ln2_b;
    L.cache = reinterpret_cast<bf16_t*>(offp(io->self_cache, l * self_layer, c.es));
    L.cross_kv = reinterpret_cast<const bf16_t*>(offp(io->cross_kv, l * cross_layer, c.es));
    Carver fc(w.fused + l * w.fused_layer_bytes); const int64_t rm = io->r_max;
    L.xin = (bf16_t*)fc.take(rm * d * 2); L.ctx1 = (bf16_t*)fc.take(rm * d * 2); L.a = (bf16_t*)fc.take(rm * d * 2);
    L.q = (bf16_t*)fc.take(rm * d * 2); L.ctx2 = (bf16_t*)fc.take(rm * d * 2); L.b = (bf16_t*)fc.take(rm * d * 2); L.h = (bf16_t*)fc.take(rm * ff * 2);
    L.pre1 = (float*)fc.take(rm * d * 4); L.pre2 = (float*)fc.take(rm * d * 4); L.pre3 = (float*)fc.take(rm * d * 4);
  }
  f.n_layers = m->n_layers; f.d = d; f.R = io->R; f.rep = io->rep; f.pos = io->pos; f.Tk = io->Tk; f.t_max = io->t_max; f.r_max = io->r_max;
  f.H = m->heads; f.dh = d / m->heads; f.ff = ff; f.ids = io->ids; f.pos_ids = io->pos_ids; f.type_ids = io->type_ids;
  f.emb_word = P + m->emb_word; f.emb_pos = P + m->emb_pos; f.emb_type = P + m->emb_type; f.emb_g = P + m->emb_ln_g; f.emb_b = P + m->emb_ln_b;
  f.vocab = m->vocab; f.max_pos = m->max_pos; f.n_types = m->n_types; f.out = reinterpret_cast<bf16_t*>(io->out);
  f.slots = io->slots; f.enc_mask = io->enc_mask; f.eps = m->ln_eps; f.bar = w.fused_bar;
}

}  // namespace

extern "C" int64_t imt_decode_workspace_bytes(const imt_stack_desc* m, int r_max) {
  if (!m || r_max <= 0) return -1;
  DecodeWs w; carve_decode(m, r_max, nullptr, w);
  return w.bytes;
}
extern "C" int64_t imt_decode_self_cache_bytes(const imt_stack_desc* m, int r_max, int t_max) {
  if (!m || r_max <= 0 || t_max <= 0) return -1;
  return (int64_t)m->n_layers * r_max * t_max * 3 * m->d * imt_dtype_bytes(m->dtype);
}
extern "C" int64_t imt_decode_cross_bytes(const imt_stack_desc* m, int B, int Tk) {
  if (!m || B <= 0 || Tk <= 0) return -1;
  return (int64_t)m->n_layers * B * Tk * 2 * m->d * imt_dtype_bytes(m->dtype);
}

extern "C" int imt_decode_begin(const imt_stack_desc* m, const void* enc_states, int B, int Tk, void* cross_kv, void* stream) {
  RC(validate_decoder(m));
  IMT_CHECK_ARG(enc_states && cross_kv && B > 0 && Tk > 0, "decode_begin: bad arguments");
  Ctx c(m, stream);
  const int d = m->d;
  const int64_t per_layer = (int64_t)B * Tk * 2 * d;
  for (int l = 0; l < m->n_layers; ++l)
    RC(run(c, linear_fwd(c, enc_states, d, B * Tk, d, kv_w_off(m, m->layers[l]), kv_b_off(m, m->layers[l]), 2 * d,
                         offp(cross_kv, l * per_layer, c.es), 2 * d)));
  return IMT_OK;
}

extern "C" int imt_decode_check(const imt_stack_desc* m, int r_max, const void* ws, void* stream) {
  RC(validate_decoder(m));
  IMT_CHECK_ARG(ws && r_max > 0, "decode_check: bad arguments");
  DecodeWs w;
  carve_decode(m, r_max, const_cast<void*>(ws), w);
  if (!w.fused || !imt_decode_fused_enabled()) return IMT_OK;
  unsigned status = 0;
  if (hipMemcpyAsync(&status, w.fused_bar + IMT_FUSED_BAR_WORDS - 1, sizeof(unsigned), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
      hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
    imt_set_error("decode_check: cannot read the status word");
    return IMT_ERR_LAUNCH;
  }
  if (status != 0) {
    imt_set_error("decode: a one-launch decoder step was abandoned (grid barrier %u timed out); its tokens are not valid", status & 0xfffu);
    return IMT_ERR_LAUNCH;
  }
  return IMT_OK;
}

extern "C" int imt_decode_step(const imt_stack_desc* m, const imt_decode_io* io, void* ws, int64_t ws_bytes, void* stream) {
  RC(validate_decoder(m));
  IMT_CHECK_ARG(io, "decode_step: null io");
  IMT_CHECK_ARG(io->R > 0 && io->rep > 0 && io->R % io->rep == 0 && io->R <= io->r_max, "decode_step: bad row counts (R=%d rep=%d r_max=%d)", io->R, io->rep, io->r_max);
  IMT_CHECK_ARG(io->pos >= 0 && io->pos < io->t_max && io->Tk > 0, "decode_step: position %d outside the cache (t_max=%d)", io->pos, io->t_max);
  IMT_CHECK_ARG(io->ids && io->pos_ids && io->self_cache && io->cross_kv && io->out, "decode_step: null tensor");
  DecodeWs w;
  carve_decode(m, io->r_max, ws, w);
  IMT_CHECK_ARG(ws && ws_bytes >= w.bytes, "decode_step: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)w.bytes);
  IMT_CHECK_ARG(((uintptr_t)ws & 255) == 0, "decode_step: workspace must be 256-B aligned");
  Ctx c(m, stream, w.splitk, w.splitk_bytes);
  c.N = io->R;
  const int R = io->R, d = m->d, ff = m->ff;
  const int64_t row3 = (int64_t)io->t_max * 3 * d;                       // one cache row (all positions)
  const int64_t self_layer = (int64_t)io->r_max * row3;
  const int64_t cross_layer = (int64_t)(R / io->rep) * io->Tk * 2 * d;
  if (w.fused && imt_decode_fused_enabled()) {
    // one launch for the whole stack (decode_fused.hip); the per-operator chain below stays for fp32 and other shapes
    ImtFusedArgs f;
    fused_step_args(c, io, w, self_layer, cross_layer, f);
    if (io->pos == 0 && hipMemsetAsync(w.fused_bar + IMT_FUSED_BAR_WORDS - 1, 0, sizeof(unsigned), c.st) != hipSuccess) {
      imt_set_error("decode_step: memset failed");   // a new search: clear the sticky status word
      return IMT_ERR_LAUNCH;
    }
    return imt_decode_fused_launch(f, c.st);
  }
  RC(imt_embed_ln_fwd(c.dtype, io->ids, io->pos_ids, io->type_ids, c.P(m->emb_word), c.P(m->emb_pos), c.P(m->emb_type), c.P(m->emb_ln_g),
                      c.P(m->emb_ln_b), w.emb_sum, w.x, w.mean, w.rstd, R, 1, d, m->vocab, m->max_pos, m->n_types, m->ln_eps, 0.f, 0, c.st));
  const void* x = w.x;
  for (int l = 0; l < m->n_layers; ++l) {
    const imt_layer_desc& p = m->layers[l];
    // self attention: q|k|v of the new position straight into the cache row of each hypothesis
    void* cache_l = offp(io->self_cache, l * self_layer, c.es);
    void* qkv_new = offp(cache_l, (int64_t)io->pos * 3 * d, c.es);
    RC(run(c, linear_fwd(c, x, d, R, d, p.self_attn.qkv_w, p.self_attn.qkv_b, 3 * d, qkv_new, row3)));
    imt_attn_decode_args a = decode_attn_args(c, io, w, false, qkv_new, cache_l);
    RC(imt_attention_decode(&a, c.st));
    RC(dense_resid_ln(c, w.ctx, d, p.self_attn.o_w, p.self_attn.o_b, x, p.self_attn.ln_g, p.self_attn.ln_b, LnWs{w.pre_ln, w.mean, w.rstd, w.a}, 0));
    // cross attention against the per-sentence K|V
    RC(run(c, linear_fwd(c, w.a, d, R, d, p.cross_attn.qkv_w, p.cross_attn.qkv_b, d, w.q, d)));
    a = decode_attn_args(c, io, w, true, w.q, offp(io->cross_kv, l * cross_layer, c.es));
    RC(imt_attention_decode(&a, c.st));
    RC(dense_resid_ln(c, w.ctx, d, p.cross_attn.o_w, p.cross_attn.o_b, w.a, p.cross_attn.ln_g, p.cross_attn.ln_b, LnWs{w.pre_ln, w.mean, w.rstd, w.b}, 0));
    // feed-forward
    imt_gemm_args g = linear_fwd(c, w.b, d, R, d, p.ff1_w, p.ff1_b, ff, w.h, ff);
    g.aux = w.z; g.aux_mode = IMT_AUX_GELU_FWD;
    RC(run(c, g));
    void* y = (l == m->n_layers - 1) ? io->out : w.x;
    RC(dense_resid_ln(c, w.h, ff, p.ff2_w, p.ff2_b, w.b, p.ln2_g, p.ln2_b, LnWs{w.pre_ln, w.mean, w.rstd, y}, 0));
    x = y;
  }
  return IMT_OK;
}
