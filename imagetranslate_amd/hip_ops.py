"""Tensor-level wrappers over the C ABI (no autograd here): each function takes torch CUDA tensors, passes
raw device pointers / sizes / the current HIP stream to ``libimt_hip.so`` and returns torch tensors that own
the outputs.  PyTorch supplies memory and streams only.
"""
import contextlib
import ctypes
import os
import math

import torch

from . import _lib as L
from ._lib import IMT_AUX_DGELU, IMT_AUX_GELU_FWD, IMT_AUX_NONE, IMT_AUX_SPLITK_WS, IMT_BF16, IMT_F32, IMT_NN, IMT_NT, IMT_TN  # noqa: F401


def dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return IMT_F32
    if t.dtype == torch.bfloat16:
        return IMT_BF16
    raise TypeError("imagetranslate_amd supports float32 and bfloat16 tensors, got %s" % t.dtype)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _req_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.ImtError("imagetranslate_amd HIP ops need tensors on the GPU (no CPU fallback)")


def alloc_rows(n_rows, width, dtype, device):
    """[n_rows, width] view of a zero-initialised buffer whose leading dimension is rounded up to 8 elements: rows stay
    16-byte aligned for the vector loads/stores when ``width`` (e.g. a tokenizer's vocabulary size) is not a multiple
    of 8, and the pad columns hold zeros."""
    padded = (width + 7) // 8 * 8
    if padded == width:
        return torch.empty((n_rows, width), device=device, dtype=dtype)
    return torch.zeros((n_rows, padded), device=device, dtype=dtype)[:, :width]


def rows16(t):
    """A 2-D tensor as rows the kernels can address with 16-byte vector accesses: unit inner stride and a leading
    dimension that is a multiple of 8 elements (already true for the padded buffers of alloc_rows); copies otherwise."""
    if t.dim() == 2 and t.stride(1) == 1 and (t.stride(0) % 8 == 0 or t.shape[0] <= 1) and t.data_ptr() % 16 == 0:
        return t
    out = alloc_rows(t.shape[0], t.shape[1], t.dtype, t.device)
    out.copy_(t)
    return out


def _rowmajor(t):
    assert t.dim() == 2 and t.stride(1) == 1, "row-major 2-D view expected"
    return t.stride(0)


def gemm(A, B, layout, *, out=None, out_dtype=None, bias=None, resid=None, aux=None, aux_mode=IMT_AUX_NONE,
         accumulate=False, split_k=1, alpha=1.0, dropout_p=0.0, dropout_seed=0, alpha_dev=None, a_colsum=None,
         force_general=False, ln=None, splitk_ws=None, _launch=True):
    """C = epilogue(op(A) op(B)); see include/imt_hip.h:imt_gemm.  ``splitk_ws``: fp32 scratch (``splitk_workspace(device)``)
    that lets a product with few output tiles and a long K run as K ranges + one epilogue launch."""
    _req_cuda(A, B, out, bias, resid, aux)
    if layout == IMT_NT:
        M, K = A.shape; N = B.shape[0]; assert B.shape[1] == K
    elif layout == IMT_NN:
        M, K = A.shape; N = B.shape[1]; assert B.shape[0] == K
    else:
        K, M = A.shape; N = B.shape[1]; assert B.shape[0] == K
    if out is None:
        out = alloc_rows(M, N, out_dtype or A.dtype, A.device)
        assert not accumulate and split_k == 1
    a = L.GemmArgs()
    a.dtype, a.layout = dt(A), layout
    a.M, a.N, a.K = M, N, K
    a.A, a.lda = A.data_ptr(), _rowmajor(A)
    a.B, a.ldb = B.data_ptr(), _rowmajor(B)
    a.C, a.ldc = out.data_ptr(), _rowmajor(out)
    a.c_dtype = dt(out)
    a.accumulate = int(accumulate)
    a.bias = bias.data_ptr() if bias is not None else None
    a.resid, a.ldr = (resid.data_ptr(), _rowmajor(resid)) if resid is not None else (None, 0)
    a.aux, a.ldaux = (aux.data_ptr(), _rowmajor(aux)) if aux is not None else (None, 0)
    a.aux_mode, a.split_k = aux_mode, split_k
    a.alpha, a.dropout_p, a.dropout_seed = alpha, dropout_p, dropout_seed
    a.alpha_dev = alpha_dev.data_ptr() if alpha_dev is not None else None
    a.a_colsum = a_colsum.data_ptr() if a_colsum is not None else None
    a.force_general = int(force_general)
    if splitk_ws is not None:
        _req_cuda(splitk_ws)
        a.splitk_ws, a.splitk_ws_bytes = splitk_ws.data_ptr(), splitk_ws.numel() * splitk_ws.element_size()
    if ln is not None:
        # ln = dict(gamma, beta, out, mean, rstd, eps): LayerNorm of the rows of `out` in the same call
        _req_cuda(ln["gamma"], ln["beta"], ln["out"], ln["mean"], ln["rstd"])
        a.ln_gamma, a.ln_beta = ln["gamma"].data_ptr(), ln["beta"].data_ptr()
        a.ln_out, a.ld_ln = ln["out"].data_ptr(), _rowmajor(ln["out"])
        a.ln_mean, a.ln_rstd = ln["mean"].data_ptr(), ln["rstd"].data_ptr()
        a.ln_eps = float(ln.get("eps", 1e-12))
    if not _launch:
        return a
    L.check(L.load().imt_gemm(ctypes.byref(a), _stream()), "imt_gemm")
    return out


_SPLITK_WS = {}


def splitk_workspace(device):
    """One fp32 scratch per device for imt_gemm's split-K slab mode (stream-ordered use: one product at a time)."""
    key = (device.type, device.index)
    ws = _SPLITK_WS.get(key)
    if ws is None:
        ws = torch.empty(int(L.load().imt_gemm_splitk_ws_bytes()) // 4, device=device, dtype=torch.float32)
        _SPLITK_WS[key] = ws
    return ws


def dw_split_k(rows: int, N: int, K: int, rows_per_split: int) -> int:
    """K-splits of a weight-gradient TN GEMM ``dy^T x -> [N, K]`` over ``rows`` rows: one per ``rows_per_split`` rows, as
    long as the 128 x 128 output tiles times the splits stay within 512 workgroups."""
    return max(1, min(rows // rows_per_split, 512 // max(1, ((N + 127) // 128) * ((K + 127) // 128))))


@contextlib.contextmanager
def grouped_tall_min_tiles(min_tiles):
    """Tests / tuning: while the block runs, groups (and layer pairs of a stack's backward) take 256 x 128 tiles from
    ``min_tiles`` of them on, where every row count allows; 1 = always, 1 << 30 = never."""
    prev = L.load().imt_set_gemm_grouped_tall_min_tiles(int(min_tiles))
    try:
        yield
    finally:
        L.load().imt_set_gemm_grouped_tall_min_tiles(prev)


def gemm_grouped_tn(problems, tile_rows=0):
    """problems: list of dicts(A=dy[K,M], B=x[K,N], out=fp32 grad [M,N], a_colsum=optional, alpha=optional, 1.0) -> one launch
    (one imt_gemm per product where the list is not groupable: imt_gemm_grouped_tn).
    tile_rows (tests / tuning): 256 = the 256 x 128 instance whenever every row count allows it, 128 = never, 0 = the policy."""
    arr = (L.GemmArgs * len(problems))()
    for i, pr in enumerate(problems):
        arr[i] = gemm(pr["A"], pr["B"], IMT_TN, out=pr["out"], accumulate=True, a_colsum=pr.get("a_colsum"), alpha=pr.get("alpha", 1.0),
                      _launch=False)
    with grouped_tall_min_tiles({128: 1 << 30, 256: 1}[tile_rows]) if tile_rows else contextlib.nullcontext():
        L.check(L.load().imt_gemm_grouped_tn(arr, len(problems), _stream()), "imt_gemm_grouped_tn")


def grouped_tile_order(grids, plain=False):
    """Tile order of the grouped launch for a group whose problems have ``grids[i] = (tile rows, tile columns)``: a list
    with (problem, tile row, tile column) of every hardware workgroup (workgroup w runs on XCD w % 8).  Host only."""
    n = len(grids)
    total = sum(r * c for r, c in grids)
    rows, cols = (ctypes.c_int * n)(*[g[0] for g in grids]), (ctypes.c_int * n)(*[g[1] for g in grids])
    order = (ctypes.c_int * (3 * total))()
    L.check(L.load().imt_gemm_grouped_tile_order(rows, cols, n, int(plain), order, total), "imt_gemm_grouped_tile_order")
    return [(order[3 * w], order[3 * w + 1], order[3 * w + 2]) for w in range(total)]


DW_HOLD, DW_FLUSH_MAIN, DW_FLUSH_SIDE = 0, 1, 2


def stack_dw_schedule(n_layers, layer_lo, layer_hi, side_stream, pairable):
    """Where imt_stack_backward(layer_lo, layer_hi) sends the weight-gradient launch of each layer (imt_stack_dw_schedule):
    ``pairable[l]`` says whether layer l's products would take the 256 x 128 instance with as many again.  Returns
    ([(layer, wait_done, action, with_held)] from layer_hi - 1 down to layer_lo, join_done).  Host only."""
    n = layer_hi - layer_lo
    pair = (ctypes.c_int * max(1, n_layers))(*[int(bool(x)) for x in pairable])
    rec = (ctypes.c_int * max(1, 3 * n))()
    join = ctypes.c_int(-1)
    L.check(L.load().imt_stack_dw_schedule(n_layers, layer_lo, layer_hi, int(side_stream), pair, rec, ctypes.byref(join)),
            "imt_stack_dw_schedule")
    return [(layer_hi - 1 - i, rec[3 * i], rec[3 * i + 1], rec[3 * i + 2]) for i in range(n)], join.value


def gemm_bias_residual_ln(x, w, bias, resid, gamma, beta, eps=1e-12, dropout_p=0.0, dropout_seed=0, want_pre_ln=True):
    """out = LayerNorm(dropout(x w^T + bias) + resid) in one launch (imt_gemm_bias_residual_ln); returns
    (out, pre_ln or None, mean, rstd)."""
    _req_cuda(x, w, bias, resid, gamma, beta)
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K
    out = torch.empty((M, N), device=x.device, dtype=x.dtype)
    pre = torch.empty((M, N), device=x.device, dtype=x.dtype) if want_pre_ln else None
    mean = torch.empty(M, device=x.device, dtype=torch.float32)
    rstd = torch.empty(M, device=x.device, dtype=torch.float32)
    L.check(L.load().imt_gemm_bias_residual_ln(dt(x), _p(x), _rowmajor(x), _p(w), _rowmajor(w), _p(bias), _p(resid),
                                               _rowmajor(resid) if resid is not None else 0, _p(gamma), _p(beta), _p(pre), _p(out), N,
                                               _p(mean), _p(rstd), M, N, K, eps, dropout_p, dropout_seed, _stream()),
            "imt_gemm_bias_residual_ln")
    return out, pre, mean, rstd


def colsum(X, out, scale_dev=None):
    _req_cuda(X, out)
    L.check(L.load().imt_colsum(dt(X), _p(X), _rowmajor(X), X.shape[0], X.shape[1], _p(out), _p(scale_dev), _stream()),
            "imt_colsum")
    return out


def layernorm_fwd(x, gamma, beta, eps=1e-12, dropout_p=0.0, dropout_seed=0):
    _req_cuda(x, gamma, beta)
    rows, d = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    L.check(L.load().imt_layernorm_fwd(dt(x), _p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, d, eps,
                                       dropout_p, dropout_seed, _stream()), "imt_layernorm_fwd")
    return y, mean, rstd


def add_layernorm_fwd(x, resid, gamma, beta, eps=1e-12, dropout_p=0.0, dropout_seed=0):
    """(y, x + resid, mean, rstd) with y = dropout(LayerNorm(x + resid)) in one launch (imt_add_layernorm_fwd)."""
    _req_cuda(x, resid, gamma, beta)
    rows, d = x.shape
    y, ssum = torch.empty_like(x), torch.empty_like(x)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    L.check(L.load().imt_add_layernorm_fwd(dt(x), _p(x), _p(resid), _p(gamma), _p(beta), _p(ssum), _p(y), _p(mean), _p(rstd), rows, d,
                                           eps, dropout_p, dropout_seed, _stream()), "imt_add_layernorm_fwd")
    return y, ssum, mean, rstd


def embed_ln_fwd(ids, pos_ids, type_ids, word, pos, typ, gamma, beta, seq_len, eps=1e-12, dropout_p=0.0, dropout_seed=0):
    """BertEmbeddings in one launch (imt_embed_ln_fwd): (y, sum, mean, rstd)."""
    _req_cuda(ids, word, gamma, beta)
    n, d = ids.numel(), word.shape[1]
    y = torch.empty((n, d), device=word.device, dtype=word.dtype)
    ssum = torch.empty_like(y)
    mean = torch.empty(n, device=word.device, dtype=torch.float32)
    rstd = torch.empty(n, device=word.device, dtype=torch.float32)
    L.check(L.load().imt_embed_ln_fwd(dt(word), _p(ids), _p(pos_ids), _p(type_ids), _p(word), _p(pos), _p(typ), _p(gamma), _p(beta),
                                      _p(ssum), _p(y), _p(mean), _p(rstd), n, seq_len, d, word.shape[0], pos.shape[0], typ.shape[0], eps,
                                      dropout_p, dropout_seed, _stream()), "imt_embed_ln_fwd")
    return y, ssum, mean, rstd


LN_PARTIAL_COPIES = 32  # IMT_LN_PARTIAL_COPIES (include/imt_hip.h)


def layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta, y_dropout_p=0.0, y_dropout_seed=0, want_dx_drop=False,
                  dx_dropout_p=0.0, dx_dropout_seed=0, partial_ws=None):
    """partial_ws: optional ZEROED fp32 [LN_PARTIAL_COPIES, 2, d] buffer -- the column sums go there instead of into
    dgamma / dbeta (fold with ln_partial_reduce); None = straight atomics into dgamma / dbeta."""
    _req_cuda(dy, x, gamma, dgamma, dbeta, partial_ws)
    rows, d = x.shape
    dx = torch.empty_like(x)
    dx_drop = torch.empty_like(x) if want_dx_drop else None
    ws = partial_ws
    if ws is not None:
        assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() == LN_PARTIAL_COPIES * 2 * d
    L.check(L.load().imt_layernorm_bwd(dt(x), _p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dgamma),
                                       _p(dbeta), rows, d, y_dropout_p, y_dropout_seed, _p(dx_drop), dx_dropout_p,
                                       dx_dropout_seed, _p(ws), _stream()), "imt_layernorm_bwd")
    return (dx, dx_drop) if want_dx_drop else dx


def ln_partial_reduce(partials, grads, dgamma_offsets, dbeta_offsets):
    """grads[dgamma_offsets[i] + c] += sum over the copies of partials[i, :, 0, c] (likewise dbeta with [i, :, 1, c]);
    partials: fp32 [n, LN_PARTIAL_COPIES, 2, d]; a negative dgamma offset skips that buffer.  One launch."""
    _req_cuda(partials, grads)
    n, copies, two, d = partials.shape
    assert copies == LN_PARTIAL_COPIES and two == 2 and partials.is_contiguous() and grads.dtype == torch.float32
    g = (ctypes.c_int64 * n)(*[int(v) for v in dgamma_offsets])
    b = (ctypes.c_int64 * n)(*[int(v) for v in dbeta_offsets])
    L.check(L.load().imt_ln_partial_reduce(_p(partials), n, d, g, b, _p(grads), _stream()), "imt_ln_partial_reduce")


def embed_fwd(ids, pos_ids, type_ids, word, pos, typ, seq_len):
    _req_cuda(ids, word)
    n = ids.numel()
    d = word.shape[1]
    out = torch.empty((n, d), device=word.device, dtype=word.dtype)
    L.check(L.load().imt_embed_fwd(dt(word), _p(ids), _p(pos_ids), _p(type_ids), _p(word), _p(pos), _p(typ), _p(out), n,
                                   seq_len, d, word.shape[0], pos.shape[0], typ.shape[0], _stream()), "imt_embed_fwd")
    return out


def embed_bwd(ids, pos_ids, type_ids, dsum, dword, dpos, dtype_tab, seq_len, pad_id):
    _req_cuda(ids, dsum, dword, dpos, dtype_tab)
    n, d = dsum.shape
    L.check(L.load().imt_embed_bwd(dt(dsum), _p(ids), _p(pos_ids), _p(type_ids), _p(dsum), _p(dword), _p(dpos),
                                   _p(dtype_tab), n, seq_len, d, pad_id, _stream()), "imt_embed_bwd")


def _attn_args(q, k, v, B, H, Tq, Tk, head_dim, key_mask, query_mask, mask3d, causal, scale, dropout_p, dropout_seed):
    a = L.AttnArgs()
    a.dtype = dt(q)
    a.B, a.H, a.Tq, a.Tk, a.head_dim = B, H, Tq, Tk, head_dim
    a.Q, a.ldq = q.data_ptr(), _rowmajor(q)
    a.K, a.ldk = k.data_ptr(), _rowmajor(k)
    a.V, a.ldv = v.data_ptr(), _rowmajor(v)
    a.key_mask = key_mask.data_ptr() if key_mask is not None else None
    a.query_mask = query_mask.data_ptr() if query_mask is not None else None
    a.mask3d = mask3d.data_ptr() if mask3d is not None else None
    a.causal = int(causal)
    a.scale = scale if scale is not None else 1.0 / math.sqrt(head_dim)
    a.dropout_p, a.dropout_seed = dropout_p, dropout_seed
    return a


def attention_fwd(q, k, v, B, H, Tq, Tk, head_dim, key_mask=None, query_mask=None, mask3d=None, causal=False,
                  scale=None, dropout_p=0.0, dropout_seed=0, o=None, lse=None):
    """q: [B*Tq, >=H*head_dim] row-major view (heads merged), k/v: [B*Tk, ...]; masks uint8.  ``o`` ([B*Tq, H*head_dim]
    row-major view of q's dtype, any 16-byte-multiple leading dimension) and ``lse`` (contiguous fp32 [B, H, Tq]) receive
    the results when given, as dq / dk / dv do in attention_bwd."""
    _req_cuda(q, k, v, key_mask, query_mask, mask3d, o, lse)
    a = _attn_args(q, k, v, B, H, Tq, Tk, head_dim, key_mask, query_mask, mask3d, causal, scale, dropout_p, dropout_seed)
    if o is None:
        o = torch.empty((B * Tq, H * head_dim), device=q.device, dtype=q.dtype)
    else:
        assert o.dtype == q.dtype and tuple(o.shape) == (B * Tq, H * head_dim), "attention_fwd: o must be [B*Tq, H*head_dim] of q's dtype"
    if lse is None:
        lse = torch.empty((B, H, Tq), device=q.device, dtype=torch.float32)
    else:
        assert lse.dtype == torch.float32 and tuple(lse.shape) == (B, H, Tq) and lse.is_contiguous(), "attention_fwd: lse must be contiguous fp32 [B, H, Tq]"
    a.O, a.ldo, a.lse = o.data_ptr(), _rowmajor(o), lse.data_ptr()
    L.check(L.load().imt_attention_fwd(ctypes.byref(a), _stream()), "imt_attention_fwd")
    return o, lse


def attention_bwd(do, q, k, v, o, lse, B, H, Tq, Tk, head_dim, key_mask=None, query_mask=None, mask3d=None,
                  causal=False, scale=None, dropout_p=0.0, dropout_seed=0, dq=None, dk=None, dv=None):
    _req_cuda(do, q, k, v, o, lse)
    a = _attn_args(q, k, v, B, H, Tq, Tk, head_dim, key_mask, query_mask, mask3d, causal, scale, dropout_p, dropout_seed)
    if dq is None:
        dq = torch.empty((B * Tq, H * head_dim), device=q.device, dtype=q.dtype)
    if dk is None:
        dk = torch.empty((B * Tk, H * head_dim), device=q.device, dtype=q.dtype)
    if dv is None:
        dv = torch.empty((B * Tk, H * head_dim), device=q.device, dtype=q.dtype)
    delta = torch.empty((B, H, Tq), device=q.device, dtype=torch.float32)
    a.O, a.ldo, a.lse = o.data_ptr(), _rowmajor(o), lse.data_ptr()
    a.dO, a.lddo = do.data_ptr(), _rowmajor(do)
    a.dQ, a.lddq = dq.data_ptr(), _rowmajor(dq)
    a.dK, a.lddk = dk.data_ptr(), _rowmajor(dk)
    a.dV, a.lddv = dv.data_ptr(), _rowmajor(dv)
    a.delta = delta.data_ptr()
    L.check(L.load().imt_attention_bwd(ctypes.byref(a), _stream()), "imt_attention_bwd")
    return dq, dk, dv


def attention_bwd_proj(dy, w_o, q, k, v, o, lse, B, H, Tq, Tk, head_dim, key_mask=None, query_mask=None, causal=False,
                       scale=None, dropout_p=0.0, dropout_seed=0, do_out=None):
    """(dq, dk, dv) of the attention whose output went through the projection y = ctx W_o^T: dO = dy W_o is formed inside
    the backward launch (imt_attention_bwd_proj).  dy [B*Tq, d], w_o [d, d] row-major; ``do_out`` ([B*Tq, d]) receives dO
    when given."""
    _req_cuda(dy, w_o, q, k, v, o, lse, do_out)
    d = H * head_dim
    a = _attn_args(q, k, v, B, H, Tq, Tk, head_dim, key_mask, query_mask, None, causal, scale, dropout_p, dropout_seed)
    dq = torch.empty((B * Tq, d), device=q.device, dtype=q.dtype)
    dk = torch.empty((B * Tk, d), device=q.device, dtype=q.dtype)
    dv = torch.empty((B * Tk, d), device=q.device, dtype=q.dtype)
    delta = torch.empty((B, H, Tq), device=q.device, dtype=torch.float32)
    a.O, a.ldo, a.lse = o.data_ptr(), _rowmajor(o), lse.data_ptr()
    if do_out is not None:
        a.dO, a.lddo = do_out.data_ptr(), _rowmajor(do_out)
    a.dQ, a.lddq = dq.data_ptr(), _rowmajor(dq)
    a.dK, a.lddk = dk.data_ptr(), _rowmajor(dk)
    a.dV, a.lddv = dv.data_ptr(), _rowmajor(dv)
    a.delta = delta.data_ptr()
    L.check(L.load().imt_attention_bwd_proj(ctypes.byref(a), _p(dy), _rowmajor(dy), _p(w_o), _rowmajor(w_o), d, _stream()),
            "imt_attention_bwd_proj")
    return dq, dk, dv


def gather_rows(x, idx):
    _req_cuda(x, idx)
    out = torch.empty((idx.numel(), x.shape[1]), device=x.device, dtype=x.dtype)
    L.check(L.load().imt_gather_rows(dt(x), _p(x), _rowmajor(x), _p(idx), _p(out), out.stride(0) if out.numel() else x.shape[1],
                                     idx.numel(), x.shape[1], _stream()), "imt_gather_rows")
    return out


def scatter_rows(dout, idx, dx):
    _req_cuda(dout, idx, dx)
    L.check(L.load().imt_scatter_rows(dt(dout), _p(dout), _rowmajor(dout) if dout.numel() else dx.shape[1], _p(idx), _p(dx),
                                      _rowmajor(dx), idx.numel(), dx.shape[1], _stream()), "imt_scatter_rows")
    return dx


def log_softmax_fwd(logits):
    _req_cuda(logits)
    N, V = logits.shape
    lp = alloc_rows(N, V, torch.float32, logits.device)
    lse = torch.empty(N, device=logits.device, dtype=torch.float32)
    L.check(L.load().imt_log_softmax_fwd(dt(logits), _p(logits), _rowmajor(logits) if N else V, _p(lp), lp.stride(0) if N else V, _p(lse), N, V,
                                         _stream()), "imt_log_softmax_fwd")
    return lp, lse


_SCORE_WS = {}
SCORE_CHUNK_ROWS = 2048  # rows per [rows, V] fp32 block where the fused scorer does not take the shape


def score_workspace(device, nbytes):
    """One scratch per device for imt_score_rows, grown on demand (stream-ordered use: one call at a time)."""
    key = (device.type, device.index)
    ws = _SCORE_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(int(nbytes), device=device, dtype=torch.uint8)
        _SCORE_WS[key] = ws
    return ws


def score_rows(x, weight, bias, targets, seg_offsets=None, normalize=True):
    """Log-probability of ``targets[r]`` under softmax(x[r] W^T + b) for every row, without the [N, V] logits
    (include/imt_hip.h: imt_score_rows; src/score_pairs.py:116-127).  x [N, K], weight [V, K], bias [V] or None in one
    dtype (fp32 / bf16); targets int64 [N], a target outside [0, V) marks the row as ignored (log-prob 0, not counted).
    seg_offsets int64 [n_seg + 1]: rows [off[s], off[s + 1]) are sentence s.  Returns (logprob [N], lse [N], seg_score
    [n_seg] or None), all fp32.  Where ``imt_score_supported`` says no, the same numbers come from the existing kernels
    (fp32 logits, log-softmax, gather) in blocks of at most SCORE_CHUNK_ROWS rows, so memory stays bounded there too."""
    _req_cuda(x, weight, bias, targets, seg_offsets)
    N, K = x.shape
    V = weight.shape[0]
    assert weight.shape[1] == K and weight.dtype == x.dtype and (bias is None or bias.dtype == x.dtype)
    assert targets.dtype == torch.int64 and targets.numel() == N
    dev = x.device
    n_seg = 0 if seg_offsets is None else seg_offsets.numel() - 1
    logprob = torch.empty(N, device=dev, dtype=torch.float32)
    lse = torch.empty(N, device=dev, dtype=torch.float32)
    seg = torch.zeros(max(n_seg, 0), device=dev, dtype=torch.float32) if seg_offsets is not None else None
    if N == 0:
        return logprob, lse, seg
    x, weight, targets = rows16(x), rows16(weight), targets.contiguous()
    if bias is not None and (bias.data_ptr() % 16 or bias.stride(0) != 1):
        bias = bias.clone()
    lib = L.load()
    if lib.imt_score_supported(dt(x), V, K):
        if seg_offsets is not None:
            assert seg_offsets.dtype == torch.int64 and n_seg >= 1
            seg_offsets = seg_offsets.contiguous()
        nbytes = int(lib.imt_score_ws_bytes(N, V))
        ws = score_workspace(dev, nbytes)
        a = L.ScoreArgs()
        a.dtype, a.N, a.V, a.K = dt(x), N, V, K
        a.x, a.ldx = x.data_ptr(), _rowmajor(x) if N > 1 else max(K, x.stride(0))
        a.w, a.ldw = weight.data_ptr(), _rowmajor(weight) if V > 1 else max(K, weight.stride(0))
        a.bias = bias.data_ptr() if bias is not None else None
        a.target, a.logprob, a.lse = targets.data_ptr(), logprob.data_ptr(), lse.data_ptr()
        if seg_offsets is not None:
            a.seg_offsets, a.n_seg, a.seg_score = seg_offsets.data_ptr(), n_seg, seg.data_ptr()
        a.normalize = int(bool(normalize))
        a.ws, a.ws_bytes = ws.data_ptr(), nbytes
        L.check(lib.imt_score_rows(ctypes.byref(a), _stream()), "imt_score_rows")
        return logprob, lse, seg
    valid = (targets >= 0) & (targets < V)
    safe = torch.where(valid, targets, torch.zeros_like(targets))
    for r0 in range(0, N, SCORE_CHUNK_ROWS):
        r1 = min(N, r0 + SCORE_CHUNK_ROWS)
        logits = gemm(x[r0:r1], weight, IMT_NT, bias=bias, out_dtype=torch.float32)
        lp, l = log_softmax_fwd(logits)
        logprob[r0:r1] = lp.gather(1, safe[r0:r1].unsqueeze(1)).squeeze(1)
        lse[r0:r1] = l
    logprob.masked_fill_(~valid, 0.0)
    if seg_offsets is not None:
        off = seg_offsets.clamp(0, N)
        csum = torch.cat([logprob.new_zeros(1, dtype=torch.float64), logprob.double().cumsum(0)])
        ccnt = torch.cat([off.new_zeros(1), valid.long().cumsum(0)])
        tot = (csum[off[1:]] - csum[off[:-1]])
        cnt = (ccnt[off[1:]] - ccnt[off[:-1]])
        if normalize:
            tot = torch.where(cnt > 0, tot / cnt.clamp(min=1).double(), tot)
        seg = tot.float()
    return logprob, lse, seg


KNN_MAX_K = 8  # IMT_KNN_MAX_K


def _knn_operand(t):
    """Rows for imt_knn_rows: K zero-padded up to a whole 128-byte K tile (a zero column changes no product), 16-byte rows."""
    tile = 128 // t.element_size()
    K = t.shape[1]
    if K % tile:
        out = torch.zeros((t.shape[0], (K + tile - 1) // tile * tile), device=t.device, dtype=t.dtype)
        out[:, :K] = t
        return out
    return rows16(t)


def _knn_max_rows(t):
    """Most rows of ``t`` one call may see: (rows + 256) * ld * element size stays below 2 GiB (32-bit DMA offsets)."""
    ld = max(t.shape[1], t.stride(0))
    return ((1 << 31) - 1) // (ld * t.element_size()) - 256


def knn_rows(x, y, k, *, splits=0, _key_chunk=None, _query_chunk=None):
    """The k keys of largest inner product for every query, without the [N, M] similarities (include/imt_hip.h:
    imt_knn_rows).  x [N, K], y [M, K] in one dtype (fp32 / bf16).  Returns (val [N, k] fp32, idx [N, k] int64): by value
    descending, then index ascending; places past M hold -inf / -1.  Operands beyond the kernel's 2 GiB limit are cut into
    row chunks; the key chunks' lists are merged by a stable descending sort (chunks arrive in index order, so equal values
    keep index order).  ``_key_chunk`` / ``_query_chunk``: keys / queries per call, for tests."""
    _req_cuda(x, y)
    N, K = x.shape
    M = y.shape[0]
    if y.shape[1] != K or y.dtype != x.dtype:
        raise ValueError("knn_rows: queries %s %s against keys %s %s" % (tuple(x.shape), x.dtype, tuple(y.shape), y.dtype))
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError("knn_rows: k = %d outside 1..%d" % (k, KNN_MAX_K))
    dev = x.device
    if N == 0 or M == 0:
        return (torch.full((N, k), float("-inf"), device=dev, dtype=torch.float32),
                torch.full((N, k), -1, device=dev, dtype=torch.int64))
    x, y = _knn_operand(x), _knn_operand(y)
    Kp = x.shape[1]
    lib = L.load()
    if not lib.imt_knn_supported(dt(x), Kp):
        raise L.ImtError("knn_rows: (dtype %s, K %d) is not taken by imt_knn_rows" % (x.dtype, Kp))
    q_rows = max(1, min(_knn_max_rows(x), int(_query_chunk) if _query_chunk else N))
    k_rows = max(1, min(_knn_max_rows(y), int(_key_chunk) if _key_chunk else M))
    val = torch.empty((N, k), device=dev, dtype=torch.float32)
    idx = torch.empty((N, k), device=dev, dtype=torch.int64)
    n_chunks = (M + k_rows - 1) // k_rows
    for r0 in range(0, N, q_rows):
        r1 = min(N, r0 + q_rows)
        xs = x[r0:r1]
        cv = torch.empty((r1 - r0, n_chunks * k), device=dev, dtype=torch.float32)
        ci = torch.empty((r1 - r0, n_chunks * k), device=dev, dtype=torch.int32)
        for c, c0 in enumerate(range(0, M, k_rows)):
            ys = y[c0:min(M, c0 + k_rows)]
            v = torch.empty((r1 - r0, k), device=dev, dtype=torch.float32)
            i = torch.empty((r1 - r0, k), device=dev, dtype=torch.int32)
            nbytes = int(lib.imt_knn_ws_bytes(xs.shape[0], ys.shape[0], k, splits))
            ws = score_workspace(dev, nbytes)
            a = L.KnnArgs()
            a.dtype, a.N, a.M, a.K, a.k = dt(x), xs.shape[0], ys.shape[0], Kp, k
            a.x, a.ldx = xs.data_ptr(), max(Kp, xs.stride(0))
            a.y, a.ldy = ys.data_ptr(), max(Kp, ys.stride(0))
            a.index_base, a.splits = c0, int(splits)
            a.val, a.idx = v.data_ptr(), i.data_ptr()
            a.ws, a.ws_bytes = ws.data_ptr(), nbytes
            L.check(lib.imt_knn_rows(ctypes.byref(a), _stream()), "imt_knn_rows")
            cv[:, c * k:(c + 1) * k] = v
            ci[:, c * k:(c + 1) * k] = i
        if n_chunks == 1:
            val[r0:r1], idx[r0:r1] = cv, ci.long()
        else:
            sv, order = torch.sort(cv, dim=1, descending=True, stable=True)
            val[r0:r1] = sv[:, :k]
            idx[r0:r1] = ci.gather(1, order[:, :k]).long()
    return val, idx


ALIGN_MAX_LEN = 512  # IMT_ALIGN_MAX_LEN


def _align_operand(t):
    """[B, rows, d] for imt_align_pairs: d zero-padded up to a whole 128-byte step (a zero column changes neither a product
    nor a norm); a view is passed as it is where its strides allow (unit inner stride, rows and pairs on 16-byte boundaries,
    pairs that do not overlap), and copied otherwise."""
    step = 128 // t.element_size()
    epv = 16 // t.element_size()
    B, rows, d = t.shape
    if d % step:
        out = torch.zeros((B, rows, (d + step - 1) // step * step), device=t.device, dtype=t.dtype)
        out[:, :, :d] = t
        return out
    ok = t.stride(2) == 1 and t.data_ptr() % 16 == 0
    ok = ok and (rows == 1 or (t.stride(1) >= d and t.stride(1) % epv == 0))
    ok = ok and (B == 1 or (t.stride(0) % epv == 0 and t.stride(0) >= (rows - 1) * (t.stride(1) if rows > 1 else 0) + d))
    return t if ok else t.contiguous()


def align_pairs(x, y, x_range, y_range, min_sim=float("-inf")):
    """Mutual arg-max word alignment of B sentence pairs without the [B, S, T] similarities (include/imt_hip.h:
    imt_align_pairs).  x [B, S, d], y [B, T, d] in one dtype (fp32 / bf16); x_range / y_range [B, 2] integer (begin, end) of
    the tokens to align.  Returns (link [B, S], fwd_idx [B, S], fwd_val [B, S], bwd_idx [B, T], bwd_val [B, T]): indices
    int64 (-1: none), values fp32 cosines (-inf: none)."""
    if x.dim() != 3 or y.dim() != 3 or x.shape[0] != y.shape[0] or x.shape[2] != y.shape[2] or x.dtype != y.dtype:
        raise ValueError("align_pairs: x %s %s against y %s %s" % (tuple(x.shape), x.dtype, tuple(y.shape), y.dtype))
    B, S, d = x.shape
    T = y.shape[1]
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("align_pairs: float32 or bfloat16 states, got %s" % x.dtype)
    for name, rng in (("x_range", x_range), ("y_range", y_range)):
        if tuple(rng.shape) != (B, 2) or rng.dtype.is_floating_point or rng.dtype == torch.bool:
            raise ValueError("align_pairs: %s must be integer [%d, 2], got %s %s" % (name, B, tuple(rng.shape), rng.dtype))
    _req_cuda(x, y, x_range, y_range)
    dev = x.device
    link = torch.full((B, S), -1, device=dev, dtype=torch.int32)
    fwd_idx = torch.full((B, S), -1, device=dev, dtype=torch.int32)
    fwd_val = torch.full((B, S), float("-inf"), device=dev, dtype=torch.float32)
    bwd_idx = torch.full((B, T), -1, device=dev, dtype=torch.int32)
    bwd_val = torch.full((B, T), float("-inf"), device=dev, dtype=torch.float32)
    if B > 0:
        x, y = _align_operand(x), _align_operand(y)
        dp = x.shape[2]
        lib = L.load()
        if not lib.imt_align_supported(dt(x), dp):
            raise L.ImtError("align_pairs: (dtype %s, d %d) is not taken by imt_align_pairs" % (x.dtype, dp))
        lim = torch.iinfo(torch.int32)
        xr = x_range.clamp(lim.min, lim.max).to(torch.int32).contiguous()
        yr = y_range.clamp(lim.min, lim.max).to(torch.int32).contiguous()
        a = L.AlignArgs()
        a.dtype, a.B, a.S, a.T, a.d = dt(x), B, S, T, dp
        a.x, a.ldx = x.data_ptr(), x.stride(1) if S > 1 else dp
        a.bsx = x.stride(0) if B > 1 else (S - 1) * a.ldx + dp
        a.y, a.ldy = y.data_ptr(), y.stride(1) if T > 1 else dp
        a.bsy = y.stride(0) if B > 1 else (T - 1) * a.ldy + dp
        a.xr, a.yr = xr.data_ptr(), yr.data_ptr()
        a.min_sim = float(min_sim)
        a.link, a.fwd_idx, a.fwd_val = link.data_ptr(), fwd_idx.data_ptr(), fwd_val.data_ptr()
        a.bwd_idx, a.bwd_val = bwd_idx.data_ptr(), bwd_val.data_ptr()
        L.check(lib.imt_align_pairs(ctypes.byref(a), _stream()), "imt_align_pairs")
    return link.long(), fwd_idx.long(), fwd_val, bwd_idx.long(), bwd_val


def conv_out_size(size, kernel, stride, pad):
    return (size + 2 * pad - kernel) // stride + 1


def conv2d_nhwc(x, w, *, stride=1, pad=0, scale=None, shift=None, residual=None, relu=False, out=None):
    """y [B, Ho, Wo, Cout] = epilogue(conv(x [B, H, W, Cin], w [Cout, KH, KW, Cin])) on MFMA (include/imt_hip.h: imt_conv2d):
    ``acc * scale + shift`` (fp32 [Cout]), ``+ residual`` (y's shape and type), ReLU.  ``pad``: int or (pad_h, pad_w).  x, w,
    residual and ``out`` are dense (contiguous) tensors of one dtype."""
    if x.dim() != 4 or w.dim() != 4 or x.shape[3] != w.shape[3] or x.dtype != w.dtype:
        raise ValueError("conv2d_nhwc: x %s %s against w %s %s" % (tuple(x.shape), x.dtype, tuple(w.shape), w.dtype))
    _req_cuda(x, w, scale, shift, residual, out)
    B, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    pad_h, pad_w = (pad, pad) if isinstance(pad, int) else pad
    Ho, Wo = conv_out_size(H, KH, stride, pad_h), conv_out_size(W, KW, stride, pad_w)
    shape = (B, max(Ho, 0), max(Wo, 0), Cout)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=x.dtype)
    for name, t, want, dtype in (("x", x, tuple(x.shape), x.dtype), ("w", w, tuple(w.shape), x.dtype), ("out", out, shape, x.dtype),
                                 ("residual", residual, shape, x.dtype), ("scale", scale, (Cout,), torch.float32),
                                 ("shift", shift, (Cout,), torch.float32)):
        if t is not None and (tuple(t.shape) != want or t.dtype != dtype or not t.is_contiguous()):
            raise ValueError("conv2d_nhwc: %s must be contiguous %s %s, got %s %s" % (name, want, dtype, tuple(t.shape), t.dtype))
    a = L.ConvArgs()
    a.dtype = dt(x)
    a.B, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW = B, H, W, Cin, Cout, KH, KW
    a.stride, a.pad_h, a.pad_w, a.relu = stride, pad_h, pad_w, int(bool(relu))
    a.x, a.w, a.y = x.data_ptr(), w.data_ptr(), out.data_ptr()
    a.scale = scale.data_ptr() if scale is not None else None
    a.shift = shift.data_ptr() if shift is not None else None
    a.residual = residual.data_ptr() if residual is not None else None
    L.check(L.load().imt_conv2d(ctypes.byref(a), _stream()), "imt_conv2d")
    return out


def maxpool2d_nhwc(x):
    """3 x 3, stride 2, padding 1 max pool of x [B, H, W, C] (NHWC, C % 8 == 0); padding counts as -inf."""
    if x.dim() != 4:
        raise ValueError("maxpool2d_nhwc: x must be [B, H, W, C], got %s" % (tuple(x.shape),))
    _req_cuda(x)
    x = x.contiguous()
    B, H, W, C = x.shape
    out = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), device=x.device, dtype=x.dtype)
    L.check(L.load().imt_maxpool2d_3x3s2(dt(x), _p(x), _p(out), B, H, W, C, _stream()), "imt_maxpool2d_3x3s2")
    return out


IMAGE_MEAN, IMAGE_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)  # transforms.Normalize of src/dataset.py:286-288


def image_to_nhwc(img, dtype=torch.float32, mean=IMAGE_MEAN, std=IMAGE_STD):
    """uint8 [B, H, W, 3] decoded images -> [B, H, W, 8] network input: (v / 255 - mean) / std in channels 0-2, zeros in 3-7."""
    if img.dim() != 4 or img.shape[3] != 3 or img.dtype != torch.uint8:
        raise ValueError("image_to_nhwc: uint8 [B, H, W, 3] expected, got %s %s" % (tuple(img.shape), img.dtype))
    _req_cuda(img)
    img = img.contiguous()
    B, H, W, _ = img.shape
    out = torch.empty((B, H, W, 8), device=img.device, dtype=dtype)
    m, s = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    L.check(L.load().imt_image_nhwc(dt(out), _p(img), _p(out), B, H, W, m, s, _stream()), "imt_image_nhwc")
    return out


def log_softmax_bwd(dlp, lp, out_dtype):
    _req_cuda(dlp, lp)
    N, V = lp.shape
    out = alloc_rows(N, V, out_dtype, lp.device)
    lp, dlp = rows16(lp), rows16(dlp)
    L.check(L.load().imt_log_softmax_bwd(_p(dlp), dlp.stride(0) if N else V, _p(lp), lp.stride(0) if N else V, dt(out), _p(out),
                                         out.stride(0) if N else V, N, V, _stream()),
            "imt_log_softmax_bwd")
    return out


def smoothed_nll_fwd(lp, target, epsilon, ignore_index):
    _req_cuda(lp, target)
    N, V = lp.shape
    loss = torch.empty((N, 1), device=lp.device, dtype=torch.float32)
    L.check(L.load().imt_smoothed_nll_fwd(_p(lp), _rowmajor(lp) if N else V, _p(target), _p(loss), N, V, epsilon,
                                          ignore_index, _stream()), "imt_smoothed_nll_fwd")
    return loss


def smoothed_nll_bwd(dloss, target, V, epsilon, ignore_index):
    _req_cuda(dloss, target)
    N = target.numel()
    dlp = alloc_rows(N, V, torch.float32, dloss.device)
    L.check(L.load().imt_smoothed_nll_bwd(_p(dloss), _p(target), _p(dlp), dlp.stride(0) if N else V, N, V, epsilon, ignore_index, _stream()),
            "imt_smoothed_nll_bwd")
    return dlp


def xent_fused_fwd_bwd(logits, target, epsilon, ignore_index, grad_scale):
    """In place: logits <- dlogits; returns per-row loss."""
    _req_cuda(logits, target)
    N, V = logits.shape
    loss = torch.empty(N, device=logits.device, dtype=torch.float32)
    L.check(L.load().imt_xent_fused_fwd_bwd(dt(logits), _p(logits), _rowmajor(logits) if N else V, _p(target), _p(loss), N, V,
                                            epsilon, ignore_index, grad_scale, _stream()), "imt_xent_fused_fwd_bwd")
    return loss


def scaled_sum(x, scale: float):
    """scale * x.sum() as a 0-d fp32 tensor (one small deterministic kernel)."""
    _req_cuda(x)
    out = torch.empty((), device=x.device, dtype=torch.float32)
    src = x if x.numel() else out  # an empty tensor has no address (the C side refuses NULL); with n = 0 nothing is read
    L.check(L.load().imt_scaled_sum(_p(src), x.numel(), float(scale), _p(out), _stream()), "imt_scaled_sum")
    return out


def sumsq(g, out, ws=None):
    _req_cuda(g, out, ws)
    if ws is None:
        ws = torch.empty(1024, device=g.device, dtype=torch.float32)  # IMT_SUMSQ_WS_FLOATS
    L.check(L.load().imt_sumsq(_p(g), g.numel(), _p(out), _p(ws), _stream()), "imt_sumsq")
    return out


def clip_adam(p, g, m, v, p_bf16, sumsq_t, max_norm, grad_scale, lr, beta1, beta2, eps, step, zero_grad=True):
    _req_cuda(p, g, m, v)
    L.check(L.load().imt_clip_adam(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), p.numel(), _p(sumsq_t), max_norm, grad_scale,
                                   lr, beta1, beta2, eps, step, int(zero_grad), _stream()), "imt_clip_adam")


def clip_scale(g, sumsq_t, max_norm, grad_scale=1.0):
    """g *= grad_scale * min(1, max_norm / (grad_scale * sqrt(sumsq) + 1e-6)), in place (imt_clip_scale)."""
    _req_cuda(g, sumsq_t)
    L.check(L.load().imt_clip_scale(_p(g), g.numel(), _p(sumsq_t), max_norm, grad_scale, _stream()), "imt_clip_scale")
    return g


def cast_f32_to_bf16(src, dst):
    _req_cuda(src, dst)
    L.check(L.load().imt_cast_f32_to_bf16(_p(src), _p(dst), src.numel(), _stream()), "imt_cast_f32_to_bf16")
    return dst


def gated_mix(a, b, gate):
    _req_cuda(a, b, gate)
    out = torch.empty_like(a)
    L.check(L.load().imt_gated_mix(dt(a), _p(a), _p(b), _p(gate), _p(out), a.shape[0], a.shape[1], _stream()), "imt_gated_mix")
    return out


OBJ_FEAT_DIM, OBJ_LABELS, GATED_MIX_BWD_PARTS = 1024, 91, 64  # include/imt_hip.h: IMT_OBJ_FEAT_DIM, IMT_OBJ_LABELS, IMT_GATED_MIX_BWD_PARTS


def obj_padded_k(d):
    """Kp of the object head's padded operands: d + 1031 rounded up to 64."""
    return (d + OBJ_FEAT_DIM + 7 + 63) // 64 * 64


def obj_rows(labels, feats, boxes, emb, w, d, dtype, want_w=True, status=None):
    """(X [R, Kp], W_pad [d, Kp] or None) of the object head (imt_obj_rows); labels [R] int64, feats [R, 1024] fp32 / bf16,
    boxes [R, 4] fp32, emb = flat [91 * d] slice, w = flat [d * (d + 1031)] slice, both in `dtype`."""
    _req_cuda(labels, feats, boxes, emb, w, status)
    assert labels.dtype == torch.int64 and boxes.dtype == torch.float32 and feats.shape[-1] == OBJ_FEAT_DIM
    assert labels.is_contiguous() and feats.is_contiguous() and boxes.is_contiguous() and emb.is_contiguous() and w.is_contiguous()
    assert emb.dtype == dtype and w.dtype == dtype and emb.numel() == OBJ_LABELS * d and w.numel() == d * (d + OBJ_FEAT_DIM + 7)
    assert feats.numel() == labels.numel() * OBJ_FEAT_DIM and boxes.numel() == labels.numel() * 4
    assert status is None or (status.dtype == torch.int32 and status.numel() >= 1)
    R = labels.numel()
    Kp = obj_padded_k(d)
    x = torch.empty((R, Kp), device=emb.device, dtype=dtype)
    w_pad = torch.empty((d, Kp), device=emb.device, dtype=dtype) if want_w else None
    L.check(L.load().imt_obj_rows(dt(feats), IMT_F32 if dtype == torch.float32 else IMT_BF16, _p(labels), _p(feats), _p(boxes),
                                  _p(emb), _p(w), _p(x), _p(w_pad), R, d, Kp, _p(status), _stream()), "imt_obj_rows")
    return x, w_pad


def relu_dropout_(y, dropout_p=0.0, dropout_seed=0):
    _req_cuda(y)
    assert y.dim() == 2 and y.is_contiguous()
    L.check(L.load().imt_relu_dropout(dt(y), _p(y), y.shape[0], y.shape[1], float(dropout_p), int(dropout_seed), _stream()),
            "imt_relu_dropout")
    return y


def relu_dropout_bwd(dy, y, dropout_p=0.0, dropout_seed=0):
    _req_cuda(dy, y)
    assert dy.shape == y.shape and dy.dtype == y.dtype and dy.is_contiguous() and y.is_contiguous()
    dz = torch.empty_like(y)
    L.check(L.load().imt_relu_dropout_bwd(dt(y), _p(dy), _p(y), _p(dz), y.shape[0], y.shape[1], float(dropout_p),
                                          int(dropout_seed), _stream()), "imt_relu_dropout_bwd")
    return dz


def obj_fold_w(dw_pad, grad, d):
    _req_cuda(dw_pad, grad)
    assert dw_pad.dtype == torch.float32 and dw_pad.is_contiguous() and dw_pad.shape[0] == d
    assert grad.dtype == torch.float32 and grad.is_contiguous() and grad.numel() == d * (d + OBJ_FEAT_DIM + 7)
    L.check(L.load().imt_obj_fold_w(_p(dw_pad), _p(grad), d, dw_pad.shape[1], _stream()), "imt_obj_fold_w")


def obj_embed_grad(labels, dx, grad):
    _req_cuda(labels, dx, grad)
    R, d = dx.shape
    assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == R
    assert dx.dim() == 2 and dx.stride(1) == 1
    assert grad.dtype == torch.float32 and grad.is_contiguous() and grad.numel() == OBJ_LABELS * d
    L.check(L.load().imt_obj_embed_grad(dt(dx), _p(labels), _p(dx), _rowmajor(dx), _p(grad), R, d, _stream()), "imt_obj_embed_grad")


def gated_mix_bwd(dy, a, b, gate, dgate):
    """(da, db); dgate (fp32 [d]) += the gate's gradient (imt_gated_mix_bwd, deterministic)."""
    _req_cuda(dy, a, b, gate, dgate)
    rows, d = a.shape
    assert dy.shape == a.shape == b.shape and dy.dtype == a.dtype == b.dtype == gate.dtype
    assert dy.is_contiguous() and a.is_contiguous() and b.is_contiguous() and gate.is_contiguous() and gate.numel() == d
    assert dgate.dtype == torch.float32 and dgate.is_contiguous() and dgate.numel() == d
    da, db = torch.empty_like(a), torch.empty_like(b)
    ws = torch.empty((GATED_MIX_BWD_PARTS, d), device=a.device, dtype=torch.float32)
    L.check(L.load().imt_gated_mix_bwd(dt(a), _p(dy), _p(a), _p(b), _p(gate), _p(da), _p(db), _p(dgate), _p(ws), rows, d, _stream()),
            "imt_gated_mix_bwd")
    return da, db


# ------------------------------------------------------------------------------------------- contrastive tail
POOL_MAX_S, POOL_MAX_D, CONTRASTIVE_MAX_N = 4096, 1024, 4096  # include/imt_hip.h: IMT_POOL_MAX_S, IMT_POOL_MAX_D, IMT_CONTRASTIVE_MAX_N


def attn_pool_plan(dtype, S, d):
    """1: a sentence of the pooled tensor stays in LDS (read from memory once), 2: it is read twice (imt_attn_pool_plan)."""
    plan = L.load().imt_attn_pool_plan(IMT_BF16 if dtype == torch.bfloat16 else IMT_F32, int(S), int(d))
    L.check(min(plan, 0), "imt_attn_pool_plan")
    return plan


def _pool_mask(mask, rows, S):
    if mask is None:
        return None
    assert tuple(mask.shape) == (rows, S) and mask.dtype in (torch.bool, torch.uint8)
    mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def attn_pool_fwd(x, w, b, mask=None, out=None):
    """(u [rows, d], probs [rows, S], norm [rows]), all fp32, of the one-vector attention pooling of x [rows, S, d]
    (imt_attn_pool_fwd); w [d] and b [1] in x's dtype, mask [rows, S] bool / uint8 or None; `out`: where u goes."""
    _req_cuda(x, w, b, mask, out)
    rows, S, d = x.shape
    assert x.is_contiguous() and w.is_contiguous() and w.dtype == x.dtype and b.dtype == x.dtype and w.numel() == d and b.numel() == 1
    mask = _pool_mask(mask, rows, S)
    u = out if out is not None else torch.empty((rows, d), device=x.device, dtype=torch.float32)
    assert u.dtype == torch.float32 and u.is_contiguous() and tuple(u.shape) == (rows, d)
    probs = torch.empty((rows, S), device=x.device, dtype=torch.float32)
    norm = torch.empty((rows,), device=x.device, dtype=torch.float32)
    L.check(L.load().imt_attn_pool_fwd(dt(x), _p(x), _p(w), _p(b), _p(mask), _p(u), _p(probs), _p(norm), rows, S, d, _stream()),
            "imt_attn_pool_fwd")
    return u, probs, norm


def attn_pool_bwd(x, w, mask, u, probs, norm, du, dw, db, du_scale=None):
    """dx [rows, S, d] in x's dtype; dw (fp32 [d]) and db (fp32 [1]) += the parameter gradients (imt_attn_pool_bwd,
    deterministic).  du_scale: optional fp32 device scalar multiplied into du (an upstream loss gradient)."""
    _req_cuda(x, w, mask, u, probs, norm, du, dw, db, du_scale)
    rows, S, d = x.shape
    assert x.is_contiguous() and w.is_contiguous() and w.dtype == x.dtype and w.numel() == d
    mask = _pool_mask(mask, rows, S)
    for t, shape in ((u, (rows, d)), (probs, (rows, S)), (norm, (rows,)), (du, (rows, d)), (dw, (d,)), (db, (1,))):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
    assert du_scale is None or (du_scale.dtype == torch.float32 and du_scale.numel() == 1)
    dx = torch.empty_like(x)
    ws = torch.empty((rows * d + rows,), device=x.device, dtype=torch.float32)
    L.check(L.load().imt_attn_pool_bwd(dt(x), _p(x), _p(w), _p(mask), _p(u), _p(probs), _p(norm), _p(du), _p(du_scale), _p(dx), _p(dw),
                                       _p(db), _p(ws), rows, S, d, _stream()), "imt_attn_pool_bwd")
    return dx


def contrastive(img, txt):
    """(loss [1], d_img [B, d], d_txt [N, d]) of the image-to-text contrastive loss over fp32 unit vectors (imt_contrastive);
    text row i < B belongs to image i."""
    _req_cuda(img, txt)
    B, d = img.shape
    N = txt.shape[0]
    assert img.dtype == txt.dtype == torch.float32 and img.is_contiguous() and txt.is_contiguous() and txt.shape[1] == d
    loss = torch.empty((1,), device=img.device, dtype=torch.float32)
    d_img, d_txt = torch.empty_like(img), torch.empty_like(txt)
    ws = torch.empty((B * N + B,), device=img.device, dtype=torch.float32)
    L.check(L.load().imt_contrastive(_p(img), _p(txt), _p(loss), _p(d_img), _p(d_txt), _p(ws), B, N, d, _stream()), "imt_contrastive")
    return loss, d_img, d_txt


# ------------------------------------------------------------------------------------------- lexical proposals
def _proposal_args(x, table, prop, gate, gamma, beta, rows_per_group):
    _req_cuda(x, table, prop, gate, gamma, beta)
    rows, d = x.shape
    rows_per_group = int(rows_per_group)
    assert x.is_contiguous() and table.is_contiguous() and table.dtype == x.dtype and table.dim() == 2 and table.shape[1] == d
    assert prop.dtype == torch.int64 and prop.dim() == 2 and prop.is_contiguous()
    assert rows_per_group >= 1 and prop.shape[0] * rows_per_group == rows, "one row of proposals per group of rows_per_group rows"
    for t in (gate, gamma, beta):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == d)
    return rows, d, int(prop.shape[1]), rows_per_group


def proposal_attn(x, table, prop, gate, gamma, beta, rows_per_group, pad_idx, eps):
    """(y [rows, d] in x's dtype, scores [rows, P] fp32, stats [rows, 4] fp32) of the lexical-proposal attention + gate +
    LayerNorm (imt_proposal_attn_fwd): x [rows, d], table [V, d] in x's dtype, prop [rows / rows_per_group, P] int64,
    gate / gamma / beta fp32 [d]."""
    rows, d, P, rpg = _proposal_args(x, table, prop, gate, gamma, beta, rows_per_group)
    y = torch.empty_like(x)
    scores = torch.empty((rows, P), device=x.device, dtype=torch.float32)
    stats = torch.empty((rows, 4), device=x.device, dtype=torch.float32)
    L.check(L.load().imt_proposal_attn_fwd(dt(x), _p(x), _p(table), _p(prop), _p(gate), _p(gamma), _p(beta), _p(y), _p(scores),
                                           _p(stats), rows, rpg, P, d, int(table.shape[0]), int(pad_idx), float(eps), _stream()),
            "imt_proposal_attn_fwd")
    return y, scores, stats


def proposal_attn_bwd(dy, x, table, prop, gate, gamma, scores, stats, dtable, dgate, dgamma, dbeta, rows_per_group, pad_idx):
    """dx [rows, d] in x's dtype; dtable (fp32 [V, d]), dgate, dgamma, dbeta (fp32 [d]) += the parameter gradients
    (imt_proposal_attn_bwd, deterministic)."""
    rows, d, P, rpg = _proposal_args(x, table, prop, gate, gamma, None, rows_per_group)
    _req_cuda(dy, scores, stats, dtable, dgate, dgamma, dbeta)
    assert dy.dtype == x.dtype and dy.is_contiguous() and dy.shape == x.shape
    for t, shape in ((scores, (rows, P)), (stats, (rows, 4)), (dtable, tuple(table.shape))):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
    for t in (dgate, dgamma, dbeta):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == d
    dx = torch.empty_like(x)
    if rows == 0:
        return dx
    nbytes = int(L.load().imt_proposal_attn_ws_bytes(rows, rpg, P, d))
    L.check(min(nbytes, 0), "imt_proposal_attn_ws_bytes")
    ws = torch.empty((nbytes,), device=x.device, dtype=torch.uint8)
    L.check(L.load().imt_proposal_attn_bwd(dt(x), _p(dy), _p(x), _p(table), _p(prop), _p(gate), _p(gamma), _p(scores), _p(stats),
                                           _p(dx), _p(dtable), _p(dgate), _p(dgamma), _p(dbeta), _p(ws), nbytes, rows, rpg, P, d,
                                           int(table.shape[0]), int(pad_idx), _stream()), "imt_proposal_attn_bwd")
    return dx


# ------------------------------------------------------------------------------------------- Caption2Image tail
L2_DIST_PARTS = 256  # include/imt_hip.h: IMT_L2_DIST_PARTS


def sent_pool_fwd(x, w, b, mask=None, dropout_p=0.0, dropout_seed=0):
    """(v [rows, d] in x's dtype, probs [rows, S] fp32) of the sentence pooling of dropout(x), x [rows, S, d]
    (imt_sent_pool_fwd); w [d] and b [1] in x's dtype, mask [rows, S] bool / uint8 or None.  The dropout keeps what
    ``add_rows_dropout`` keeps of the flattened [rows * S, d] tensor under the same seed."""
    _req_cuda(x, w, b, mask)
    rows, S, d = x.shape
    assert x.is_contiguous() and w.is_contiguous() and w.dtype == x.dtype and b.dtype == x.dtype and w.numel() == d and b.numel() == 1
    mask = _pool_mask(mask, rows, S)
    v = torch.empty((rows, d), device=x.device, dtype=x.dtype)
    probs = torch.empty((rows, S), device=x.device, dtype=torch.float32)
    L.check(L.load().imt_sent_pool_fwd(dt(x), _p(x), _p(w), _p(b), _p(mask), _p(v), _p(probs), rows, S, d, float(dropout_p),
                                       int(dropout_seed), _stream()), "imt_sent_pool_fwd")
    return v, probs


def sent_pool_bwd(x, w, mask, probs, dv, dw, db, dropout_p=0.0, dropout_seed=0):
    """dx [rows, S, d] in x's dtype; dw (fp32 [d]) and db (fp32 [1]) += the parameter gradients (imt_sent_pool_bwd,
    deterministic); dv [rows, d] in x's dtype, the dropout mask is regenerated from the seed."""
    _req_cuda(x, w, mask, probs, dv, dw, db)
    rows, S, d = x.shape
    assert x.is_contiguous() and w.is_contiguous() and w.dtype == x.dtype and w.numel() == d
    assert dv.dtype == x.dtype and dv.is_contiguous() and tuple(dv.shape) == (rows, d)
    mask = _pool_mask(mask, rows, S)
    for t, shape in ((probs, (rows, S)), (dw, (d,)), (db, (1,))):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
    dx = torch.empty_like(x)
    ws = torch.empty((rows * d + rows,), device=x.device, dtype=torch.float32)
    L.check(L.load().imt_sent_pool_bwd(dt(x), _p(x), _p(w), _p(mask), _p(probs), _p(dv), _p(dx), _p(dw), _p(db), _p(ws), rows, S, d,
                                       float(dropout_p), int(dropout_seed), _stream()), "imt_sent_pool_bwd")
    return dx


def l2_dist(pred, target):
    """(loss [1] fp32, dpred like pred): |pred - target|_2 / B over [B, n] tensors of one dtype and its gradient with respect
    to pred, from one call (imt_l2_dist); the gradient is all zeros where the distance is 0."""
    _req_cuda(pred, target)
    assert pred.dim() == 2 and pred.shape == target.shape and pred.dtype == target.dtype
    assert pred.is_contiguous() and target.is_contiguous()
    B, n = pred.shape
    loss = torch.empty((1,), device=pred.device, dtype=torch.float32)
    dpred = torch.empty_like(pred)
    ws = torch.empty((L2_DIST_PARTS,), device=pred.device, dtype=torch.float32)
    L.check(L.load().imt_l2_dist(dt(pred), _p(pred), _p(target), _p(loss), _p(dpred), _p(ws), B, n, _stream()), "imt_l2_dist")
    return loss, dpred


# ------------------------------------------------------------------------------------------- SenSim tail
def sensim_loss(scat, tcat, B):
    """(loss [1], d_scat [Ns, d], d_tcat [Nt, d]) of the two-sided contrastive loss over fp32 unit vectors (imt_sensim_loss);
    the last B rows of scat / tcat are the sentence pairs, the rows before them each side's negatives."""
    _req_cuda(scat, tcat)
    Ns, d = scat.shape
    Nt = tcat.shape[0]
    B = int(B)
    assert scat.dtype == tcat.dtype == torch.float32 and scat.is_contiguous() and tcat.is_contiguous() and tcat.shape[1] == d
    loss = torch.empty((1,), device=scat.device, dtype=torch.float32)
    d_scat, d_tcat = torch.empty_like(scat), torch.empty_like(tcat)
    ws = torch.empty((max(B, 0) * (Ns + Nt + 2 * d + 1),), device=scat.device, dtype=torch.float32)
    L.check(L.load().imt_sensim_loss(_p(scat), _p(tcat), _p(loss), _p(d_scat), _p(d_tcat), _p(ws), B, Ns, Nt, d, _stream()),
            "imt_sensim_loss")
    return loss, d_scat, d_tcat


def pair_dot(a, b):
    """out [rows] fp32: out_r = a_r . b_r over fp32 [rows, d] tensors (imt_pair_dot)."""
    _req_cuda(a, b)
    assert a.dim() == 2 and a.shape == b.shape and a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous()
    rows, d = a.shape
    out = torch.empty((rows,), device=a.device, dtype=torch.float32)
    L.check(L.load().imt_pair_dot(_p(a), _p(b), _p(out), rows, d, _stream()), "imt_pair_dot")
    return out


def pair_dot_bwd(a, b, g):
    """(da, db) = (g_r b_r, g_r a_r) for an upstream g [rows] fp32 (imt_pair_dot_bwd)."""
    _req_cuda(a, b, g)
    assert a.dim() == 2 and a.shape == b.shape and a.dtype == b.dtype == g.dtype == torch.float32
    assert a.is_contiguous() and b.is_contiguous() and g.is_contiguous() and tuple(g.shape) == (a.shape[0],)
    rows, d = a.shape
    da, db = torch.empty_like(a), torch.empty_like(b)
    L.check(L.load().imt_pair_dot_bwd(_p(a), _p(b), _p(g), _p(da), _p(db), rows, d, _stream()), "imt_pair_dot_bwd")
    return da, db


def add_rows_dropout(x, add=None, out_dtype=None, dropout_p=0.0, dropout_seed=0):
    """out[r, :] = dropout(x[r, :] + add[r % add.shape[0], :]) for a 2-D x (imt_add_rows_dropout); add may be None."""
    _req_cuda(x, add)
    assert x.dim() == 2 and x.is_contiguous()
    out_dtype = out_dtype or x.dtype
    out = torch.empty(x.shape, device=x.device, dtype=out_dtype)
    if add is not None:
        assert add.dtype == out_dtype and add.is_contiguous() and add.shape[1] == x.shape[1]
    L.check(L.load().imt_add_rows_dropout(dt(x), _p(x), dt(out), _p(out), _p(add), x.shape[0], x.shape[1],
                                          add.shape[0] if add is not None else 1, float(dropout_p), int(dropout_seed), _stream()),
            "imt_add_rows_dropout")
    return out


# ------------------------------------------------------------------------------------------- incremental decoding
def attention_decode(q, k_base, v_base, n_keys, heads, *, ld_row, ld_pos, rep=1, slots=None, key_mask=None, ldq=None,
                     rows=None, scale=None):
    """Single-query attention against a (slot-addressed) K/V cache; see include/imt_hip.h:imt_attention_decode.
    ``k_base`` / ``v_base`` are tensors whose data_ptr is the (row 0, position 0, head 0) element."""
    _req_cuda(q, k_base, v_base, slots, key_mask)
    R = rows if rows is not None else q.shape[0]
    d = q.shape[-1]
    a = L.AttnDecodeArgs()
    a.dtype, a.R, a.H, a.head_dim, a.n_keys, a.rep = dt(q), R, heads, d // heads, n_keys, rep
    a.Q, a.ldq = q.data_ptr(), (ldq if ldq is not None else q.stride(0))
    a.K, a.V, a.ld_row, a.ld_pos = k_base.data_ptr(), v_base.data_ptr(), ld_row, ld_pos
    if slots is not None:
        assert slots.dtype == torch.int32
        a.slots, a.ld_slots = slots.data_ptr(), slots.stride(0)
    if key_mask is not None:
        assert key_mask.dtype == torch.uint8
        a.key_mask, a.ld_mask = key_mask.data_ptr(), key_mask.stride(0)
    out = torch.empty((R, d), device=q.device, dtype=q.dtype)
    a.O, a.ldo = out.data_ptr(), d
    a.scale = scale if scale is not None else 1.0 / math.sqrt(d // heads)
    L.check(L.load().imt_attention_decode(ctypes.byref(a), _stream()), "imt_attention_decode")
    return out


def beam_step(args: "L.BeamArgs"):
    L.check(L.load().imt_beam_step(ctypes.byref(args), _stream()), "imt_beam_step")


def sample_step(args: "L.SampleArgs"):
    L.check(L.load().imt_sample_step(ctypes.byref(args), _stream()), "imt_sample_step")


def select_plan(mask, ids, col0: int = 1, count=None):
    """(idx int32 [n], targets int64 [n]) of the positions with mask[b, col0 + t] set; ONE small kernel + one 4-byte
    device->host read (the row count shapes everything downstream, so this is the step's only synchronisation).
    `count`: the number of set positions when the caller already knows it on the host (a data loader builds the masks on
    the CPU) -- no read-back, the step is then enqueued without any synchronisation.  It MUST equal
    mask[:, col0:].sum(); IMT_CHECK_COUNT=1 verifies it (with the read-back)."""
    _req_cuda(mask, ids)
    B, T = ids.shape
    T1 = T - col0
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8) if mask.is_contiguous() else mask.contiguous().view(torch.uint8)
    assert mask.dtype == torch.uint8 and mask.stride(1) == 1 and ids.stride(1) == 1 and ids.dtype == torch.int64
    n = B * max(T1, 0)
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=ids.device)
    targets = torch.empty(max(n, 1), dtype=torch.int64, device=ids.device)
    count_dev = torch.empty(1, dtype=torch.int32, device=ids.device)
    if n == 0:
        return idx[:0], targets[:0]
    L.check(L.load().imt_select_plan(_p(mask), mask.stride(0), _p(ids), ids.stride(0), B, T1, col0, _p(idx), _p(targets), _p(count_dev),
                                     _stream()), "imt_select_plan")
    if count is None or os.environ.get("IMT_CHECK_COUNT"):
        k = int(count_dev.item())
        if count is not None and int(count) != k:
            raise L.ImtError("select_plan: count hint %d but the mask selects %d positions" % (int(count), k))
    else:
        k = int(count)
    return idx[:k], targets[:k]
