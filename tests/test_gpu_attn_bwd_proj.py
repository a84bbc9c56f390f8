"""imt_attention_bwd_proj: the attention backward that forms dO = dy W_o itself, against the pair it replaces (imt_gemm NN
into a dO buffer, then imt_attention_bwd) on the same inputs.  Both run the same MFMA accumulation order (fp32 over ascending
32-element k-steps, one rounding to bf16) and the same attention code, so dQ / dK / dV and the optionally stored dO must be
BIT-identical."""
import pytest
import torch

DH = 64
B = 2
SHAPES = [(65, 65), (127, 128), (128, 128), (128, 70)]  # ragged rows, the cross-attention shape, a full tile, ragged keys
MASKS = ["causal", "key", "query", "none"]


def _kinds(fn):
    from imagetranslate_amd import _lib as L
    lib = L.load()
    torch.cuda.synchronize()
    lib.imt_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        rows = (L.ProfRow * 64)()
        kinds = {rows[i].kind.decode(): int(rows[i].launches) for i in range(lib.imt_prof_report(rows, 64))}
    finally:
        lib.imt_prof_enable(0)
    return out, kinds


def _inputs(H, Tq, Tk, pad=0):
    g = torch.Generator().manual_seed(1000 * H + 10 * Tq + Tk)
    d = H * DH

    def mk(rows, cols, scale, ld=None):
        buf = (torch.randn(rows, ld or cols, generator=g) * scale).bfloat16().cuda()
        return buf[:, :cols]

    q, k, v = mk(B * Tq, d, 0.8), mk(B * Tk, d, 0.8), mk(B * Tk, d, 0.8)
    dy = mk(B * Tq, d, 0.5, d + pad)  # pad != 0: a leading dimension wider than d_model, other values behind each row
    w_o = mk(d, d, 0.06)
    klen = torch.randint(Tk // 2, Tk + 1, (B,), generator=g)
    kmask = (torch.arange(Tk)[None] < klen[:, None]).to(torch.uint8).cuda()
    qmask = (torch.rand(B, Tq, generator=g) > 0.15).to(torch.uint8).cuda()
    return q, k, v, dy, w_o, kmask, qmask


def _both(H, Tq, Tk, mask, drop, inp):
    from imagetranslate_amd import hip_ops as O
    q, k, v, dy, w_o, kmask, qmask = inp
    d = H * DH
    kw = dict(key_mask=kmask if mask == "key" else None, query_mask=qmask if mask == "query" else None, causal=mask == "causal",
              dropout_p=drop, dropout_seed=4242)
    o, lse = O.attention_fwd(q, k, v, B, H, Tq, Tk, DH, **kw)
    do_ref = O.gemm(dy, w_o, O.IMT_NN)
    ref, kinds_ref = _kinds(lambda: O.attention_bwd(do_ref, q, k, v, o, lse, B, H, Tq, Tk, DH, **kw))
    assert kinds_ref == {"attn_bwd_fused_bf16": 1}, kinds_ref
    do_out = torch.full((B * Tq, d), float("nan"), dtype=torch.bfloat16, device="cuda")
    # one launch, no GEMM; it is profiled under the kind of the kernel it is an instance of
    got, kinds = _kinds(lambda: O.attention_bwd_proj(dy, w_o, q, k, v, o, lse, B, H, Tq, Tk, DH, do_out=do_out, **kw))
    assert kinds == {"attn_bwd_fused_bf16": 1}, kinds
    got_nostore = O.attention_bwd_proj(dy, w_o, q, k, v, o, lse, B, H, Tq, Tk, DH, **kw)
    return do_ref, ref, do_out, got, got_nostore


def _assert_identical(tag, do_ref, ref, do_out, got, got_nostore):
    assert torch.equal(do_out.view(torch.int16), do_ref.view(torch.int16)), \
        "%s: dO differs from the GEMM's (max %g)" % (tag, float((do_out.float() - do_ref.float()).abs().max()))
    for name, a, b_, c in zip(("dQ", "dK", "dV"), got, ref, got_nostore):
        assert torch.isfinite(b_.float()).all(), "%s: %s of the pair is not finite" % (tag, name)
        assert torch.equal(a.view(torch.int16), b_.view(torch.int16)), \
            "%s: %s differs (max %g)" % (tag, name, float((a.float() - b_.float()).abs().max()))
        assert torch.equal(c.view(torch.int16), b_.view(torch.int16)), "%s: %s differs when dO is not stored" % (tag, name)


@pytest.mark.gpu
@pytest.mark.parametrize("Tq,Tk", SHAPES)
@pytest.mark.parametrize("H", [2, 8])  # d_model 128 and 512: one and two chunks of the W_o staging, more than one head offset
def test_bwd_proj_is_bit_identical_to_gemm_plus_bwd(cuda, H, Tq, Tk):
    inp = _inputs(H, Tq, Tk)
    for mask in MASKS:
        for drop in (0.0, 0.1):
            _assert_identical("H=%d Tq=%d Tk=%d %s p=%g" % (H, Tq, Tk, mask, drop), *_both(H, Tq, Tk, mask, drop, inp))


@pytest.mark.gpu
def test_bwd_proj_with_a_padded_leading_dimension_of_dy(cuda):
    H, Tq, Tk = 8, 127, 128
    _assert_identical("lddy = d + 24", *_both(H, Tq, Tk, "key", 0.1, _inputs(H, Tq, Tk, pad=24)))


def test_bwd_proj_supported_shapes():
    from imagetranslate_amd import _lib as L
    sup = L.load().imt_attention_bwd_proj_supported
    assert sup(L.IMT_BF16, 64, 8, 128, 128, 512, 0) == 1
    assert sup(L.IMT_BF16, 64, 12, 128, 70, 768, 0) == 1
    assert sup(L.IMT_F32, 64, 8, 128, 128, 512, 0) == 0
    assert sup(L.IMT_BF16, 32, 8, 128, 128, 256, 0) == 0
    assert sup(L.IMT_BF16, 64, 8, 129, 128, 512, 0) == 0
    assert sup(L.IMT_BF16, 64, 8, 128, 129, 512, 0) == 0
    assert sup(L.IMT_BF16, 64, 8, 128, 128, 576, 0) == 0  # d_model != 64 H
    assert sup(L.IMT_BF16, 64, 8, 128, 128, 512, 1) == 0  # explicit [B, Tq, Tk] mask: the pair
    # the fused backward switched off: the instance this one is a variant of is not in use
    import os
    os.environ["IMT_ATTN_NO_FUSED_BWD"] = "1"
    try:
        assert sup(L.IMT_BF16, 64, 8, 128, 128, 512, 0) == 0
    finally:
        os.environ.pop("IMT_ATTN_NO_FUSED_BWD", None)
    assert sup(L.IMT_BF16, 64, 8, 128, 128, 512, 0) == 1


@pytest.mark.gpu
def test_bwd_proj_rejects_an_unsupported_call(cuda):
    from imagetranslate_amd import _lib as L
    from imagetranslate_amd import hip_ops as O
    H, T = 2, 64
    g = torch.Generator().manual_seed(5)
    x = [(torch.randn(B * T, H * 32, generator=g)).bfloat16().cuda() for _ in range(4)]
    w = torch.randn(H * 32, H * 32, generator=g).bfloat16().cuda()
    o, lse = O.attention_fwd(x[0], x[1], x[2], B, H, T, T, 32)
    with pytest.raises(L.ImtError):
        O.attention_bwd_proj(x[3], w, x[0], x[1], x[2], o, lse, B, H, T, T, 32)


@pytest.mark.gpu
def test_stack_backward_takes_the_fused_entry_only_where_supported(cuda):
    """Toy stacks with d = 128: head_dim 64 (supported) and head_dim 32 (not: the GEMM + backward pair).  Both run the same
    products, except that the pair has one NN launch (d_dense W_o) in front of each attention backward."""
    from imagetranslate_amd.seq2seq import Seq2Seq
    from imagetranslate_amd.textprocessor import SyntheticTextProcessor
    g = torch.Generator().manual_seed(1)
    Bm, S, T = 4, 24, 20
    src = torch.randint(6, 1000, (Bm, S), generator=g)
    tgt = torch.randint(6, 1000, (Bm, T), generator=g)
    src[0, 18:] = 0
    tgt[1, 15:] = 0
    args = (src, tgt, src != 0, tgt != 0, torch.zeros(Bm, dtype=torch.long), torch.ones(Bm, dtype=torch.long))
    n_attn = 2 + 2 * 2  # encoder self, decoder self + cross
    nn_launches = {}
    for heads in (2, 4):
        torch.manual_seed(0)
        m = Seq2Seq(SyntheticTextProcessor(1000), lang_dec=False, enc_layer=2, dec_layer=2, embed_dim=128, intermediate_dim=512,
                    num_attention_heads=heads).cuda().eval()
        m.set_compute_dtype(torch.bfloat16)

        def run():
            loss, _ = m.loss_fused(*args)
            loss.backward()
            return loss

        loss, kinds = _kinds(run)
        assert torch.isfinite(loss.detach()).all()
        assert kinds.get("attn_bwd_fused_bf16") == n_attn, kinds
        nn_launches[heads] = sum(v for k, v in kinds.items() if k.startswith("gemm_") and k.endswith("_nn"))
        for name, p in m.named_parameters():
            if "attention.self.query.weight" in name:
                assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, name
    assert nn_launches[4] - nn_launches[2] == n_attn, nn_launches
