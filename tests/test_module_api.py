"""CPU tests of the host-side mirror of the reference's module API: parameter names / shapes (checkpoint
compatibility), weight topology, flat-store layout, constructor errors.  No kernels run."""
import pytest
import torch

from oracle import reference_model as R


def _ours(cls="Seq2Seq", **kw):
    import imagetranslate_amd.seq2seq as S
    import imagetranslate_amd.image_model as I
    c = {"Seq2Seq": S.Seq2Seq, "ImageMassSeq2Seq": I.ImageMassSeq2Seq, "ImageCaptioning": I.ImageCaptioning}[cls]
    return c(R.SyntheticTextProcessor(1000), **kw)


@pytest.mark.parametrize("kw", [dict(lang_dec=False, enc_layer=2, dec_layer=2), dict(lang_dec=False, enc_layer=2, dec_layer=1),
                                dict(lang_dec=True, enc_layer=2, dec_layer=1), dict(lang_dec=False, tie_embed=True, enc_layer=1, dec_layer=1),
                                dict(lang_dec=True, tie_embed=True, enc_layer=1, dec_layer=1)])
def test_state_dict_keys_and_shapes_match_oracle(kw):
    kw = dict(kw, embed_dim=64, intermediate_dim=128, num_attention_heads=4)
    ref = R.Seq2Seq(R.SyntheticTextProcessor(1000), **kw)
    ours = _ours(**kw)
    a, b = ref.state_dict(), ours.state_dict()
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert a[k].shape == b[k].shape, k
    # same sharing pattern (which keys alias the same storage)
    def groups(sd):
        by = {}
        for k, v in sd.items():
            by.setdefault(v.data_ptr(), []).append(k)
        return sorted(sorted(v) for v in by.values() if len(v) > 1)
    assert groups(a) == groups(b)
    ours.load_state_dict(a)  # strict


def test_weight_topology_and_attributes():
    m = _ours(lang_dec=False, enc_layer=2, dec_layer=2, embed_dim=64, intermediate_dim=128, num_attention_heads=4)
    assert m.decoder.decoder.layer[0].attention is m.encoder.encoder.layer[0].attention
    assert m.encoder.embeddings.word_embeddings.weight is m.decoder.embeddings.word_embeddings.weight
    assert m.encoder.embeddings.position_embeddings.num_embeddings == 512          # seq_gen.py:114
    assert m.config.vocab_size == 1000 and m.config.hidden_size == 64               # seq_gen.py:128
    assert hasattr(m.decoder.decoder.layer[0], "crossattention")
    assert not hasattr(m.encoder.encoder.layer[0], "crossattention")
    assert isinstance(m.output_layer, torch.nn.ModuleList) and len(m.output_layer) == 2
    assert m.lang_dec is False and m.tie_embed is False and m.use_proposals is False


def test_heads_must_divide_hidden():
    with pytest.raises(ValueError):
        _ours(embed_dim=512, intermediate_dim=1024, enc_layer=1, dec_layer=1)  # reference default 12 heads, 512 % 12 != 0


def test_flat_store_layout_on_cpu():
    from imagetranslate_amd.param_store import store_of
    m = _ours(lang_dec=False, enc_layer=2, dec_layer=2, embed_dim=64, intermediate_dim=128, num_attention_heads=4)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    st = store_of(m.encoder).ensure()
    assert st is store_of(m.decoder)
    assert st.valid() and len(st.entries) == len(list(m.parameters()))
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    a = m.encoder.encoder.layer[1].attention.self
    off = st.offset(a.query.weight)
    assert st.offset(a.key.weight) == off + 64 * 64 and st.offset(a.value.weight) == off + 2 * 64 * 64
    assert st.offset(a.key.bias) == st.offset(a.query.bias) + 64
    assert all(o % 64 == 0 for _, o, _ in st.entries)
    # gradient views alias the flat gradient buffer; zero_grad keeps them
    p = m.output_layer[0].layer.weight
    st.grad.fill_(1.0)
    assert float(p.grad.sum()) == p.numel()
    m.zero_grad()
    assert float(st.grad.abs().sum()) == 0 and p.grad is not None
    # in-place edits of a parameter land in the flat master
    with torch.no_grad():
        p.fill_(3.0)
    assert float(st.flat[st.offset(p)]) == 3.0


def test_image_models_construct_without_network():
    m = _ours("ImageMassSeq2Seq", enc_layer=1, dec_layer=1, embed_dim=64, intermediate_dim=128, num_attention_heads=4,
              resnet_depth=3)
    assert m.image_model.fc.in_features == 2048 and m.image_model.fc.bias is None
    assert m.image_model.location_embedding.num_embeddings == 49
    c = _ours("ImageCaptioning", enc_layer=1, dec_layer=1, embed_dim=64, intermediate_dim=128, num_attention_heads=4)
    assert hasattr(c, "obj_decoder") and hasattr(c, "multistream_attention_gate")


def test_optimizer_lr_schedule_matches_oracle():
    from imagetranslate_amd.utils import AdamInverseSqrtWithWarmup
    p = torch.nn.Parameter(torch.zeros(3))
    opt = AdamInverseSqrtWithWarmup([p], lr=1e-4, betas=(0.9, 0.98), warmup_updates=5)
    for t in [0, 1, 4, 5, 6, 100, 10 ** 6]:
        assert opt.get_lr_for_step(t) == pytest.approx(R.inverse_sqrt_lr(t, 1e-4, 5))
    assert opt.param_groups[0]["lr"] == 1e-7


def _small(**kw):
    return _ours(**dict(dict(lang_dec=False, enc_layer=2, dec_layer=2, embed_dim=64, intermediate_dim=128, num_attention_heads=4), **kw))


def test_flat_store_typed_views():
    from imagetranslate_amd._lib import ImtError
    from imagetranslate_amd.param_store import store_of
    m = _small()
    st = store_of(m.encoder).ensure()
    lin = m.output_layer[1].layer
    w, b, none = st.views(torch.float32, lin.weight, lin.bias, None)
    assert none is None
    for v, p in ((w, lin.weight), (b, lin.bias)):
        assert v.shape == p.shape and v.dtype == torch.float32
        assert v.data_ptr() == st.flat.data_ptr() + 4 * st.offset(p) == p.data_ptr()
    for p in m.parameters():
        g = st.grad_view(p)
        assert g.shape == p.shape and g.data_ptr() == p.grad.data_ptr() == st.grad.data_ptr() + 4 * st.offset(p)
    for lyr in list(m.encoder.encoder.layer) + list(m.decoder.decoder.layer):
        ps = lyr.ordered_params()
        assert st.span(ps) == (min(st.offset(p) for p in ps), max(st.offset(p) + p.numel() for p in ps))
        assert st.span(iter(ps)) == st.span(ps)
    assert st.span([lin.bias]) == (st.offset(lin.bias), st.offset(lin.bias) + 1000)
    with torch.no_grad():
        assert st.anchor_if_grad() is None
    assert st.anchor_if_grad() is st.anchor() and st.anchor().requires_grad
    version = st.layout_version
    st.check_layout(version, "test")  # unchanged layout: no error
    st.rebuild()
    with pytest.raises(ImtError, match="parameter layout changed between forward and backward"):
        st.check_layout(version, "test")
    st.check_layout(st.layout_version, "test")


def test_dropout_seed_cases():
    from imagetranslate_amd.bert_seq2seq import dropout_seed
    mod = torch.nn.Module()
    torch.manual_seed(5)
    before = torch.get_rng_state()
    assert dropout_seed(mod, False) == 0 and dropout_seed(mod, False, salt=2) == 0
    mod._imt_dropout_seed = 7
    assert dropout_seed(mod, False) == 0  # inactive wins over a pinned seed
    assert dropout_seed(mod, True) == 7 and dropout_seed(mod, True, salt=2) == 9
    assert torch.equal(torch.get_rng_state(), before)  # neither case draws
    mod._imt_dropout_seed = None
    seed = dropout_seed(mod, True, salt=2)
    after = torch.get_rng_state()
    torch.set_rng_state(before)
    assert seed == int(torch.randint(0, 2 ** 62, (1,)))  # the draw itself, no salt
    assert torch.equal(torch.get_rng_state(), after)     # exactly one randint
    assert not torch.equal(after, before)


@pytest.mark.parametrize("lang_dec", [False, True])
@pytest.mark.parametrize("tie_embed", [False, True])
def test_output_layer_and_decoder_choice(lang_dec, tie_embed):
    m = _small(lang_dec=lang_dec, tie_embed=tie_embed)
    for lang in (0, 1):
        if not lang_dec and tie_embed:
            assert not isinstance(m.output_layer, torch.nn.ModuleList) and m._output_layer(lang) is m.output_layer
        else:
            assert m._output_layer(lang) is m.output_layer[lang]
        assert m._decoder_for(lang) is (m.decoder[lang] if lang_dec else m.decoder)
    assert m._device == m.encoder.embeddings.word_embeddings.weight.device
    c = _ours("ImageCaptioning", lang_dec=lang_dec, tie_embed=tie_embed, enc_layer=2, dec_layer=2, embed_dim=64,
              intermediate_dim=128, num_attention_heads=4)
    assert c._obj_decoder_for(1) is (c.obj_decoder[1] if lang_dec else c.obj_decoder)
