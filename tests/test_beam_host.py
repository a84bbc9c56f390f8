"""CPU tests of the host side of beam search and of the decoder-stream list: the length limits, which decoder / key mask /
gate every stream carries in each search mode, and the order, masks and dropout seeds of ``Seq2Seq._decode``'s passes.  The
expectations are restated from the reference (src/seq_gen.py:86-91,113-121,151-188; src/image_model.py:213-219,357-366), not
read back from the code under test.  No kernels run.

Where the GPU suite reaches each branch of a search (ids bit-exact with the oracle, fp32, kv_cache True and False in every row):
  text                      beam 1/3/4/5/12          tests/test_gpu_decode.py (and with proposals: tests/test_gpu_proposal.py)
  caption, images=          beam 3                   tests/test_gpu_decode.py::test_beam_decoder_caption (image_embed=: cached only)
  caption + objects         beam 1/3, lang_dec too   tests/test_gpu_object_stream.py::test_beam_search_fp32_matches_oracle,
                                                     images= and image_embed= together with objects=
  text + image              beam 1/3, lang_dec too   tests/test_gpu_multimodal.py::test_text_and_image_beam_search_fp32_matches_oracle
  no step at all (max_len 1; beam 1, every first token EOS)   tests/test_gpu_decode_oracle.py::
                                                     test_search_without_a_step_reports_no_abandoned_launch; max_len 2 and an EOS first
                                                     token: tests/test_gpu_decode.py::test_beam_first_step_against_reference_beam_decoder"""
import inspect

import pytest
import torch

from oracle import reference_model as R

DIMS = dict(enc_layer=1, dec_layer=1, embed_dim=64, intermediate_dim=128, num_attention_heads=4)


# ------------------------------------------------------------------------------------------------ length limits
def test_length_limits_follow_the_reference():
    from imagetranslate_amd.seq_gen import length_limits
    ref_limit = lambda s, a, b, max_pos: min(int(a * s + b), max_pos)   # :113-114
    # text search, no max_len: the limit of the source WIDTH (:116-117); per sentence the limit of its own size (:121)
    assert length_limits(None, 1.1, 5, 512, 3, src_len=12, src_sizes=torch.tensor([12, 10, 3])) == (18, [18, 16, 8], 18)
    assert ref_limit(12, 1.1, 5, 512) == 18 and ref_limit(10, 1.1, 5, 512) == 16 and ref_limit(3, 1.1, 5, 512) == 8
    # ... capped by max_position_embeddings, the width's limit and every sentence's
    assert length_limits(None, 1.1, 5, 16, 3, src_len=12, src_sizes=[12, 10, 3]) == (16, [16, 16, 8], 16)
    assert length_limits(None, 2.0, 10, 20, 2, src_len=30, src_sizes=[30, 4]) == (20, [20, 18], 20)
    # a given max_len is kept; the per-sentence limits of a text search do not depend on it (:121)
    assert length_limits(10, 1.1, 5, 512, 2, src_len=12, src_sizes=[12, 3]) == (10, [18, 8], 10)
    # images without max_len: 512 (:90-91), every sentence gets max_len when there is no source (:118-119)
    assert length_limits(None, 1.1, 5, 64, 2, images=True) == (512, [512, 512], 512)
    assert length_limits(14, 1.1, 5, 64, 3, images=True) == (14, [14, 14, 14], 14)
    assert length_limits(14, 1.1, 5, 64, 2) == (14, [14, 14], 14)                      # image_embed alone
    # a source sentence AND images: 512 columns, but the sentences keep their own limits
    assert length_limits(None, 1.1, 5, 64, 2, src_len=12, src_sizes=[12, 3], images=True) == (512, [18, 8], 512)
    # the state buffers hold at least the first token and one step
    assert length_limits(1, 1.1, 5, 64, 1, images=True) == (1, [1], 2)
    assert length_limits(0, 1.1, 5, 64, 1, images=True)[2] == 2
    assert length_limits(2, 1.1, 5, 64, 1, images=True)[2] == 2 and length_limits(3, 1.1, 5, 64, 1, images=True)[2] == 3


# ------------------------------------------------------------------------------------------------ the stream list
def _model(cls, lang_dec):
    import imagetranslate_amd.image_model as I
    import imagetranslate_amd.seq2seq as S
    kw = dict(DIMS, lang_dec=lang_dec)
    if cls == "Seq2Seq":
        return S.Seq2Seq(R.SyntheticTextProcessor(200), **kw)
    if cls == "ImageMassSeq2Seq":
        return I.ImageMassSeq2Seq(R.SyntheticTextProcessor(200), image_feat_dim=16, **kw)
    return I.ImageCaptioning(R.SyntheticTextProcessor(200), image_feat_dim=16, use_obj=True, **kw)


def _is(streams, want):
    """Every stream against (decoder, states, key mask, gate), all by identity."""
    assert len(streams) == len(want)
    for s, w in zip(streams, want):
        assert all(got is exp for got, exp in zip(s, w)), (s, w)


@pytest.mark.parametrize("lang_dec", [False, True], ids=["one_decoder", "lang_dec"])
@pytest.mark.parametrize("cls", ["Seq2Seq", "ImageMassSeq2Seq", "ImageCaptioning"])
def test_streams_of_each_search_mode(cls, lang_dec):
    from imagetranslate_amd.seq_gen import decoder_streams
    m = _model(cls, lang_dec)
    lang = 1
    decoder = m.decoder[lang] if lang_dec else m.decoder           # :156-157
    if lang_dec:
        assert decoder is not m.decoder[0]
    text, image, objects = torch.zeros(3, 7, 64), torch.zeros(3, 49, 64), torch.zeros(3, 5, 64)
    mask = torch.ones(3, 7, dtype=torch.uint8)
    # text (:151-152,163-166): the decoder over the encoder states, key mask = the source mask
    _is(decoder_streams(m, lang, text=text, text_mask=mask), [(decoder, text, mask, None)])
    if cls == "Seq2Seq":
        return
    # caption, from images= or image_embed= (:153-154,164-166): no key mask
    _is(decoder_streams(m, lang, image=image), [(decoder, image, None, None)])
    # text + image (:181-188): the SAME decoder a second time over the image regions, no key mask, multimodal_attention_gate
    _is(decoder_streams(m, lang, text=text, text_mask=mask, image=image),
        [(decoder, text, mask, None), (decoder, image, None, m.multimodal_attention_gate)])
    if cls == "ImageCaptioning":
        # caption + objects (:167-179): obj_decoder (per language with lang_dec, :168-169) over the object rows with the
        # caption's key mask -- None, there is no source -- and multistream_attention_gate
        obj_decoder = m.obj_decoder[lang] if lang_dec else m.obj_decoder
        assert obj_decoder is not decoder and (not lang_dec or obj_decoder is not m.obj_decoder[0])
        _is(decoder_streams(m, lang, image=image, objects=objects),
            [(decoder, image, None, None), (obj_decoder, objects, None, m.multistream_attention_gate)])
        assert m.multistream_attention_gate is not m.multimodal_attention_gate


# ------------------------------------------------------------------------------------------------ Seq2Seq._decode
def test_base_class_names_no_subclass_hook():
    import imagetranslate_amd.seq2seq as S
    src = inspect.getsource(S.Seq2Seq)
    assert "_mix_image_stream" not in src and "_mix_object_stream" not in src
    assert "img_states" not in inspect.signature(S.Seq2Seq._decode).parameters
    assert "obj_states" not in inspect.signature(S.Seq2Seq._decode).parameters


class _RecordingDecoder(torch.nn.Module):
    """Stands in for a decoder stack: records what a pass receives and returns a constant [B, T, d] tensor."""

    def __init__(self, log, value):
        super().__init__()
        self.log, self.value = log, value

    def forward(self, encoder_states=None, encoder_attention_mask=None, input_ids=None, **kw):
        self.log.append((self, encoder_states, encoder_attention_mask, getattr(self, "_imt_dropout_seed", None)))
        return torch.full(tuple(input_ids.shape) + (4,), self.value)


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned_seed", "drawn_seed"])
def test_decode_runs_the_streams_in_order_with_their_masks_and_seeds(monkeypatch, pinned):
    """First pass first; every pass gets its own stream's key mask (the image pass none, src/image_model.py:213-216); under a
    pinned seed a second pass over the SAME stack reads seed + 1 and a pass over another stack that stack's own seed; the pinned
    seeds are back in place afterwards.  The mix is gate-weighted left to right (:217-219, :362-366)."""
    import imagetranslate_amd.seq2seq as S
    m = _model("Seq2Seq", False)
    log, mixes = [], []
    dec, other = _RecordingDecoder(log, 1.0), _RecordingDecoder(log, 2.0)
    if pinned:
        dec._imt_dropout_seed, other._imt_dropout_seed = 40, 70
    monkeypatch.setattr(S, "gated_mix", lambda model, gate, a, b: mixes.append((model, gate, float(a.mean()), float(b.mean()))) or a + b)
    text, image, objects = torch.zeros(2, 7, 4), torch.zeros(2, 49, 4), torch.zeros(2, 5, 4)
    mask = torch.ones(2, 7, dtype=torch.bool)
    g1, g2 = torch.nn.Parameter(torch.zeros(1, 4)), torch.nn.Parameter(torch.zeros(1, 4))
    streams = [S.DecoderStream(dec, text, mask, None), S.DecoderStream(dec, image, None, g1), S.DecoderStream(other, objects, mask, g2)]
    tgt = torch.randint(6, 200, (2, 6))
    before = torch.get_rng_state()
    rows = m._decode(streams, tgt, torch.ones_like(tgt, dtype=torch.bool), torch.ones_like(tgt))
    assert torch.equal(torch.get_rng_state(), before)   # the stream loop itself draws nothing
    seeds = [40, 41, 70] if pinned else [None, None, None]
    assert len(log) == 3
    for got, want in zip(log, [(dec, text, mask, seeds[0]), (dec, image, None, seeds[1]), (other, objects, mask, seeds[2])]):
        assert all(a is b for a, b in zip(got[:3], want[:3])) and got[3] == want[3], (got, want)
    assert (getattr(dec, "_imt_dropout_seed", None), getattr(other, "_imt_dropout_seed", None)) == ((40, 70) if pinned else (None, None))
    assert mixes == [(m, g1, 1.0, 1.0), (m, g2, 2.0, 2.0)]
    assert rows.shape == (10, 4) and float(rows.min()) == float(rows.max()) == 4.0   # no padding: every row of [2, 5, 4]


def test_dropout_seed_offset_restores_the_pinned_seed():
    from imagetranslate_amd.bert_seq2seq import dropout_seed, dropout_seed_offset
    mod = torch.nn.Module()
    mod._imt_dropout_seed = 7
    with dropout_seed_offset(mod, 2):
        assert dropout_seed(mod, True) == 9
    assert mod._imt_dropout_seed == 7
    with pytest.raises(RuntimeError):
        with dropout_seed_offset(mod, 1):
            assert mod._imt_dropout_seed == 8
            raise RuntimeError("a pass fails")
    assert mod._imt_dropout_seed == 7
    with dropout_seed_offset(mod, 0):
        assert mod._imt_dropout_seed == 7
    plain = torch.nn.Module()
    with dropout_seed_offset(plain, 3):   # no pinned seed: nothing to offset, every pass draws its own
        assert getattr(plain, "_imt_dropout_seed", None) is None
    assert not hasattr(plain, "_imt_dropout_seed")


def test_unwrap_and_mass_arguments_wrapped_on_their_own():
    import imagetranslate_amd.image_model as I
    import imagetranslate_amd.mass_seq2seq as MS
    import imagetranslate_amd.seq2seq as S
    import imagetranslate_amd.seq_gen as G
    t = torch.zeros(2)
    assert S.unwrap([t]) is t and S.unwrap(t) is t and S.unwrap(None) is None
    assert MS.unwrap is S.unwrap and I.unwrap is S.unwrap and G.unwrap is S.unwrap
    for mod in (MS.MassSeq2Seq, I.ImageMassSeq2Seq, G):
        assert not hasattr(mod, "_un") and not hasattr(mod, "_unwrap_mass_args")
