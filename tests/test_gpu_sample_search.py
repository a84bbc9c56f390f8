"""Sampled decoding through ``BeamDecoder(sampling=True)`` on the toy models of tests/test_gpu_decode.py.

The sampled search is tied to paths that the oracle and the reference already pin:
  * with ``sampling_topk=1`` it IS the greedy search (``beam_width=1``): same tokens, every stream kind, both step providers,
    fp32 and bf16 with the one-launch decoder step (the d = 512 model of test_beam_search_with_the_one_launch_step);
  * ``last_scores`` is the teacher-forced log-probability of the returned tokens (``Seq2Seq.score(normalize=False)``; for the
    models whose ``score`` is refused -- captioning, proposals -- the same sum over ``forward(log_softmax=True)``), within 1e-4;
together with the step-level parity of tests/test_gpu_sample_step.py that covers the history, the cache hand-off to the children
at step 1 and the score sum."""
import os

import pytest
import torch

from oracle import reference_model as R
from tests.test_gpu_decode import _fixture_state, _pair
from tests.util import beam_inputs, beam_state_dict, caption_beam_inputs, rel_err

pytestmark = pytest.mark.gpu
EOS, PAD = 4, 0


@pytest.fixture(scope="module")
def text_model(cuda):
    return _pair(state=_fixture_state())[1]


def _decoder(model, **kw):
    from imagetranslate_amd.seq_gen import BeamDecoder
    return BeamDecoder(model, **kw)


def _padded(outs, limits, nsamples):
    """(tokens [R, T], mask [R, T]) of a search's ``unpad_output=False`` rows: a row holds its tokens through the first EOS, or up to
    its sentence's length limit (a sampled token may be id 0, so the mask comes from the structure, not from the ids)."""
    tokens = torch.stack([o.cpu() for o in outs])
    R_, T = tokens.shape
    is_eos = tokens == EOS
    first = torch.where(is_eos.any(1), is_eos.int().argmax(1) + 1, torch.full((R_,), T))
    lens = torch.minimum(first, torch.tensor([min(l, T) for l in limits for _ in range(nsamples)]))
    return tokens, torch.arange(T)[None, :] < lens[:, None]


def _summed_logprob(logprobs, tokens, mask):
    """Per-row sum of the [rows, V] log-probabilities of ``forward(log_softmax=True)`` at the targets tokens[:, 1:][mask[:, 1:]]."""
    sel = mask[:, 1:]
    targets = tokens[:, 1:][sel].to(logprobs.device)
    picked = logprobs.float().gather(1, targets[:, None]).squeeze(1).double().cpu()
    row = torch.arange(tokens.size(0))[:, None].expand_as(sel)[sel]
    return torch.zeros(tokens.size(0), dtype=torch.float64).index_add_(0, row, picked)


def _text_limits(dec, model, inp):
    from imagetranslate_amd.seq_gen import length_limits
    B = inp["src_inputs"].size(0)
    return length_limits(None, dec.max_len_a, dec.max_len_b, model.encoder.embeddings.position_embeddings.num_embeddings, B,
                         src_len=inp["src_inputs"].size(1), src_sizes=inp["src_sizes"])[1]


# ------------------------------------------------------------------------------------------- top-1 sampling == greedy
@pytest.mark.parametrize("kv_cache", [True, False], ids=["kv_cache", "recompute"])
def test_top1_sampling_is_the_greedy_search_text_fp32(cuda, text_model, kv_cache):
    inp = beam_inputs()
    for kw in (dict(), dict(unpad_output=False), dict(max_len=10)):
        want = _decoder(text_model, beam_width=1, kv_cache=kv_cache, sync_every=3)(pad_idx=0, **inp, **kw)
        dec = _decoder(text_model, kv_cache=kv_cache, sync_every=3, sampling=True, sampling_topk=1, temperature=0.7)
        got = dec(pad_idx=0, **inp, **kw)
        assert [g.tolist() for g in got] == [w.tolist() for w in want], kw
        assert dec.last_scores.shape == (6, 1) and dec.last_scores.dtype == torch.float32 and not dec.last_scores.is_cuda
    with pytest.raises(ValueError):
        dec(pad_idx=0, beam_width=3, **inp)
    assert len(dec(pad_idx=0, beam_width=1, **inp)) == 6


@pytest.mark.parametrize("kv_cache", [True, False], ids=["kv_cache", "recompute"])
def test_top1_sampling_is_the_greedy_search_caption_fp32(cuda, kv_cache):
    gold = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toy_beam.pt"), weights_only=True)
    state = {**_fixture_state(), **gold["caption_beam3"]["extra_state"]}
    ours = _pair("ImageCaptioning", state=state, image_feat_dim=64)[1]
    inp = caption_beam_inputs()
    want = _decoder(ours, beam_width=1, kv_cache=kv_cache)(pad_idx=0, max_len=14, **inp)
    got = _decoder(ours, kv_cache=kv_cache, sampling=True, sampling_topk=1)(pad_idx=0, max_len=14, **inp)
    assert [g.tolist() for g in got] == [w.tolist() for w in want]


def test_top1_sampling_is_the_greedy_search_bf16_one_launch_step(cuda):
    """bf16 at hidden size 512, where a step is ONE launch (the model of test_gpu_decode.test_beam_search_with_the_one_launch_step):
    both searches run the same decoder steps on the same tokens, so the logits -- and their argmax -- are the same bits."""
    import imagetranslate_amd.seq2seq as S
    torch.manual_seed(11)
    tp = R.SyntheticTextProcessor(1000)
    ours = S.Seq2Seq(tp, lang_dec=False, enc_layer=2, dec_layer=3, embed_dim=512, intermediate_dim=2048, num_attention_heads=8).cuda().eval()
    ours.set_compute_dtype(torch.bfloat16)
    g = torch.Generator().manual_seed(3)
    B, Sx = 12, 24
    src = torch.randint(6, 1000, (B, Sx), generator=g)
    src[:, 0], src[:, -1] = 5, 4
    args = dict(src_inputs=src.cuda(), src_sizes=torch.full((B,), Sx), first_tokens=torch.full((B,), 5),
                src_mask=torch.ones(B, Sx, dtype=torch.bool).cuda(), src_langs=torch.zeros(B, dtype=torch.long).cuda(),
                tgt_langs=torch.ones(B, dtype=torch.long).cuda(), pad_idx=0, max_len=12)
    want = _decoder(ours, beam_width=1)(**args)
    got = _decoder(ours, sampling=True, sampling_topk=1)(**args)
    assert [g_.tolist() for g_ in got] == [w.tolist() for w in want]


# ------------------------------------------------------------------------------------------- sampled search
def test_sampled_scores_are_the_models_logprobs_and_cache_modes_agree(cuda, text_model):
    inp, n = beam_inputs(), 3
    runs = {}
    for kv in (True, False):
        dec = _decoder(text_model, kv_cache=kv, sampling=True, nsamples=n, seed=99)
        runs[kv] = (dec(pad_idx=0, unpad_output=False, **inp), dec.last_scores)
    assert [o.tolist() for o in runs[True][0]] == [o.tolist() for o in runs[False][0]], "kv_cache on / off, same seed"
    outs, last = runs[True]
    assert len(outs) == 6 * n and last.shape == (6, n)
    tokens, mask = _padded(outs, _text_limits(dec, text_model, inp), n)
    assert bool((tokens[:, 0] == 5).all()) and bool((tokens[~mask] == PAD).all())
    assert len({tuple(r.tolist()) for r in tokens[:n]}) > 1, "the samples of one sentence share a parent at step 1 and must differ"
    rep = lambda t: torch.repeat_interleave(t, n, 0)
    want = text_model.score(rep(inp["src_inputs"]), tokens, rep(inp["src_mask"]), mask, rep(inp["src_langs"]), rep(inp["tgt_langs"]),
                            normalize=False)
    e = rel_err(last.view(-1), want)
    print("sampled scores against Seq2Seq.score: %.2e" % e)
    assert e <= 1e-4
    # cut at EOS: the same rows without their tail
    cut = _decoder(text_model, sampling=True, nsamples=n, seed=99)(pad_idx=0, **inp)
    assert len(cut) == 6 * n and all(EOS not in c.tolist() and c.tolist() == t[:len(c)].tolist() for c, t in zip(cut, tokens))


def test_seeds(cuda, text_model):
    inp = beam_inputs()
    dec = _decoder(text_model, sampling=True, seed=7)
    first, second = dec(pad_idx=0, **inp), dec(pad_idx=0, **inp)
    assert [o.tolist() for o in first] != [o.tolist() for o in second], "two searches of one decoder draw different noise"
    fresh = _decoder(text_model, sampling=True, seed=7)
    assert [o.tolist() for o in fresh(pad_idx=0, **inp)] == [o.tolist() for o in first]
    assert [o.tolist() for o in fresh(pad_idx=0, **inp)] == [o.tolist() for o in second]
    other = _decoder(text_model, sampling=True, seed=8)(pad_idx=0, **inp)
    assert [o.tolist() for o in other] != [o.tolist() for o in first]


def test_captioning_with_objects(cuda):
    from tests.test_gpu_object_stream import _caption_batch, _pair as obj_pair
    ref, ours = obj_pair(False, seed=3)
    ours.load_state_dict(beam_state_dict(ref.state_dict()), strict=False)
    B, n = 4, 2
    b = _caption_batch(B=B, N=19, seed=8, counts=[19, 3, 0, 11])
    dec = _decoder(ours, sampling=True, nsamples=n, sampling_topk=20, temperature=0.9, seed=3)
    outs = dec(images=b["images"], objects=b["objects"], first_tokens=torch.full((B,), 5, dtype=torch.long),
               tgt_langs=torch.ones(B, dtype=torch.long), pad_idx=0, max_len=14, unpad_output=False)
    tokens, mask = _padded(outs, [14] * B, n)
    rep = lambda t: torch.repeat_interleave(t, n, 0)
    with torch.no_grad():
        lp = ours(batch={"images": rep(b["images"]), "objects": {k: rep(v) for k, v in b["objects"].items()}}, tgt_inputs=tokens,
                  tgt_mask=mask, tgt_langs=torch.ones(B * n, dtype=torch.long), pad_idx=0, log_softmax=True)
    e = rel_err(dec.last_scores.view(-1), _summed_logprob(lp, tokens, mask))
    print("captioning with objects: %.2e" % e)
    assert e <= 1e-4


def test_proposals(cuda):
    import imagetranslate_amd.seq2seq as S
    from tests.test_gpu_proposal import _ragged_proposals
    state = _fixture_state()
    g = torch.Generator().manual_seed(4)
    state["lexical_gate"] = torch.randn(1, 128, generator=g)
    state["lexical_layer_norm.weight"] = 1.0 + 0.1 * torch.randn(128, generator=g)
    state["lexical_layer_norm.bias"] = 0.1 * torch.randn(128, generator=g)
    ours = S.Seq2Seq(R.SyntheticTextProcessor(1000), lang_dec=False, enc_layer=2, dec_layer=2, embed_dim=128, intermediate_dim=512,
                     num_attention_heads=4, use_proposals=True)
    missing = ours.load_state_dict(state, strict=False)
    assert not any("lexical" in k for k in missing.missing_keys), missing.missing_keys
    ours = ours.cuda().eval()
    inp, n = beam_inputs(), 2
    props = _ragged_proposals(6, P=9, seed=12)
    dec = _decoder(ours, sampling=True, nsamples=n, seed=21)
    outs = dec(pad_idx=0, max_len=12, proposals=props, unpad_output=False, **inp)
    limits = [min(l, 12) for l in _text_limits(dec, ours, inp)]
    tokens, mask = _padded(outs, limits, n)
    rep = lambda t: torch.repeat_interleave(t, n, 0)
    with torch.no_grad():
        lp = ours(rep(inp["src_inputs"]), tokens, rep(inp["src_mask"]), mask, rep(inp["src_langs"]), rep(inp["tgt_langs"]),
                  proposals=rep(props), log_softmax=True)
    e = rel_err(dec.last_scores.view(-1), _summed_logprob(lp, tokens, mask))
    print("proposals: %.2e" % e)
    assert e <= 1e-4
    without = _decoder(ours, sampling=True, nsamples=n, seed=21)(pad_idx=0, max_len=12, proposals=torch.zeros_like(props),
                                                                 unpad_output=False, **inp)
    assert [o.tolist() for o in without] != [o.tolist() for o in outs], "the proposals must change the draws"


# ------------------------------------------------------------------------------------------- entry points
def test_translate_cli_writes_n_lines_per_input_line(cuda, tmp_path):
    from imagetranslate_amd import train_tokenizer, translate
    from imagetranslate_amd.image_model import ImageMassSeq2Seq
    from imagetranslate_amd.textprocessor import TextProcessor
    from tests.test_gpu_cli import _corpus
    src, dst = _corpus(200, 5)
    d = str(tmp_path)
    with open(os.path.join(d, "all.txt"), "w") as fw:
        fw.write("\n".join(["<xa> " + s + " </s>" for s in src] + ["<xb> " + t + " </s>" for t in dst]) + "\n")
    with open(os.path.join(d, "in.xa"), "w") as fw:
        fw.write("\n".join(src[:7]) + "\n")
    tok, model_dir = os.path.join(d, "tok"), os.path.join(d, "model")
    train_tokenizer.main(["--data", os.path.join(d, "all.txt"), "--vocab_size", "300", "--model", tok])
    torch.manual_seed(5)
    ImageMassSeq2Seq(TextProcessor(tok), lang_dec=False, enc_layer=1, dec_layer=1, embed_dim=128, intermediate_dim=256,
                     num_attention_heads=4).save(model_dir)
    outs = []
    for run in range(2):
        out = os.path.join(d, "out%d" % run)
        translate.main(["--input", os.path.join(d, "in.xa"), "--output", out, "--src", "xa", "--target", "xb", "--tok", tok,
                        "--model", model_dir, "--fp32", "--sampling", "--nsamples", "2", "--seed", "5"])
        with open(out) as fp:
            outs.append(fp.read())
    assert outs[0].endswith("\n") and len(outs[0][:-1].split("\n")) == 14
    assert outs[0] == outs[1], "the same seed writes the same samples"
    lines = outs[0][:-1].split("\n")
    assert any(lines[2 * i] != lines[2 * i + 1] for i in range(7)), "the two samples of a line are different draws"


def test_back_translation_step_with_sampled_sources(cuda, monkeypatch):
    from imagetranslate_amd.image_model import ImageMassSeq2Seq
    from imagetranslate_amd.seq_gen import BeamDecoder
    from imagetranslate_amd.textprocessor import SyntheticTextProcessor
    from imagetranslate_amd.train_image_mt import ImageMTTrainer
    from imagetranslate_amd.utils import AdamInverseSqrtWithWarmup
    from torch.nn.utils.rnn import pad_sequence
    tp = SyntheticTextProcessor(1000)
    ours = ImageMassSeq2Seq(tp, lang_dec=False, enc_layer=2, dec_layer=2, embed_dim=128, intermediate_dim=512, num_attention_heads=4)
    assert not ours.load_state_dict(_fixture_state(), strict=False).unexpected_keys
    ours = ours.cuda().train()
    ours.set_compute_dtype(torch.float32)
    g = torch.Generator().manual_seed(12)
    B, S = 4, 12
    src = torch.randint(7, 1000, (B, S), generator=g)
    lens = torch.tensor([12, 9, 12, 7])
    src[:, 0] = 5
    for b in range(B):
        src[b, lens[b] - 1] = 4
        src[b, lens[b]:] = 0
    langs = torch.zeros(B, dtype=torch.long)
    batch = {"src_texts": src, "langs": langs, "pad_idx": torch.where(lens < S, lens, torch.full_like(lens, S - 1))}
    dirs = ImageMTTrainer.get_lang_dirs("en,fa", tp)
    tags, dst_langs = torch.full((B,), 6), torch.ones(B, dtype=torch.long)
    # the sampled sources, from an identically seeded decoder (trainer seed 1234 + rank 0), and their loss on the same weights
    ours.eval()
    twin = BeamDecoder(ours, beam_width=1, max_len_a=1.3, max_len_b=5, sampling=True, sampling_topk=10, seed=1234)
    outs = twin(src_inputs=src, src_sizes=batch["pad_idx"], first_tokens=tags, src_langs=langs, tgt_langs=dst_langs, pad_idx=0,
                src_mask=src != 0, unpad_output=False)
    trans = pad_sequence([o.cpu() for o in outs], batch_first=True, padding_value=0)
    ours.train()
    torch.manual_seed(0)  # the dropout seeds of a forward are drawn from torch's generator: the same draws for both losses
    with torch.no_grad():
        want, n_want = ours.loss_fused(src_inputs=trans, tgt_inputs=src, src_langs=dst_langs, tgt_langs=langs, pad_idx=0)
    opt = AdamInverseSqrtWithWarmup(ours.parameters(), lr=1e-4, betas=(0.9, 0.98), warmup_updates=10)
    trainer = ImageMTTrainer(ours, optimizer=opt, clip=1.0, bt_sampling=True, bt_topk=10)
    assert trainer.bt_kw["sampling"] is True and trainer.bt_kw["sampling_topk"] == 10 and trainer.bt_kw["seed"] == 1234
    torch.manual_seed(0)
    loss, n = trainer.bt_step(batch, dirs)
    assert ours.training, "the model is back in train mode"
    assert trainer.generator.sampling and trainer.generator.searches == 1
    assert n == n_want
    assert float(loss) == pytest.approx(float(want), rel=1e-4)
    # a failing generator leaves the model in train mode as well
    def boom(*a, **kw):
        raise RuntimeError("generator failed")
    monkeypatch.setattr(trainer, "generator", boom)
    with pytest.raises(RuntimeError, match="generator failed"):
        trainer.bt_step(batch, dirs)
    assert ours.training
