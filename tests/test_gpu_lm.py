"""The masked language model on the GPU against its fp64 restatement (tests/lm_oracle.LM, with a genuinely tied word table):
forward, the fused loss and every gradient -- the table's is the sum of its two writers --, a batch with nothing masked, a bf16
step, save / load, ``init_from_lm`` of Seq2Seq and SenSim, ``train_lm`` end to end with a resumed run, ``train_image_mt --lm``."""
import os

import pytest
import torch
import torch.nn as nn

from oracle import reference_model as R
from tests import lm_oracle as M
from tests.util import assert_close, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lm_batches")
KW = dict(enc_layer=2, embed_dim=128, intermediate_dim=512, num_attention_heads=4)
V, B, S = 1000, 8, 32
BAR = 3e-4  # resumed against uninterrupted: the bound of tests/test_gpu_resume.py, for its reason (fp32 atomics in the weight gradients)


def _pair(seed=0):
    from imagetranslate_amd.lm import LM
    torch.manual_seed(seed)
    tp = R.SyntheticTextProcessor(V)
    ref = M.LM(tp, **KW).eval()
    with torch.no_grad():
        ref.masked_lm.layer.bias.normal_(std=0.5)
    ours = LM(tp, **KW)
    ours.load_state_dict(ref.state_dict())
    return tp, ref.double(), ours.cuda().eval()   # eval: dropout 0


def _batch(tp, seed=4, p=0.3):
    """Ragged rows (the first full), </s> at every row's end, masked by the oracle with probability p."""
    g = torch.Generator().manual_seed(seed)
    texts = torch.randint(7, V, (B, S), generator=g)
    lens = torch.randint(3, S + 1, (B,), generator=g)
    lens[0] = S
    pads = torch.arange(S)[None] < lens[:, None]
    texts[torch.arange(B), lens - 1] = 4
    texts[~pads] = 0
    m = M.mlm_mask_for(texts, pads, p, 1000 + seed, tp)
    assert 20 < m["count"] < int(pads.sum())
    return dict(original=texts, texts=m["texts"], pads=pads, mask=m["mask"], idx=m["idx"], targets=m["targets"],
                langs=torch.tensor([0, 1] * (B // 2)))


def _zero_in_exact_arithmetic(k):
    """A key bias adds the same number to every score of a softmax: its gradient is zero in exact arithmetic."""
    return k.endswith("self.key.bias")


def _compare_grads(ours, ref, tol, what):
    """The rule of tests/test_gpu_sensim.py: every gradient tensor of the oracle against ours; the shift-invariant key biases are
    rounding noise on both sides, bounded absolutely."""
    ref_params = dict(ref.named_parameters(remove_duplicate=False))
    checked, errs = [], {}
    for k, p in ours.named_parameters():
        rp = ref_params[k]
        assert rp.grad is not None and p.grad is not None, k
        if _zero_in_exact_arithmetic(k):
            assert float(p.grad.abs().max()) < 1e-6 and float(rp.grad.abs().max()) < 1e-6, k
        else:
            assert float(rp.grad.abs().max()) > 0, k
            errs[k] = rel_err(p.grad, rp.grad)
            checked.append(k)
    worst = max(errs, key=errs.get)
    print("\n[%s] %d gradient tensors, worst %.2e (%s)" % (what, len(errs), errs[worst], worst))
    for k in checked:
        assert_close(dict(ours.named_parameters())[k].grad, ref_params[k].grad, tol, "%s grad %s" % (what, k))
    return checked


def test_forward_loss_and_every_gradient_against_fp64(cuda):
    tp, ref, ours = _pair()
    b = _batch(tp)
    lp_ref = ref(b["mask"], b["texts"], b["pads"], b["langs"])
    loss_ref = nn.NLLLoss(ignore_index=0)(lp_ref, b["targets"])
    loss_ref.backward()
    table = ref.encoder.embeddings.word_embeddings.weight
    assert ref.masked_lm.layer.weight is table
    # the oracle's table gradient really is a sum of two parts: the projection's alone differs from it
    ref2 = M.LM(tp, **KW).eval().double()
    ref2.load_state_dict(ref.state_dict())
    hidden = ref2.encoder(b["texts"], attention_mask=b["pads"], token_type_ids=b["langs"].unsqueeze(1).expand(-1, S)).detach()
    proj = nn.NLLLoss(ignore_index=0)(torch.log_softmax(ref2.masked_lm(hidden[b["mask"]]), 1), b["targets"])
    (g_proj,) = torch.autograd.grad(proj, ref2.masked_lm.layer.weight)
    assert rel_err(g_proj, table.grad) > 1e-2, "the embedding gather's share of the tied gradient is visible"
    # forward: log-probs in the order of texts[mask]
    lp = ours(b["mask"], b["texts"], b["pads"], b["langs"])
    assert lp.dtype == torch.float32 and tuple(lp.shape) == (int(b["mask"].sum()), V)
    print("\n[lm forward] log-probs rel err %.2e" % assert_close(lp, lp_ref, 1e-4, "log-probs"))
    # the fused loss and its gradients
    ours.zero_grad()
    loss, n = ours.loss_fused(b["texts"], b["pads"], b["langs"], b["idx"], b["targets"])
    assert n == b["targets"].numel() and loss.dtype == torch.float32 and loss.dim() == 0
    print("[lm loss_fused] rel err %.2e" % assert_close(loss.view(1), loss_ref.view(1), 1e-4, "fused loss"))
    loss.backward()
    checked = _compare_grads(ours, ref, 1e-4, "loss_fused")
    assert "masked_lm.layer.weight" in checked and "masked_lm.layer.bias" in checked
    assert len(checked) == len(list(ours.parameters())) - KW["enc_layer"], "every parameter but the key biases"
    assert ours.encoder.embeddings.word_embeddings.weight is ours.masked_lm.layer.weight
    fused_table = ours.masked_lm.layer.weight.grad.clone()
    # loss_fused == NLLLoss(forward), and the materialising path's gradients
    ours.zero_grad()
    lp = ours(b["mask"], b["texts"], b["pads"], b["langs"])
    nll = nn.NLLLoss(ignore_index=0)(lp, b["targets"].cuda())
    assert_close(loss.detach().view(1), nll.detach().view(1), 1e-4, "loss_fused against NLLLoss(forward)")
    nll.backward()
    _compare_grads(ours, ref, 1e-4, "NLLLoss(forward)")
    assert_close(ours.masked_lm.layer.weight.grad, fused_table, 1e-4, "the table's gradient on the two paths")


def test_device_masking_feeds_the_loss(cuda):
    """mask_text_device -> loss_fused on the device batch equals the oracle's loss on the oracle's mask of the same seed."""
    from imagetranslate_amd.utils import mask_text_count, mask_text_device
    tp, ref, ours = _pair(seed=1)
    b = _batch(tp, seed=6)
    seed = 1000 + 6
    n = mask_text_count(0.3, b["pads"], b["original"], tp, seed)
    texts = b["original"].cuda()
    masked = mask_text_device(0.3, b["pads"].cuda(), texts, tp, seed, count=n)
    assert torch.equal(masked["texts"].cpu(), b["texts"]) and torch.equal(masked["idx"].cpu(), b["idx"])
    loss, k = ours.loss_fused(masked["texts"], b["pads"], b["langs"], masked["idx"], masked["targets"])
    want = ref.loss(b["mask"], b["texts"], b["pads"], b["langs"], b["targets"])
    assert k == n == b["targets"].numel()
    assert_close(loss.view(1), want.view(1), 1e-4, "loss on the device-masked batch")


def test_a_batch_with_nothing_masked(cuda):
    from imagetranslate_amd.train_lm import LMTrainer
    tp, _, ours = _pair(seed=2)
    b = _batch(tp)
    ours.zero_grad()
    loss, n = ours.loss_fused(b["original"], b["pads"], b["langs"], b["idx"][:0], b["targets"][:0])
    assert n == 0 and float(loss) == 0.0 and not loss.requires_grad and loss.is_cuda
    lp = ours(torch.zeros_like(b["mask"]), b["original"], b["pads"], b["langs"])
    assert tuple(lp.shape) == (0, V)
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in ours.parameters())
    # the trainer: an all-pad batch masks nothing, launches nothing and is no step
    trainer = LMTrainer(ours, mask_prob=0.15, optimizer=None, seed=3)
    empty = {"texts": torch.zeros(2, 8, dtype=torch.int64), "pad_mask": torch.zeros(2, 8, dtype=torch.bool), "langs": torch.zeros(2, dtype=torch.int64)}
    loss, n = trainer.lm_step(empty, step=0)
    assert n == 0 and float(loss) == 0.0 and trainer.micro_step == 0


def test_bf16_step(cuda):
    """bf16 compute (train_lm's default) against the fp64 oracle at the bounds tests/test_gpu_model.py asks of the bf16 model: the
    fused loss within a relative 2e-2, gradients within 8e-2 -- the tied table's against the oracle's sum --, all of them finite,
    and an optimizer step that leaves finite parameters and moves the tied table."""
    from imagetranslate_amd.utils import AdamInverseSqrtWithWarmup
    tp, ref, ours = _pair(seed=3)
    b = _batch(tp, seed=8)
    want = ref.loss(b["mask"], b["texts"], b["pads"], b["langs"], b["targets"])
    ours.set_compute_dtype(torch.bfloat16)
    opt = AdamInverseSqrtWithWarmup(ours.parameters(), lr=1e-3, betas=(0.9, 0.98), warmup_updates=2)
    ours.zero_grad()
    loss, n = ours.loss_fused(b["texts"], b["pads"], b["langs"], b["idx"], b["targets"])
    print("\n[lm bf16] loss %.5f, fp64 %.5f" % (float(loss), float(want)))
    assert float(loss) == pytest.approx(float(want), rel=2e-2)
    loss.backward()
    grads = {k: p.grad for k, p in ours.named_parameters()}
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
    ref.zero_grad()
    want.backward()
    ref_params = dict(ref.named_parameters(remove_duplicate=False))
    # the gradients at the 8e-2 of tests/test_gpu_model.py::test_bf16_mode_tracks_fp32, on that test's kinds of tensor: the tied
    # table (both writers: one overwriting the other would miss the oracle's sum by far more), the head's bias, an attention
    # projection and a feed-forward weight
    assert "encoder.embeddings.word_embeddings.weight" not in grads, "the tied table is listed once, under the head's name"
    for k in ["masked_lm.layer.weight", "masked_lm.layer.bias", "encoder.encoder.layer.0.attention.self.query.weight",
              "encoder.encoder.layer.1.output.dense.weight"]:
        print("[lm bf16] grad %s rel err %.2e" % (k, assert_close(grads[k], ref_params[k].grad, 8e-2, "bf16 grad " + k)))
    before = ours.masked_lm.layer.weight.detach().clone()
    opt.step(max_grad_norm=1.0, zero_grad=True)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in ours.parameters())
    assert float((ours.masked_lm.layer.weight.detach() - before).abs().max()) > 0
    assert ours.masked_lm.layer.weight is ours.encoder.embeddings.word_embeddings.weight


def test_save_load_round_trip(cuda, tmp_path):
    from imagetranslate_amd.lm import LM
    tp, _, ours = _pair(seed=5)
    b = _batch(tp)
    with torch.no_grad():
        before = ours(b["mask"], b["texts"], b["pads"], b["langs"])
    out = str(tmp_path / "lm")
    ours.save(out)
    loaded = LM.load(out, text_processor=tp).eval()
    assert loaded.masked_lm.layer.weight.is_cuda and loaded.config.num_attention_heads == 4
    assert loaded.masked_lm.layer.weight is loaded.encoder.embeddings.word_embeddings.weight
    with torch.no_grad():
        after = loaded(b["mask"], b["texts"], b["pads"], b["langs"])
    assert torch.equal(before, after)


def test_init_from_lm_gives_the_lm_encoders_output(cuda):
    from imagetranslate_amd.sen_sim import SenSim
    from imagetranslate_amd.seq2seq import Seq2Seq
    tp, _, lm = _pair(seed=7)
    b = _batch(tp)
    texts, pads = b["original"].cuda(), b["pads"].cuda()
    langs = b["langs"].cuda().unsqueeze(-1).expand(-1, S)
    torch.manual_seed(12)
    mt = Seq2Seq(tp, lang_dec=False, dec_layer=2, **KW).cuda().eval()
    sim = SenSim(tp, **KW).cuda().eval()
    with torch.no_grad():
        want = lm.encoder(texts, attention_mask=pads, token_type_ids=langs)
        assert not torch.equal(mt.encode(texts, pads, langs)[0], want) and not torch.equal(sim.encoder(texts, attention_mask=pads, token_type_ids=langs), want)
        mt.init_from_lm(lm)
        sim.init_from_lm(lm)
        assert torch.equal(mt.encode(texts, pads, langs)[0], want), "Seq2Seq.encode after init_from_lm is the LM's encoder, bit for bit"
        assert torch.equal(sim.encoder(texts, attention_mask=pads, token_type_ids=langs), want)
    assert torch.equal(mt.output_layer[0].layer.bias, lm.masked_lm.layer.bias) and torch.equal(mt.output_layer[1].layer.weight, lm.masked_lm.layer.weight)
    assert mt.encoder is not lm.encoder and sim.encoder is not lm.encoder
    # the model still trains: one fused step on a toy pair
    tgt = b["original"][:, :12].clone()
    tgt[:, 0] = 5
    loss, ntok = mt.train().loss_fused(b["original"], tgt, b["pads"], tgt != 0, torch.zeros(B, dtype=torch.long), torch.ones(B, dtype=torch.long))
    loss.backward()
    assert ntok > 0 and bool(torch.isfinite(loss))


# ------------------------------------------------------------------------------------------------ entry points
def _caches(tmp_path):
    """Two block directories written by create_batches from the fixture's lines: 24 documents to train on, 6 for the dev loss."""
    from imagetranslate_amd import create_batches as C
    from imagetranslate_amd.textprocessor import TextProcessor
    d = str(tmp_path)
    tok = os.path.join(GOLD, "tok")
    tp = TextProcessor(tok)
    lines = [ln for ln in open(os.path.join(GOLD, "lines.txt"), encoding="utf-8") if ln.strip()]
    out = {}
    for name, part in (("train", lines[:24]), ("dev", lines[24:])):
        with open(os.path.join(d, name + ".txt"), "w", encoding="utf-8") as fw:
            fw.write("".join(part))
        out[name] = os.path.join(d, name + ".cache")
        os.makedirs(out[name])
        rows, _ = C.write(tp, out[name], 32, os.path.join(d, name + ".txt"), 10)
        assert rows > (60 if name == "train" else 10)
    return tok, out["train"], out["dev"]


def _argv(tok, train, dev, model, steps, extra=()):
    return ["--tok", tok, "--train", train, "--dev", dev, "--model", model, "--enc", "1", "--embed", "128", "--intermediate", "256",
            "--heads", "4", "--lr", "0.002", "--warmup", "10", "--step", str(steps), "--batch", "16", "--mask", "0.3", "--fp32", "--seed", "7",
            "--log-steps", "10", "--eval-steps", "20", "--save-steps", "20", "--cache_size", "3"] + list(extra)


NOISE_ONLY = ("encoder.encoder.layer.0.attention.self.key.bias",)  # zero gradient in exact arithmetic (tests/test_gpu_resume.py)


def test_train_lm_end_to_end_and_resumed(cuda, tmp_path, capsys):
    from imagetranslate_amd import train_lm as T
    from imagetranslate_amd.lm import LM
    tok, train, dev = _caches(tmp_path)
    d = str(tmp_path)
    out = os.path.join(d, "lm")
    trainer = T.LMTrainer.train(T.get_options_parser().parse_args(_argv(tok, train, dev, out, 60))[0])
    log = capsys.readouterr().out
    losses = [float(ln.split("Loss: ")[1].split()[0]) for ln in log.splitlines() if "Epoch Step:" in ln]
    assert len(losses) == 6 and all(torch.isfinite(torch.tensor(losses))), log
    print("\n[train_lm] mean loss per 10 steps:", losses)
    assert losses[-1] < losses[0], "the loss over the last 10 of 60 steps is below the loss over the first 10"
    devs = [float(ln.split("Current dev loss")[1]) for ln in log.splitlines() if ln.startswith("Current dev loss")]
    assert len(devs) == 4 and trainer.best_loss == min(devs) and devs[-1] < devs[0], devs
    assert trainer.optimizer.param_groups[0]["num_updates"] == 60 and "Tokens per Sec" in log
    for path in (out, out + ".latest"):
        assert sorted(os.listdir(path)) == ["config", "langs", "merges.txt", "model.state_dict", "tokenizer.json", "vocab.json"], path
    lm = LM.load(out + ".latest")
    assert lm.config.num_hidden_layers == 1 and lm.text_processor.vocab_size() == 1000 and lm.text_processor.languages == {"<en>": 0, "<fa>": 1}
    # interrupted at 20 and resumed to 40, against an uninterrupted run to 40
    whole, parts = os.path.join(d, "whole"), os.path.join(d, "parts")
    T.LMTrainer.train(T.get_options_parser().parse_args(_argv(tok, train, dev, whole, 40, ["--save-state"]))[0])
    T.LMTrainer.train(T.get_options_parser().parse_args(_argv(tok, train, dev, parts, 20, ["--save-state"]))[0])
    assert os.path.isfile(os.path.join(parts + ".latest", "train_state.pt"))
    resumed = T.LMTrainer.train(T.get_options_parser().parse_args(_argv(tok, train, dev, parts, 40, ["--save-state", "--resume", parts + ".latest"]))[0])
    log = capsys.readouterr().out
    assert "resumed" in log and resumed.optimizer.param_groups[0]["num_updates"] == 40 and resumed.step == 40
    a = torch.load(os.path.join(whole + ".latest", "model.state_dict"), weights_only=True)
    b = torch.load(os.path.join(parts + ".latest", "model.state_dict"), weights_only=True)
    errs = {k: rel_err(b[k], a[k]) for k in a}
    worst = max((k for k in errs if k not in NOISE_ONLY), key=errs.get)
    print("[train_lm resume] worst %.2e (%s); key bias %.2e" % (errs[worst], worst, errs[NOISE_ONLY[0]]))
    assert set(a) == set(b) and errs[worst] <= BAR, (worst, errs[worst])
    first = torch.load(os.path.join(out + ".latest", "model.state_dict"), weights_only=True)
    assert rel_err(first["masked_lm.layer.bias"], a["masked_lm.layer.bias"]) > 10 * BAR, "20 more steps move the weights: the bar can see a difference"


def test_train_image_mt_starts_from_the_lm(cuda, tmp_path):
    from imagetranslate_amd import train_image_mt as T
    from imagetranslate_amd.lm import LM
    from imagetranslate_amd.textprocessor import TextProcessor
    tok = os.path.join(GOLD, "tok")
    tp = TextProcessor(tok)
    torch.manual_seed(3)
    lm = LM(tp, enc_layer=1, embed_dim=128, intermediate_dim=256, num_attention_heads=4)
    with torch.no_grad():
        lm.masked_lm.layer.bias.normal_()
    lm_dir = str(tmp_path / "lm")
    lm.save(lm_dir)
    argv = ["--tok", tok, "--lm", lm_dir, "--enc", "1", "--dec", "1", "--embed", "128", "--intermediate", "256", "--heads", "4", "--step", "0",
            "--fp32"]
    trainer = T.train(T.get_option_parser().parse_args(argv)[0])
    got, want = trainer.model.encoder.state_dict(), lm.encoder.state_dict()
    assert set(got) == set(want) and all(torch.equal(got[k].cpu(), want[k]) for k in want)
    for layer in trainer.model.output_layer:
        assert torch.equal(layer.layer.weight.cpu(), lm.masked_lm.layer.weight) and torch.equal(layer.layer.bias.cpu(), lm.masked_lm.layer.bias)
    with pytest.raises(ValueError, match="init_from_lm"):
        T.train(T.get_option_parser().parse_args(argv[:4] + ["--enc", "2"] + argv[6:])[0])
