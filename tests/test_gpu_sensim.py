"""SenSim on the GPU: the two-sided contrastive loss and the pair dot products against the fp64 restatement
(tests/sensim_oracle.py), whole-model parity of the three modes in fp32, the bf16 fused tail against a composition of torch
operators, encode(), save / load, init_from_lm, and the two entry points."""
import json
import os

import pytest
import torch

from oracle import reference_model as R
from tests import sensim_oracle as S
from tests.util import assert_close, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# The tolerance tests/test_gpu_multimodal.py derives for imt_contrastive: every sum is fp32 on inputs the oracle receives bit for
# bit, sums of at most a few thousand terms of unit scale -> 1e-5 of the tensor's scale.
F32_TOL = 1e-5

LOSS_CASES = [(1, 0, 0, 4), (5, 30, 17, 128), (3, 0, 40, 12), (4, 300, 263, 64), (37, 5, 2, 1024)]


def _unit_vectors(B, nsn, ntn, d, seed):
    """Normalised random vectors with a shared offset (scores away from zero), as tests/test_gpu_multimodal.py draws them."""
    g = torch.Generator().manual_seed(seed)
    off = 0.5 * torch.randn(1, d, generator=g)
    mk = lambda n: torch.nn.functional.normalize(torch.randn(n, d, generator=g) + off, dim=-1)
    return mk(nsn), mk(B), mk(ntn), mk(B)


@pytest.mark.parametrize("B,nsn,ntn,d", LOSS_CASES, ids=["B%d_sn%d_tn%d_d%d" % c for c in LOSS_CASES])
def test_two_sided_loss_kernel_against_fp64(cuda, B, nsn, ntn, d):
    from imagetranslate_amd import hip_ops as O
    sneg, src, tneg, tgt = _unit_vectors(B, nsn, ntn, d, seed=B + nsn + d)
    scat, tcat = torch.cat([sneg, src]), torch.cat([tneg, tgt])
    want = S.two_sided_loss(scat.double(), tcat.double(), B)
    g_s, g_t = S.two_sided_grads(scat.double(), tcat.double(), B)
    loss, d_s, d_t = O.sensim_loss(scat.cuda(), tcat.cuda(), B)
    e = [assert_close(loss, want.view(1), F32_TOL, "two-sided loss"),
         assert_close(d_s, g_s, F32_TOL, "d loss / d [source negatives; sources]"),
         assert_close(d_t, g_t, F32_TOL, "d loss / d [target negatives; targets]")]
    print("\n[sensim loss B=%d Ns=%d Nt=%d d=%d] loss / d_scat / d_tcat rel err %.2e / %.2e / %.2e" % (B, nsn + B, ntn + B, d, *e))
    again = O.sensim_loss(scat.cuda(), tcat.cuda(), B)
    assert all(torch.equal(a, b) for a, b in zip((loss, d_s, d_t), again)), "a second call does not give the same bits"
    if nsn != ntn:
        # the sides are not interchangeable: with the two sides' negatives swapped the loss is another one
        swapped, _, _ = O.sensim_loss(torch.cat([tneg, src]).cuda(), torch.cat([sneg, tgt]).cuda(), B)
        want_sw = S.two_sided_loss(torch.cat([tneg, src]).double(), torch.cat([sneg, tgt]).double(), B)
        assert_close(swapped, want_sw.view(1), F32_TOL, "two-sided loss, negatives swapped")
        # Both losses are within F32_TOL of fp64, so the change the kernel sees is the oracle's to 2 F32_TOL of the loss.  Random
        # negatives of one distribution move the loss little when both sides have hundreds of them; where the oracle's change
        # is well above fp32 resolution (10 F32_TOL: the two cases with few, unequal negatives) the kernel must show it.
        change64, change = float(want_sw - want), float(swapped) - float(loss)
        assert abs(change - change64) <= 2 * F32_TOL * abs(float(want))
        decisive = abs(change64) > 10 * F32_TOL * abs(float(want))
        assert decisive or (B, nsn, ntn, d) not in ((5, 30, 17, 128), (3, 0, 40, 12)), "the inputs no longer tell the sides apart"
        if decisive:
            assert abs(change) > 0.5 * abs(change64), "swapping the sides' negatives must change the loss"


@pytest.mark.parametrize("rows,d", [(1, 4), (7, 12), (300, 1024)])
def test_pair_dot_kernels_against_fp64(cuda, rows, d):
    from imagetranslate_amd import hip_ops as O
    g = torch.Generator().manual_seed(rows + d)
    a = torch.nn.functional.normalize(torch.randn(rows, d, generator=g) + 0.5 * torch.randn(1, d, generator=g), dim=-1)
    b = torch.nn.functional.normalize(torch.randn(rows, d, generator=g) + 0.5 * torch.randn(1, d, generator=g), dim=-1)
    up = torch.randn(rows, generator=g)
    out = O.pair_dot(a.cuda(), b.cuda())
    assert_close(out, S.pair_dot(a.double(), b.double()), F32_TOL, "pair dots")
    da, db = O.pair_dot_bwd(a.cuda(), b.cuda(), up.cuda())
    wa, wb = S.pair_dot_grads(a.double(), b.double(), up.double())
    assert_close(da, wa, F32_TOL, "d / d a")
    assert_close(db, wb, F32_TOL, "d / d b")
    assert torch.equal(O.pair_dot(a.cuda(), b.cuda()), out)


def test_pair_dot_of_no_rows_returns_without_a_launch(cuda):
    from imagetranslate_amd import _lib as L
    from imagetranslate_amd import hip_ops as O
    lib = L.load()
    assert lib.imt_pair_dot(None, None, None, 0, 128, None) == 0 and lib.imt_pair_dot_bwd(None, None, None, None, None, 0, 128, None) == 0
    empty = torch.empty(0, 128, device="cuda")
    assert tuple(O.pair_dot(empty, empty).shape) == (0,)
    da, db = O.pair_dot_bwd(empty, empty, torch.empty(0, device="cuda"))
    assert tuple(da.shape) == tuple(db.shape) == (0, 128)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ model level
def _pair(seed=0, d=128, heads=4, enc=2, V=1000):
    from imagetranslate_amd.sen_sim import SenSim
    torch.manual_seed(seed)
    tp = R.SyntheticTextProcessor(V)
    args = dict(enc_layer=enc, embed_dim=d, intermediate_dim=4 * d, num_attention_heads=heads)
    ref = S.SenSim(tp, **args).eval()
    with torch.no_grad():
        ref.input_attention.weight.mul_(3.0)   # pooling weights away from uniform
    ours = SenSim(tp, **args)
    ours.load_state_dict(ref.state_dict())
    return tp, ref.double(), ours.cuda().eval()


def _batch(B=5, S_=12, T=9, seed=6, nsn=30, ntn=17, V=1000):
    g = torch.Generator().manual_seed(seed)

    def ragged(n, width, lo):
        t = torch.randint(6, V, (n, width), generator=g)
        lens = torch.randint(lo, width + 1, (n,), generator=g)
        lens[0] = width
        t[torch.arange(width)[None] >= lens[:, None]] = 0
        return t
    src, tgt, sneg, tneg = ragged(B, S_, 3), ragged(B, T, 3), ragged(nsn, S_ + 2, 2), ragged(ntn, T - 2, 2)
    pos = dict(src_inputs=src, src_mask=src != 0, src_langs=torch.zeros(B, dtype=torch.long), tgt_inputs=tgt, tgt_mask=tgt != 0,
               tgt_langs=torch.ones(B, dtype=torch.long))
    neg = dict(src_neg_inputs=sneg, src_neg_mask=sneg != 0, src_neg_langs=torch.zeros(nsn, dtype=torch.long), tgt_neg_inputs=tneg,
               tgt_neg_mask=tneg != 0, tgt_neg_langs=torch.ones(ntn, dtype=torch.long))
    return pos, neg


MODES = {"dot": dict(normalize=False, neg=False), "one_sided": dict(normalize=True, neg=False),
         "two_sided": dict(normalize=True, neg=True)}


def _kwargs(mode, pos, neg):
    return dict(pos, normalize=MODES[mode]["normalize"], **(neg if MODES[mode]["neg"] else {}))


def _head(out, up):
    """A scalar to differentiate: the loss itself, or the dot products against fixed weights."""
    return out if out.dim() == 0 else (out * up.to(out.device, out.dtype)).sum()


def _zero_in_exact_arithmetic(k):
    """Biases added to every score of a softmax: their gradient is zero in exact arithmetic (shift invariance)."""
    return k.endswith("self.key.bias") or k == "input_attention.bias"


def _compare_grads(ours, ref, tol, what):
    """The rule of tests/test_gpu_multimodal.py: every gradient tensor of the oracle against ours; where the oracle has none
    ours is exactly zero; the shift-invariant biases are rounding noise on both sides, bounded absolutely."""
    ref_params = dict(ref.named_parameters())
    checked = []
    for k, p in ours.named_parameters():
        rp = ref_params[k]
        if rp.grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, "%s: %s has a gradient the oracle does not" % (what, k)
        elif _zero_in_exact_arithmetic(k):
            assert float(p.grad.abs().max()) < 1e-6 and float(rp.grad.abs().max()) < 1e-6, k
        else:
            assert float(rp.grad.abs().max()) > 0, k
            assert_close(p.grad, rp.grad, tol, "%s grad %s" % (what, k))
            checked.append(k)
    return checked


def test_three_modes_fp32_against_fp64(cuda):
    tp, ref, ours = _pair()
    pos, neg = _batch()
    up = torch.randn(5, generator=torch.Generator().manual_seed(2))
    values = {}
    for mode in MODES:
        kw = _kwargs(mode, pos, neg)
        ref.zero_grad()
        want = ref(**kw)
        _head(want, up).backward()
        ours.zero_grad()
        out = ours(**kw)
        assert out.dtype == torch.float32 and tuple(out.shape) == (() if MODES[mode]["normalize"] else (5,))
        assert_close(out.view(-1), want.view(-1), 1e-4, mode + " output")
        _head(out, up).backward()
        checked = _compare_grads(ours, ref, 1e-4, mode)
        must = ["input_attention.weight", "encoder.embeddings.word_embeddings.weight", "encoder.encoder.layer.1.output.dense.weight"]
        assert set(must) <= set(checked), set(must) - set(checked)
        assert len(checked) == len(dict(ref.named_parameters())) - 3, "every parameter but the three shift-invariant biases"
        values[mode] = out.detach()
    assert bool((values["dot"].abs() <= 1.0).all())
    assert abs(float(values["two_sided"]) - float(values["one_sided"])) > 1e-3, "the negatives change the loss"
    # negatives are used only when src_neg_langs is given (src/sen_sim.py:73)
    with torch.no_grad():
        kw = _kwargs("two_sided", pos, neg)
        assert torch.equal(ours(**dict(kw, src_neg_langs=None)), values["one_sided"])
        loss, n = ours.loss_fused(**{k: v for k, v in kw.items() if k != "normalize"})
        assert n == 5 and torch.equal(loss, values["two_sided"])
    # the same step twice from the same state: bit-identical gradient of the pooling weights
    grads = []
    for _ in range(2):
        ours.zero_grad()
        ours(**_kwargs("two_sided", pos, neg)).backward()
        grads.append(ours.input_attention.weight.grad.clone())
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0


def test_training_mode_draws_a_seed_per_encoder_pass(cuda):
    tp, _, ours = _pair(seed=4, d=64, heads=2, enc=1)
    pos, _ = _batch(seed=3)
    same = dict(pos, tgt_inputs=pos["src_inputs"], tgt_mask=pos["src_mask"], tgt_langs=pos["src_langs"])
    with torch.no_grad():
        assert float((ours(**same) - 1.0).abs().max()) < 1e-3, "eval mode: a sentence against itself"
        ours.train()
        ours.encoder._imt_dropout_seed = 77
        a, b = ours(**same), ours(**same)
        assert torch.equal(a, b), "a pinned seed repeats"
        assert float((a - 1.0).abs().max()) > 1e-3, "the two passes over the same sentences drop different elements"


class _TorchTail:
    """SenSim's tail as a composition of torch operators in the compute dtype (what the fused tail replaces)."""

    @staticmethod
    def apply(anchor, model, mode, n_neg_batches, *flat):
        states, masks = flat[0::2], flat[1::2]
        dt = states[0].dtype
        lin = model.input_attention

        def pool(x, mask):
            scores = (x @ lin.weight[0].to(dt)) + lin.bias[0].to(dt)
            scores = scores.masked_fill(~mask.bool(), -10000.0)
            v = torch.einsum("bfd,bf->bd", x, torch.softmax(scores, dim=1))
            return v / (torch.norm(v, dim=-1, p=2).unsqueeze(-1) + 1e-4)
        us = [pool(x.to(dt), m) for x, m in zip(states, masks)]
        assert mode == "two_sided" and n_neg_batches == 2
        sneg, src, tneg, tgt = us
        scat, tcat = torch.cat([sneg, src]), torch.cat([tneg, tgt])
        nominator = torch.sum(src * tgt, dim=-1) + 1e-4
        cross = torch.cat([src @ tcat.t(), tgt @ scat.t()], dim=1)
        return (torch.sum(torch.log(torch.sum(torch.exp(cross), dim=-1) + 1e-4) - nominator) / src.size(0)).float()


def test_bf16_fused_tail_against_torch_composition(cuda, monkeypatch):
    """bf16 compute: the fused tail (imt_attn_pool_* + imt_sensim_loss) against a composition of torch operators for the same steps
    in bf16 on the same encoder passes, both measured against the fp64 oracle: the worst max-norm relative error over the loss and
    every gradient tensor.  The fused path may be at most 1.5 x as far from fp64 as the composition (the margin and method of
    tests/test_gpu_multimodal.py); both distances go to profiles/sensim_parity.json."""
    import imagetranslate_amd.sen_sim as SS
    tp, ref, ours = _pair(seed=2)
    ours.set_compute_dtype(torch.bfloat16)
    pos, neg = _batch(seed=10)
    kw = _kwargs("two_sided", pos, neg)
    loss_ref = ref(**kw)
    loss_ref.backward()
    ref_params = dict(ref.named_parameters())
    report = {}
    for path in ("fused", "torch_ops"):
        with monkeypatch.context() as mp:
            if path == "torch_ops":
                mp.setattr(SS, "_PooledTailFn", _TorchTail)
            ours.zero_grad()
            loss = ours(**kw)
            loss.backward()
            per = {"loss": rel_err(loss.view(1), loss_ref.view(1))}
            for k, prm in ours.named_parameters():
                if not _zero_in_exact_arithmetic(k):
                    per[k] = rel_err(prm.grad, ref_params[k].grad)
            worst = max(per, key=per.get)
            report[path] = {"distance": per[worst], "worst": worst, "loss": per["loss"]}
    f, t = report["fused"]["distance"], report["torch_ops"]["distance"]
    report["ratio"] = f / t
    print("\n[bf16 sensim tail] fused %.3e (%s) | torch ops %.3e (%s) | ratio %.3f"
          % (f, report["fused"]["worst"], t, report["torch_ops"]["worst"], f / t))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sensim_parity.json"), "w") as fw:
        json.dump({"what": "max-norm relative distance from the fp64 oracle, worst of loss and every gradient tensor; toy model, "
                           "two-sided loss, bf16 compute, eval mode", "results": report}, fw, indent=1, sort_keys=True)
        fw.write("\n")
    assert f <= 1.5 * t, "fused %.3e from fp64, the torch composition %.3e" % (f, t)


def test_encode_returns_the_unnormalised_vectors_without_a_gradient(cuda):
    tp, ref, ours = _pair(seed=1)
    pos, _ = _batch(seed=5)
    src, mask, langs = pos["src_inputs"], pos["src_mask"], pos["src_langs"]
    with torch.no_grad():
        want = ref.encode(src, mask, langs)
    assert torch.is_grad_enabled()   # even where autograd would record: the helper is detached
    got = ours.encode(src, mask, langs.unsqueeze(-1).expand(-1, src.size(-1)))
    assert got.dtype == torch.float32 and not got.requires_grad and got.grad_fn is None
    assert_close(got, want, 1e-4, "unnormalised sentence vectors")
    norms = got.norm(dim=-1)
    assert float((norms - 1.0).abs().min()) > 1e-3, "these are not the unit vectors"
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in ours.parameters())


def test_save_load_on_the_gpu_is_bit_identical(cuda, tmp_path):
    from imagetranslate_amd.sen_sim import SenSim
    tp, _, ours = _pair(seed=3)
    pos, neg = _batch(seed=7)
    with torch.no_grad():
        before = [ours(**_kwargs(m, pos, neg)) for m in MODES]
    out = str(tmp_path / "sim")
    ours.save(out)
    loaded, tp2 = SenSim.load(out, None, text_processor=tp)
    assert loaded.encoder.embeddings.word_embeddings.weight.is_cuda and loaded.config.num_attention_heads == 4
    loaded.eval()
    with torch.no_grad():
        after = [loaded(**_kwargs(m, pos, neg)) for m in MODES]
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_init_from_lm_gives_the_lm_encoders_output(cuda):
    from imagetranslate_amd.sen_sim import SenSim
    from imagetranslate_amd.seq2seq import Seq2Seq
    tp = R.SyntheticTextProcessor(1000)
    torch.manual_seed(11)
    lm = Seq2Seq(tp, lang_dec=False, enc_layer=2, dec_layer=1, embed_dim=128, intermediate_dim=512, num_attention_heads=4).cuda().eval()
    ours = SenSim(tp, enc_layer=2, embed_dim=128, intermediate_dim=512, num_attention_heads=4).cuda().eval()
    pos, _ = _batch(seed=9)
    src, mask = pos["src_inputs"].cuda(), pos["src_mask"].cuda()
    langs = pos["src_langs"].cuda().unsqueeze(-1).expand(-1, src.size(-1))
    with torch.no_grad():
        want = lm.encoder(src, attention_mask=mask, token_type_ids=langs)
        first = ours.encoder(src, attention_mask=mask, token_type_ids=langs)
        assert not torch.equal(first, want)
        ours.init_from_lm(lm)
        got = ours.encoder(src, attention_mask=mask, token_type_ids=langs)
    assert torch.equal(got, want), "after init_from_lm the encoder is the language model's, bit for bit"
    assert ours.encoder is not lm.encoder


# ------------------------------------------------------------------------------------------------ entry points
def _files(tmp_path, n_train=200, n_dev=12):
    """MT and monolingual batch files written by the package's own writers: the tokenizer of tests/golden/marshal_kat, the
    first lines of tests/golden/sample_enfa as training pairs and negatives, marshal_kat's own corpus as the dev set."""
    from imagetranslate_amd import create_mt_batches as C
    from imagetranslate_amd.textprocessor import TextProcessor
    d = str(tmp_path)
    tok = os.path.join(GOLD, "marshal_kat", "tok")
    tp = TextProcessor(tok)
    en, fa = tp.token_id("<en>"), tp.token_id("<fa>")
    for lang in ("en", "fa"):
        lines = open(os.path.join(GOLD, "sample_enfa", lang + ".txt"), encoding="utf-8").read().split("\n")
        with open(os.path.join(d, "train." + lang), "w", encoding="utf-8") as fw:
            fw.write("\n".join(lines[:n_train]) + "\n")
        with open(os.path.join(d, "neg." + lang), "w", encoding="utf-8") as fw:
            fw.write("\n".join(lines[n_train:2 * n_train]) + "\n")
    kat = os.path.join(GOLD, "marshal_kat")
    assert C.write(tp, os.path.join(d, "train.mt"), os.path.join(d, "train.en"), en, os.path.join(d, "train.fa"), fa, min_len=3, max_len=80) > 50
    n = C.write(tp, os.path.join(d, "dev.mt"), os.path.join(kat, "src.txt"), en, os.path.join(kat, "dst.txt"), fa, min_len=3, max_len=80)
    assert n >= n_dev
    assert C.write(tp, os.path.join(d, "neg.src"), os.path.join(d, "neg.en"), en, max_len=80) > 50
    assert C.write(tp, os.path.join(d, "neg.dst"), os.path.join(d, "neg.fa"), fa, max_len=80) > 50
    return tok, tp, n


def test_train_txt_sim_and_get_sen_sim_entry_points(cuda, tmp_path, capsys, monkeypatch):
    from imagetranslate_amd import get_sen_sim as G
    from imagetranslate_amd import train_txt_sim as T
    from imagetranslate_amd.dataset import MTDataset
    from imagetranslate_amd.sen_sim import SenSim
    tok, tp, n_dev = _files(tmp_path)
    d = str(tmp_path)
    out = os.path.join(d, "sim")
    argv = ["--tok", tok, "--train_mt", os.path.join(d, "train.mt"), "--dev_mt", os.path.join(d, "dev.mt"), "--src-neg",
            os.path.join(d, "neg.src"), "--dst-neg", os.path.join(d, "neg.dst"), "--model", out, "--enc", "1", "--embed", "128",
            "--intermediate", "256", "--heads", "4", "--lr", "0.001", "--warmup", "5", "--step", "6", "--batch", "1200", "--capacity", "50",
            "--max_seq_len", "80", "--fp32", "--seed", "7", "--log-steps", "2", "--eval-steps", "3", "--save-steps", "3"]
    parse = lambda extra=(): T.get_img_options_parser().parse_args(argv + list(extra))[0]
    for flag in (["--dict", "x"], ["--cont"], ["--save-opt"], ["--lm", "x"]):
        with pytest.raises(NotImplementedError):
            T.SenSimTrainer.train(parse(flag))
    with monkeypatch.context() as mp:
        mp.setenv("WORLD_SIZE", "2")
        with pytest.raises(NotImplementedError, match="one process"):
            T.SenSimTrainer.train(parse())
    assert not os.path.exists(out) and not os.path.exists(out + ".latest")
    trainer = T.SenSimTrainer.train(parse())
    log = capsys.readouterr().out
    losses = [float(ln.split("Loss: ")[1].split()[0]) for ln in log.splitlines() if "Epoch Step:" in ln]
    assert len(losses) == 3 and all(torch.isfinite(torch.tensor(losses))), log
    dev = [float(ln.split("Dev Loss:")[1]) for ln in log.splitlines() if ln.startswith("Dev Loss:")]
    assert len(dev) >= 2 and all(torch.isfinite(torch.tensor(dev))), log
    assert trainer.optimizer.param_groups[0]["num_updates"] == 6 and trainer.best_loss == min(dev)
    for path in (out, out + ".latest"):
        assert sorted(os.listdir(path)) == ["imt_config.json", "mt_config", "mt_model.state_dict"], "weights only: no pickled optimizer"
    # scoring
    sims_path = os.path.join(d, "sims.txt")
    G.main(["--tok", tok, "--model", out + ".latest", "--dev_mt", os.path.join(d, "dev.mt"), "--output", sims_path, "--batch", "800",
            "--beam", "2", "--capacity", "50", "--fp32"])
    lines = open(sims_path, encoding="utf-8").read().split("\n")
    assert lines[-1] == "" and len(lines) - 1 == n_dev
    rows = [ln.split("\t") for ln in lines[:-1]]
    assert all(len(r) == 3 for r in rows)
    got = [float(r[2]) for r in rows]
    assert all(-1.0 <= v <= 1.0 for v in got)
    model, _ = SenSim.load(out + ".latest", tok)
    model.eval()
    data = MTDataset(batch_pickle_dir=os.path.join(d, "dev.mt"), max_batch_capacity=50, max_batch=int(800 / (2 * 2)), pad_idx=0,
                     keep_pad_idx=False)
    assert len(data) > 1, "more than one batch is scored"
    want, k = [], 0
    for b in data.batches:
        with torch.no_grad():
            sims = model(b["src_texts"], b["src_pad_mask"], b["src_langs"], b["dst_texts"], b["dst_pad_mask"], b["dst_langs"],
                         normalize=False).cpu()
        want += [float(s) for s in sims]
        for i in range(sims.numel()):
            src_ids = b["src_texts"][i][b["src_pad_mask"][i]].tolist()
            text = tp.tokenizer.decode(torch.tensor(src_ids[1:src_ids.index(tp.sep_token_id())]).numpy())
            assert rows[k][0] == text, "until </s>, first token removed"
            k += 1
    assert got == want, "the written similarities are SenSim.forward(normalize=False)"
    # one pair on its own (another batch shape: fp32 round-off only)
    b = data.batches[0]
    with torch.no_grad():
        one = model(b["src_texts"][:1], b["src_pad_mask"][:1], b["src_langs"][:1], b["dst_texts"][:1], b["dst_pad_mask"][:1],
                    b["dst_langs"][:1], normalize=False)
    assert abs(float(one[0]) - got[0]) < 1e-4
