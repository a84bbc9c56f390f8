"""Caption2Image on the GPU: the sentence-pooling and L2-distance kernels against the fp64 restatement
(tests/caption2image_oracle.py), whole-model parity in fp32, dropout consistency in training mode, the bf16 fused tail against a
composition of torch operators, the trainer and the three-hop translation."""
import json
import os

import pytest
import torch

from oracle import reference_model as R
from tests import caption2image_oracle as C
from tests.util import assert_close, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Kernel tolerances: those of tests/test_gpu_multimodal.py, for the same reasons.  Every sum is fp32 on inputs the oracle
# receives bit for bit, so probs, dw, db (and v in fp32) carry fp32 round-off only: 1e-5 of the tensor's scale.  v and dx in bf16
# are stored with one bf16 rounding: 2^-8 of the tensor's maximum.
F32_TOL = 1e-5
STORED_TOL = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -8}
SEED = 0x5EED1234ABCD

POOL_CASES = [
    ("rows5_S37_d128_ragged", 5, 37, 128, [37, 1, 0, 20, 9], 1),
    ("rows3_S200_d512_two_reads", 3, 200, 512, None, 2),
    ("rows2_S1_d1024", 2, 1, 1024, None, 1),
    # S > 256: the per-position loops take their second and third strides; d / 4 not dividing 256: idle threads in the column groups
    ("rows4_S300_d32_strided", 4, 300, 32, [300, 257, 0, 1], 1),
    ("rows3_S520_d64_strided_two_reads", 3, 520, 64, [520, 1, 0], 2),
    ("rows2_S9_d12_idle_threads", 2, 9, 12, None, 1),
]


def _keep_from_seed(rows, S, d, p, seed):
    """The dropout's keep-mask, restated by running imt_add_rows_dropout on ones over the flattened [rows * S, d] tensor."""
    from imagetranslate_amd import hip_ops as O
    ones = torch.ones(rows * S, d, device="cuda")
    return (O.add_rows_dropout(ones, None, dropout_p=p, dropout_seed=seed) != 0).view(rows, S, d).cpu()


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["p0", "p0.1"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_sent_pool_kernels_against_fp64(cuda, case, dtype, p):
    from imagetranslate_amd import hip_ops as O
    name, rows, S, d, lens, want_plan = case
    assert O.attn_pool_plan(dtype, S, d) == want_plan, "the LDS-fit switch took the other path"
    g = torch.Generator().manual_seed(rows + S)
    x = torch.randn(rows, S, d, generator=g).to(dtype)                # rounded to the compute dtype before the oracle sees them
    w = (torch.randn(d, generator=g) * (2.0 / d ** 0.5)).to(dtype)   # scores of a few units: a softmax far from uniform
    b = (torch.randn(1, generator=g) * 0.5).to(dtype)
    dv = torch.randn(rows, d, generator=g).to(dtype)
    mask = None if lens is None else torch.arange(S)[None, :] < torch.tensor(lens)[:, None]
    keep = _keep_from_seed(rows, S, d, p, SEED) if p > 0 else None
    if keep is not None:
        frac = float((~keep).float().mean())
        assert abs(frac - p) < 5 * (p * (1 - p) / keep.numel()) ** 0.5 + 1e-3, "dropped fraction %.4f for p = %.2f" % (frac, p)
    x64, w64, b64, dv64 = x.double(), w.double(), b.double()[0], dv.double()
    v_ref, p_ref = C.sent_pool(x64, w64, b64, mask, keep, p)
    dx_ref, dw_ref, db_ref = C.sent_pool_grads(x64, w64, mask, p_ref, dv64, keep, p)
    xd = C.dropped(x64, keep, p)
    dp = torch.einsum("bfd,bd->bf", xd, dv64)
    ds = p_ref * (dp - (p_ref * dp).sum(1, keepdim=True))
    ds_scale = float((ds if mask is None else ds.masked_fill(~mask, 0.0)).abs().sum())   # the scale of db's round-off

    xc, wc, bc, dvc = x.cuda(), w.cuda(), b.cuda(), dv.cuda()
    mc = None if mask is None else mask.cuda()
    v, probs = O.sent_pool_fwd(xc, wc, bc, mc, dropout_p=p, dropout_seed=SEED)
    assert v.dtype == dtype and probs.dtype == torch.float32
    e_v = assert_close(v.float(), v_ref, STORED_TOL[dtype], name + " pooled vectors")
    e_p = assert_close(probs, p_ref, F32_TOL, name + " probabilities")
    if lens is not None:
        k = lens.index(0)
        assert float(probs[k].min()) == float(probs[k].max()) and abs(float(probs[k, 0]) * S - 1.0) < 1e-6, "an all-masked row pools uniformly"
        assert_close(v[k].float(), xd[k].mean(0), STORED_TOL[dtype], name + " all-masked row = the plain average")
        one = lens.index(1)
        assert float(probs[one, 0]) == 1.0 and float(probs[one, 1:].abs().max()) == 0.0
    if S == 1:
        assert float(probs.min()) == 1.0
    # dw / db accumulate onto what the buffers hold
    g9 = torch.Generator().manual_seed(9)
    dw0, db0 = torch.randn(d, generator=g9), torch.randn(1, generator=g9)
    dw, db = dw0.cuda(), db0.cuda()
    dx = O.sent_pool_bwd(xc, wc, mc, probs, dvc, dw, db, dropout_p=p, dropout_seed=SEED)
    assert dx.dtype == dtype
    e_dx = assert_close(dx.float(), dx_ref, STORED_TOL[dtype], name + " dx")
    e_dw = assert_close(dw, dw0.double() + dw_ref, F32_TOL, name + " dw (accumulated)")
    if keep is not None:
        assert float(dx.float().cpu()[~keep].abs().max()) == 0.0, "a dropped element receives no gradient"
    # db is zero in exact arithmetic (softmax shift invariance): what comes back is the round-off of sum_s dscore_s
    db_err = abs(float(db[0]) - (float(db0[0]) + float(db_ref)))
    assert db_err <= F32_TOL * max(ds_scale, abs(float(db0[0]))), "%s db: %.3e" % (name, db_err)
    print("\n[sent pool %s %s p=%.1f] v/probs/dx/dw rel err %.2e / %.2e / %.2e / %.2e, db abs err %.2e"
          % (name, dtype, p, e_v, e_p, e_dx, e_dw, db_err))
    # a second identical call gives the same bits
    v2, probs2 = O.sent_pool_fwd(xc, wc, bc, mc, dropout_p=p, dropout_seed=SEED)
    assert torch.equal(v2, v) and torch.equal(probs2, probs)
    outs = []
    for _ in range(2):
        dw2, db2 = torch.zeros(d, device="cuda"), torch.zeros(1, device="cuda")
        outs.append((O.sent_pool_bwd(xc, wc, mc, probs, dvc, dw2, db2, dropout_p=p, dropout_seed=SEED), dw2, db2))
    assert all(torch.equal(a, b_) for a, b_ in zip(outs[0], outs[1])), "the backward does not repeat itself bit for bit"
    assert torch.equal(outs[0][0], dx)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,n", [(1, 49 * 128), (5, 49 * 128), (64, 49 * 512)])
def test_l2_dist_kernel_against_fp64(cuda, B, n, dtype):
    from imagetranslate_amd import hip_ops as O
    from imagetranslate_amd.image_model import _L2DistFn
    g = torch.Generator().manual_seed(B + n)
    pred = torch.randn(B, n, generator=g).to(dtype)
    target = (torch.randn(B, n, generator=g) * 0.5 + 0.1).to(dtype)
    want = C.l2_dist(pred.double(), target.double())
    grad = C.l2_dist_grad(pred.double(), target.double())
    loss, dpred = O.l2_dist(pred.cuda(), target.cuda())
    assert loss.dtype == torch.float32 and dpred.dtype == dtype
    e_l = assert_close(loss, want.view(1), 1e-5, "L2 loss")
    e_g = assert_close(dpred.float(), grad, STORED_TOL[dtype], "d loss / d pred")
    print("\n[l2 %dx%d %s] loss rel err %.2e, gradient rel err %.2e" % (B, n, dtype, e_l, e_g))
    again = O.l2_dist(pred.cuda(), target.cuda())
    assert torch.equal(again[0], loss) and torch.equal(again[1], dpred)
    # pred == target: distance 0, an all-zero gradient, no NaN
    zl, zg = O.l2_dist(target.cuda(), target.cuda().clone())
    assert float(zl) == 0.0 and bool(torch.isfinite(zg.float()).all()) and float(zg.float().abs().max()) == 0.0
    # an upstream factor scales the gradient (backward of 3 * loss)
    pg = pred.cuda().requires_grad_()
    (3.0 * _L2DistFn.apply(pg, target.cuda())).backward()
    assert pg.grad.dtype == dtype
    # the factor multiplies the stored gradient on the device: in bf16 that is a second rounding of unit round-off 2^-8 on top
    # of the stored one (a factor of 1, the trainer's case, is exact); in fp32 both are far below the bound
    scaled_tol = {torch.float32: 1e-5, torch.bfloat16: 2 * 2.0 ** -8}[dtype]
    assert_close(pg.grad.float(), 3.0 * grad, scaled_tol, "gradient under an upstream factor of 3")
    assert torch.equal(pg.grad, (dpred.float() * 3.0).to(dtype)), "the factor is applied in fp32 to the stored gradient"


# ------------------------------------------------------------------------------------------------ model level
def _pair(seed=0, d=128, heads=4, enc=2, ff=256, V=300):
    from imagetranslate_amd.image_model import Caption2Image
    torch.manual_seed(seed)
    tp = R.SyntheticTextProcessor(V)
    args = dict(enc_layer=enc, embed_dim=d, intermediate_dim=ff, num_attention_heads=heads)
    ref = C.Caption2Image(tp, **args).eval()
    with torch.no_grad():
        ref.input_attention.weight.mul_(10.0)   # pooling weights away from uniform
        ref.input_attention.bias.fill_(0.3)
        ref.decoder.weight.mul_(5.0)
        ref.decoder.bias.normal_(0.0, 0.1)
    ours = Caption2Image(tp, **args)
    ours.load_state_dict(ref.state_dict())
    return tp, ref.double(), ours.cuda().eval()


def _captioner(tp, d=128, heads=4, seed=5):
    from imagetranslate_amd.image_model import ImageCaptioning
    torch.manual_seed(seed)
    m = ImageCaptioning(tp, lang_dec=False, enc_layer=1, dec_layer=1, embed_dim=d, intermediate_dim=2 * d, num_attention_heads=heads,
                        image_feat_dim=64)
    return m.cuda().eval()


def _batch(B=5, S=12, seed=6, V=300):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(6, V, (B, S), generator=g)
    lens = torch.randint(3, S + 1, (B,), generator=g)
    lens[0] = S
    src[torch.arange(S)[None] >= lens[:, None]] = 0
    return dict(src=src, mask=src != 0, langs=torch.ones(B, dtype=torch.long), images=torch.randn(B, 49, 64, generator=g))


def _zero_in_exact_arithmetic(k):
    """Biases added to every score of a softmax: their gradient is zero in exact arithmetic (shift invariance)."""
    return k.endswith("self.key.bias") or k == "input_attention.bias"


def test_model_fp32_eval_against_fp64(cuda):
    tp, ref, ours = _pair()
    b = _batch()
    with torch.no_grad():
        target = _captioner(tp)(batch=[{"images": b["images"]}], encode_only=True)
    assert tuple(target.shape) == (5, 49, 128)
    want = ref(b["src"], b["mask"], b["langs"])
    with torch.no_grad():
        out = ours([b["src"]], [b["mask"]], [b["langs"]])                 # the 1-element-list convention
        enc = ours.encode(b["src"], b["mask"], b["langs"].unsqueeze(-1).expand(-1, 12))
    assert tuple(out.shape) == (5, 49 * 128) and enc[1] is None and tuple(enc[0].shape) == (5, 12, 128)
    assert_close(out, want, 1e-4, "predicted image embeddings")
    loss_ref = C.l2_dist(want, target.double().cpu().reshape(5, -1))
    loss_ref.backward()
    ours.zero_grad()
    loss, n = ours.loss_fused(b["src"], b["mask"], b["langs"], target)
    assert n == 5 and loss.dim() == 0
    assert_close(loss.view(1), loss_ref.view(1), 1e-4, "L2 loss")
    loss.backward()
    flat, n2 = ours.loss_fused(b["src"], b["mask"], b["langs"], target.reshape(5, -1))   # [B, 49 d] targets: the same number
    assert torch.equal(flat.detach(), loss.detach())
    ref_params = dict(ref.named_parameters())
    checked = []
    for k, prm in ours.named_parameters():
        rg = ref_params[k].grad
        if rg is None:
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, "%s has a gradient the oracle does not" % k
        elif _zero_in_exact_arithmetic(k):
            assert float(prm.grad.abs().max()) < 1e-6 and float(rg.abs().max()) < 1e-6, k
        else:
            assert float(rg.abs().max()) > 0, k
            assert_close(prm.grad, rg, 1e-4, "grad " + k)
            checked.append(k)
        if rg is not None and "embeddings." in k and rg.dim() == 2:
            # rows of a table the batch never reads (positions past the longest sentence, unseen words and languages, padding)
            untouched = (rg == 0).all(-1)
            assert bool(untouched.any()) and float(prm.grad[untouched.cuda()].abs().max()) == 0.0, k
    assert len(checked) == len(ref_params) - 3, "every parameter but the three shift-invariant biases is compared"
    for k in ("input_attention.weight", "decoder.weight", "decoder.bias", "encoder.embeddings.word_embeddings.weight"):
        assert k in checked


def test_training_mode_dropout_is_consistent_between_forward_and_backward(cuda):
    """The method of tests/test_gpu_model.py: with the seeds pinned the train-mode loss is a deterministic function of the
    parameters, so the analytic gradients must match central finite differences -- this fails if the pooling's backward (or a
    site of the encoder) regenerates another mask than the forward used."""
    tp, _, ours = _pair(seed=2, d=64, heads=2, enc=1, ff=128)
    ours.train()
    ours._imt_dropout_seed = 4242
    ours.encoder._imt_dropout_seed = 12345
    b = _batch(B=4, seed=9)
    target = torch.randn(4, 49, 64, generator=torch.Generator().manual_seed(1)).cuda() * 0.3

    def loss_value():
        with torch.no_grad():
            return float(ours.loss_fused(b["src"], b["mask"], b["langs"], target)[0])

    l1, l2 = loss_value(), loss_value()
    assert l1 == l2, "train-mode forward is not deterministic for a pinned seed"
    ours.eval()
    l_eval = loss_value()
    ours.train()
    assert abs(l1 - l_eval) > 1e-6, "dropout had no effect in training mode"
    # the pooling's own dropout: with the encoder's seed unchanged, another pooling seed gives another loss
    ours._imt_dropout_seed = 4243
    assert loss_value() != l1
    ours._imt_dropout_seed = 4242
    ours.zero_grad()
    loss, _ = ours.loss_fused(b["src"], b["mask"], b["langs"], target)
    loss.backward()
    named = dict(ours.named_parameters())
    assert float(named["decoder.bias"].grad.abs().max()) > 1e-4
    checks = [("input_attention.weight", (0, 5)), ("decoder.weight", (100, 7)), ("decoder.bias", (11,)),
              ("encoder.encoder.layer.0.attention.self.value.weight", (3, 5)),
              ("encoder.encoder.layer.0.intermediate.dense.weight", (7, 11)), ("encoder.embeddings.LayerNorm.weight", (6,))]
    eps = 2e-2
    for key, idx in checks:
        prm = named[key]
        g = float(prm.grad[idx])
        with torch.no_grad():
            old = float(prm[idx])
            prm[idx] = old + eps
        lp = loss_value()
        with torch.no_grad():
            prm[idx] = old - eps
        lm = loss_value()
        with torch.no_grad():
            prm[idx] = old
        fd = (lp - lm) / (2 * eps)
        assert abs(fd - g) <= 0.08 * max(abs(fd), abs(g)) + 2e-5, "%s%s: analytic %.6g vs finite-difference %.6g" % (key, idx, g, fd)


class _TorchPool:
    """The pooling as a composition of torch operators in the compute dtype (dropout-free: eval mode)."""

    @staticmethod
    def apply(anchor, states, mask, model, p, seed):
        assert p == 0.0
        dt = states.dtype
        att = model.input_attention
        scores = (states @ att.weight[0].to(dt)) + att.bias[0].to(dt)
        scores = scores.masked_fill(~mask.bool(), -10000.0)
        return torch.einsum("bfd,bf->bd", states, torch.softmax(scores, dim=1))


class _TorchDist:
    @staticmethod
    def apply(pred, target):
        return (torch.dist(pred, target, 2) / pred.size(0)).float()


def test_bf16_fused_tail_against_torch_composition(cuda, monkeypatch):
    """bf16 compute: the fused tail (imt_sent_pool_* + imt_l2_dist) against a composition of torch operators for the same steps
    in bf16 on the same encoder and linear layer, both measured against the fp64 oracle.  The fused path may be at most 1.5 x
    as far from fp64 as the composition (the margin of tests/test_gpu_multimodal.py); both distances go to
    profiles/caption2image_parity.json."""
    import imagetranslate_amd.image_model as IM
    tp, ref, ours = _pair(seed=3)
    ours.set_compute_dtype(torch.bfloat16)
    b = _batch(seed=10)
    with torch.no_grad():
        target = _captioner(tp)(batch={"images": b["images"]}, encode_only=True)
    loss_ref = ref.loss(b["src"], b["mask"], b["langs"], target.double().cpu())
    loss_ref.backward()
    ref_params = dict(ref.named_parameters())
    report = {}
    for path in ("fused", "torch_ops"):
        with monkeypatch.context() as mp:
            if path == "torch_ops":
                mp.setattr(IM, "_SentPoolFn", _TorchPool)
                mp.setattr(IM, "_L2DistFn", _TorchDist)
            ours.zero_grad()
            loss = ours.loss_fused(b["src"], b["mask"], b["langs"], target)[0]
            loss.backward()
            per = {"loss": rel_err(loss.view(1), loss_ref.view(1))}
            for k, prm in ours.named_parameters():
                if not _zero_in_exact_arithmetic(k):
                    per[k] = rel_err(prm.grad, ref_params[k].grad)
            worst = max(per, key=per.get)
            report[path] = {"distance": per[worst], "worst": worst, "loss": per["loss"]}
    f, t = report["fused"]["distance"], report["torch_ops"]["distance"]
    report["ratio"] = f / t
    print("\n[bf16 caption2image tail] fused %.3e (%s) | torch ops %.3e (%s) | ratio %.3f"
          % (f, report["fused"]["worst"], t, report["torch_ops"]["worst"], f / t))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "caption2image_parity.json"), "w") as fw:
        json.dump({"what": "max-norm relative distance from the fp64 oracle, worst of loss and every gradient tensor; toy model, "
                           "bf16 compute, eval mode", "results": report}, fw, indent=1, sort_keys=True)
        fw.write("\n")
    assert f <= 1.5 * t, "fused %.3e from fp64, the torch composition %.3e" % (f, t)


# ------------------------------------------------------------------------------------------------ trainer and translation
def _files(tmp_path, n_img=8, n_train=16, n_held=4):
    """A two-language tokenizer, features.pt (8 images, 49 x 64), 16 training captions and 4 held-out ones."""
    from imagetranslate_amd import create_mt_batches, train_tokenizer
    from imagetranslate_amd.textprocessor import TextProcessor
    from tests.test_gpu_cli import _corpus
    d = str(tmp_path)
    src, dst = _corpus(100, 4)
    with open(os.path.join(d, "all.txt"), "w") as fw:
        fw.write("\n".join(["<xa> " + s + " </s>" for s in src] + ["<xb> " + s + " </s>" for s in dst]) + "\n")
    tok = os.path.join(d, "tok")
    train_tokenizer.main(["--data", os.path.join(d, "all.txt"), "--vocab_size", "200", "--model", tok])
    tp = TextProcessor(tok)
    paths = ["img%02d.jpg" % i for i in range(n_img)]
    img_dir = os.path.join(d, "images")
    os.makedirs(img_dir)
    torch.save({"paths": paths, "feats": torch.randn(n_img, 49, 64, generator=torch.Generator().manual_seed(0))},
               os.path.join(img_dir, "features.pt"))
    out = {}
    for name, lo, hi in (("train", 0, n_train), ("held", n_train, n_train + n_held)):
        with open(os.path.join(d, name + ".tsv"), "w") as fw:
            for i in range(lo, hi):
                fw.write("%s\t%s\n" % (paths[i % n_img], src[i]))
        out[name] = os.path.join(d, name + ".cap")
        assert create_mt_batches.write_captions(tp, out[name], os.path.join(d, name + ".tsv"), tp.token_id("<xa>")) == hi - lo
    return tok, tp, img_dir, out["train"], out["held"], src


def _toy_captioner(tp, seed=1):
    from imagetranslate_amd.image_model import ImageCaptioning
    torch.manual_seed(seed)
    return ImageCaptioning(tp, lang_dec=False, enc_layer=1, dec_layer=1, embed_dim=128, intermediate_dim=256, num_attention_heads=4,
                           image_feat_dim=64)


def test_trainer_lowers_a_held_out_loss_and_its_checkpoint_loads(cuda, tmp_path, capsys, monkeypatch):
    from imagetranslate_amd import train_txt2image as T
    from imagetranslate_amd.dataset import ImageCaptionDataset
    from imagetranslate_amd.image_model import Caption2Image
    tok, tp, img_dir, caps, held, _ = _files(tmp_path)
    cap_dir = os.path.join(str(tmp_path), "captioner")
    _toy_captioner(tp).save(cap_dir)
    seen = {}
    run = T.Caption2ImageTrainer.run

    def spy(options, model, caption_model, tp_, features=None):
        seen["init"] = {k: v.detach().clone() for k, v in model.state_dict().items()}
        return run(options, model, caption_model, tp_, features)
    monkeypatch.setattr(T.Caption2ImageTrainer, "run", staticmethod(spy))
    out = os.path.join(str(tmp_path), "c2i")
    options = T.get_img_options_parser().parse_args(
        ["--tok", tok, "--pretrained", cap_dir, "--train", caps, "--image", img_dir, "--model", out, "--enc", "1", "--embed", "128",
         "--intermediate", "256", "--heads", "4", "--lr", "0.001", "--warmup", "5", "--clip", "1", "--step", "30", "--max-image", "4",
         "--img_capacity", "50", "--fp32", "--seed", "7", "--log-steps", "10"])[0]
    trainer = T.Caption2ImageTrainer.train(options)
    log = capsys.readouterr().out
    assert "Epoch Step: 30" in log and "Image per Sec" in log, log
    assert trainer.optimizer.param_groups[0]["num_updates"] == 30
    assert not trainer.caption_model.training and trainer.model.training
    assert not os.path.exists(os.path.join(out + ".latest", "optim")), "weights only: no pickled optimizer"
    batch = ImageCaptionDataset(img_dir, held, 50, tp, 4)[0]
    trained = trainer.model

    def held_out_loss(model):
        model.eval()
        with torch.no_grad():
            return float(model.loss_fused(batch["captions"], batch["caption_mask"], batch["langs"], trainer.image_encoding(batch))[0])
    before = Caption2Image(tp, enc_layer=1, embed_dim=128, intermediate_dim=256, num_attention_heads=4)
    before.load_state_dict(seen["init"])
    l0, l1 = held_out_loss(before.cuda()), held_out_loss(trained)
    print("\n[txt2image trainer] held-out loss %.5f -> %.5f after 30 steps" % (l0, l1))
    assert l1 < l0, "held-out loss %.5f before, %.5f after 30 steps" % (l0, l1)
    assert trainer.dev_loss(ImageCaptionDataset(img_dir, held, 50, tp, 4)) == pytest.approx(l1 / batch["captions"].size(0), rel=1e-6)
    loaded = Caption2Image.load(out + ".latest", tok).eval()
    assert loaded.config.num_attention_heads == 4
    with torch.no_grad():
        a = trained.eval()(batch["captions"], batch["caption_mask"], batch["langs"])
        c = loaded(batch["captions"], batch["caption_mask"], batch["langs"])
    assert torch.equal(a, c), "the checkpoint's outputs differ from the trained model's"


class _Recording:
    """A generator that keeps what every hop returned."""

    def __init__(self, gen):
        self.gen, self.max_len_a, self.max_len_b, self.outs = gen, gen.max_len_a, gen.max_len_b, []

    def __call__(self, **kw):
        self.outs.append([o.cpu() for o in self.gen(**kw)])
        return self.outs[-1]


@pytest.mark.parametrize("verbose", [False, True])
def test_three_hop_translation_through_the_toy_models(cuda, tmp_path, verbose):
    from imagetranslate_amd import translate_img as T
    from imagetranslate_amd.dataset import MTDataset
    from imagetranslate_amd.image_model import Caption2Image
    from imagetranslate_amd.seq_gen import BeamDecoder
    tok, tp, _, _, _, src = _files(tmp_path)
    torch.manual_seed(3)
    txt2img = Caption2Image(tp, enc_layer=1, embed_dim=128, intermediate_dim=256, num_attention_heads=4).cuda().eval()
    captioner = _toy_captioner(tp).cuda().eval()
    xa, xb = tp.token_id("<xa>"), tp.token_id("<xb>")
    examples = [(tp.tokenize_one_sentence("<xa> " + s + " </s>"), [xb], tp.languages["<xa>"], tp.languages["<xb>"]) for s in src[:5]]
    data = MTDataset(examples=examples, max_batch_capacity=150, max_batch=512, pad_idx=tp.pad_token_id(), max_seq_len=10000)
    batch = {k: (v.unsqueeze(0) if torch.is_tensor(v) else v) for k, v in data[0].items()}   # what a DataLoader(batch_size=1) hands over
    B = batch["src_texts"].size(1)
    gen = _Recording(BeamDecoder(captioner, beam_width=3, max_len_a=1.3, max_len_b=5))
    mt, src_text, second, third = T.translate_batch(batch, txt2img, gen, tp, verbose=verbose)
    assert len(gen.outs) == 3 and all(len(o) == B for o in gen.outs) and len(mt) == len(second) == len(third) == B
    for outs, tag in zip(gen.outs, (xb, xa, xb)):
        assert all(int(o[0]) == tag for o in outs), "every hop starts with the language tag of its side"
    # hop 1 is the direct call
    s, m = batch["src_texts"][0], batch["src_pad_mask"][0]
    with torch.no_grad():
        emb = txt2img(s, m, batch["src_langs"][0]).view(B, 49, -1)
    max_len = min(int(1.3 * s.size(1) + 5), 512)
    direct = BeamDecoder(captioner, beam_width=3, max_len_a=1.3, max_len_b=5)(
        first_tokens=batch["dst_texts"][0][:, 0], max_len=max_len, tgt_langs=batch["dst_langs"][0], image_embed=emb, pad_idx=tp.pad_token_id())
    assert [o.tolist() for o in gen.outs[0]] == [o.tolist() for o in direct]
    assert all(len(o) <= max_len for outs in gen.outs for o in outs)
    text = T.format_outputs(mt, src_text, second, third, verbose=verbose)
    if verbose:
        assert (src_text is not None) and text.count("****\n") == B and len(text.split("\n")) == 5 * B + 1
    else:
        assert src_text is None and text == "\n".join(mt) + "\n"
