"""ImageMassSeq2Seq's image branches on the GPU: the pooling and contrastive kernels against the fp64 restatement
(tests/multimodal_oracle.py), whole-model parity of the gated text + image branch and of the contrastive branch, text + image
beam search, and the trainer's image steps."""
import json
import os
import random

import pytest
import torch

from oracle import reference_model as R
from tests import multimodal_oracle as M
from tests.util import assert_close, beam_state_dict, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Kernel tolerances.  Every sum in the pooling / contrastive kernels is fp32 on inputs the oracle receives bit for bit (the bf16
# inputs are exactly representable in fp64), so u, dw, db, the loss and its gradients carry fp32 round-off only in BOTH dtypes:
# sums of at most S * d = 1e5 terms, 6e-8 each, growing like their square root -> 1e-5 of the tensor's scale.  dx is stored in
# the compute dtype: one bf16 rounding, half an ulp = 2^-9 of the element, bounded by 2^-8 of the tensor's maximum with the fp32
# error on top.
F32_TOL = 1e-5
DX_TOL = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -8}

POOL_CASES = [
    ("rows5_S37_d128_ragged", 5, 37, 128, [37, 1, 0, 20, 9], 1),
    ("rows35_S49_d128_unmasked", 35, 49, 128, None, 1),
    ("rows3_S200_d512_two_reads", 3, 200, 512, [200, 1, 0], 2),
    # S > 256: the per-position loops take their second and third strides; d / 4 not dividing 256: idle threads in the column groups
    ("rows4_S300_d32_strided", 4, 300, 32, [300, 257, 0, 1], 1),
    ("rows3_S520_d64_strided_two_reads", 3, 520, 64, [520, 1, 0], 2),
    ("rows2_S9_d12_idle_threads", 2, 9, 12, None, 1),
]


def _pool_inputs(rows, S, d, lens, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, S, d, generator=g).to(dtype)
    w = (torch.randn(d, generator=g) * (2.0 / d ** 0.5)).to(dtype)   # scores of a few units: a softmax far from uniform
    b = (torch.randn(1, generator=g) * 0.5).to(dtype)
    du = torch.randn(rows, d, generator=g)
    mask = None if lens is None else torch.arange(S)[None, :] < torch.tensor(lens)[:, None]
    return x, w, b, du, mask


_POOL_REF = {}


def _pool_reference(case, dtype):
    """fp64 oracle results of one case, computed once and shared by the tests that need them."""
    key = (case[0], dtype)
    if key not in _POOL_REF:
        name, rows, S, d, lens, _ = case
        x, w, b, du, mask = _pool_inputs(rows, S, d, lens, dtype, seed=rows + S)
        x64, w64, b64 = x.double(), w.double(), b.double()[0]
        u, p, norm = M.attn_pool(x64, w64, b64, mask)
        dx, dw, db = M.attn_pool_grads(x64, w64, mask, u, p, norm, du.double())
        # sum_s |dscore_s|: the scale of db's round-off (db itself is ~0, see below)
        r = norm.unsqueeze(-1)
        dv = du.double() / (r + 1e-4) - u * (du.double() * u).sum(-1, keepdim=True) / r
        dp = torch.einsum("bfd,bd->bf", x64, dv)
        ds = p * (dp - (p * dp).sum(1, keepdim=True))
        ds_scale = float((ds if mask is None else ds.masked_fill(~mask, 0.0)).abs().sum())
        _POOL_REF[key] = dict(inputs=(x, w, b, du, mask), u=u, p=p, dx=dx, dw=dw, db=db, ds_scale=ds_scale)
    return _POOL_REF[key]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_attn_pool_kernels_against_fp64(cuda, case, dtype):
    from imagetranslate_amd import hip_ops as O
    name, rows, S, d, lens, want_plan = case
    assert O.attn_pool_plan(dtype, S, d) == want_plan, "the LDS-fit switch took the other path"
    ref = _pool_reference(case, dtype)
    x, w, b, du, mask = (None if t is None else t.cuda() for t in ref["inputs"])
    u, probs, norm = O.attn_pool_fwd(x, w, b, mask)
    assert_close(u, ref["u"], F32_TOL, name + " unit vectors")
    assert_close(probs, ref["p"], F32_TOL, name + " probabilities")
    if lens is not None:
        k = lens.index(0)
        assert float(probs[k].min()) == float(probs[k].max()) and abs(float(probs[k, 0]) * S - 1.0) < 1e-6, "an all-masked row pools uniformly"
        one = lens.index(1)
        assert float(probs[one, 0]) == 1.0 and float(probs[one, 1:].abs().max()) == 0.0
    # dw / db accumulate onto what the buffers hold
    g = torch.Generator().manual_seed(9)
    dw0, db0 = torch.randn(d, generator=g), torch.randn(1, generator=g)
    dw, db = dw0.cuda(), db0.cuda()
    dx = O.attn_pool_bwd(x, w, mask, u, probs, norm, du, dw, db)
    assert dx.dtype == dtype
    e = [assert_close(dx.float(), ref["dx"], DX_TOL[dtype], name + " dx"),
         assert_close(dw, dw0.double() + ref["dw"], F32_TOL, name + " dw (accumulated)")]
    # db is zero in exact arithmetic whenever a row has an unmasked position (softmax shift invariance) and exactly zero for an
    # all-masked row: what the kernel returns is the round-off of sum_s dscore_s, bounded relative to sum_s |dscore_s|
    db_err = abs(float(db[0]) - (float(db0[0]) + float(ref["db"])))
    assert db_err <= F32_TOL * max(ref["ds_scale"], abs(float(db0[0]))), "%s db: %.3e" % (name, db_err)
    print("\n[pool %s %s] u/dx/dw rel err %.2e / %.2e / %.2e, db abs err %.2e" % (name, dtype, rel_err(u, ref["u"]), e[0], e[1], db_err))
    # a second identical call gives the same bits (per-sentence partials, fixed-order fold)
    outs = []
    for _ in range(2):
        dw2, db2 = torch.zeros(d, device="cuda"), torch.zeros(1, device="cuda")
        dx2 = O.attn_pool_bwd(x, w, mask, u, probs, norm, du, dw2, db2)
        outs.append((dx2, dw2, db2))
    assert all(torch.equal(a, b_) for a, b_ in zip(outs[0], outs[1])), "the backward does not repeat itself bit for bit"
    assert torch.equal(outs[0][0], dx)
    # the upstream-gradient scalar multiplies du
    dw3, db3 = torch.zeros(d, device="cuda"), torch.zeros(1, device="cuda")
    dx3 = O.attn_pool_bwd(x, w, mask, u, probs, norm, du, dw3, db3, du_scale=torch.full((1,), 0.5, device="cuda"))
    assert_close(dw3, 0.5 * ref["dw"], F32_TOL, name + " dw with du_scale")
    assert_close(dx3.float(), 0.5 * ref["dx"], DX_TOL[dtype], name + " dx with du_scale")


def test_contrastive_kernel_against_fp64(cuda):
    from imagetranslate_amd import hip_ops as O
    g = torch.Generator().manual_seed(5)
    B, Nn, d = 5, 30, 128
    img = torch.nn.functional.normalize(torch.randn(B, d, generator=g), dim=-1)
    txt = torch.nn.functional.normalize(torch.randn(B + Nn, d, generator=g) + 0.5 * torch.randn(1, d, generator=g), dim=-1)
    loss, d_img, d_txt = O.contrastive(img.cuda(), txt.cuda())
    want = M.contrastive(img.double(), txt.double())
    g_img, g_txt = M.contrastive_grads(img.double(), txt.double())
    assert_close(loss, want.view(1), F32_TOL, "contrastive loss")
    assert_close(d_img, g_img, F32_TOL, "d loss / d image vectors")
    assert_close(d_txt, g_txt, F32_TOL, "d loss / d text vectors")
    again = O.contrastive(img.cuda(), txt.cuda())
    assert all(torch.equal(a, b) for a, b in zip((loss, d_img, d_txt), again))


# ------------------------------------------------------------------------------------------------ model level
def _pair(seed=0, d=128, heads=4, enc=2, dec=2, V=1000, double=True, sharpen=False, lang_dec=False, **kw):
    from imagetranslate_amd.image_model import ImageMassSeq2Seq
    torch.manual_seed(seed)
    tp = R.SyntheticTextProcessor(V)
    args = dict(lang_dec=lang_dec, enc_layer=enc, dec_layer=dec, embed_dim=d, intermediate_dim=4 * d, num_attention_heads=heads,
                image_feat_dim=64, **kw)
    ref = M.MultimodalSeq2Seq(tp, **args).eval()
    with torch.no_grad():
        ref.multimodal_attention_gate.normal_(0.0, 1.0)   # away from its 0.1 fill: both streams matter, per column
        ref.encoder_attention_w.weight.mul_(3.0)          # pooling weights away from uniform
        ref.image_attention_w.weight.mul_(3.0)
        if lang_dec:  # the per-language decoders start as copies of one another: language 0's must differ, so that running it shows
            for lyr in ref.decoder[0].decoder.layer:
                lyr.output.dense.weight.neg_()
    if sharpen:
        ref.load_state_dict(beam_state_dict(ref.state_dict()))
    ours = ImageMassSeq2Seq(tp, **args)
    res = ours.load_state_dict(ref.state_dict(), strict=False)
    assert not res.unexpected_keys and all("layer_norm" in k for k in res.missing_keys), res
    return (ref.double() if double else ref), ours.cuda().eval()


def _batch(B=5, S=12, T=9, seed=6, Nn=30):
    g = torch.Generator().manual_seed(seed)

    def ragged(n, width, lo):
        t = torch.randint(6, 1000, (n, width), generator=g)
        lens = torch.randint(lo, width + 1, (n,), generator=g)
        lens[0] = width
        t[torch.arange(width)[None] >= lens[:, None]] = 0
        return t
    src, tgt, neg = ragged(B, S, 3), ragged(B, T, 3), ragged(Nn, S + 1, 2)
    return dict(src=src, tgt=tgt, neg=neg, pos=torch.randint(0, S, (B, T), generator=g), images=torch.randn(B, 49, 64, generator=g),
                langs=torch.ones(B, dtype=torch.long))


def _zero_in_exact_arithmetic(k):
    """Biases added to every score of a softmax: their gradient is zero in exact arithmetic (shift invariance)."""
    return k.endswith("self.key.bias") or k in ("encoder_attention_w.bias", "image_attention_w.bias")


def _compare_grads(ours, ref, tol, what):
    """Every gradient tensor of the oracle against ours; where the oracle has none ours is exactly zero.  The self-attention
    key biases and the pooling biases are zero in exact arithmetic (softmax shift invariance): rounding noise on both sides,
    bounded absolutely, the rule of tests/test_gpu_object_stream.py."""
    ref_params = dict(ref.named_parameters())
    checked, zero = [], []
    for k, p in ours.named_parameters():
        rp = ref_params.get(k)
        if rp is None:
            continue
        if rp.grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, "%s: %s has a gradient the oracle does not" % (what, k)
            zero.append(k)
        elif _zero_in_exact_arithmetic(k):
            assert float(p.grad.abs().max()) < 1e-6 and float(rp.grad.abs().max()) < 1e-6, k
            checked.append(k)
        else:
            assert float(rp.grad.abs().max()) > 0, k
            assert_close(p.grad, rp.grad, tol, "%s grad %s" % (what, k))
            checked.append(k)
    return checked, zero


def _gated_kw(b, with_pos, lists=False):
    wrap = (lambda t: [t]) if lists else (lambda t: t)
    return dict(src_inputs=wrap(b["src"]), src_pads=wrap(b["src"] != 0), tgt_inputs=wrap(b["tgt"]), src_langs=wrap(b["langs"]),
                tgt_langs=wrap(b["langs"]), pad_idx=0, tgt_positions=wrap(b["pos"]) if with_pos else None)


@pytest.mark.parametrize("with_pos", [False, True], ids=["no_positions", "tgt_positions"])
def test_gated_branch_fp32_against_fp64(cuda, with_pos):
    ref, ours = _pair()
    b = _batch()
    batch = {"images": b["images"]}
    kw = _gated_kw(b, with_pos)
    lp_ref = ref(batch=batch, log_softmax=True, **kw)
    lp = ours(batch=[batch], log_softmax=True, **_gated_kw(b, with_pos, lists=True))   # the 1-element-list convention
    assert_close(lp, lp_ref, 1e-4, "gated branch log-probs")
    assert torch.equal(lp.argmax(-1).cpu(), lp_ref.argmax(-1))
    targets = b["tgt"][:, 1:][b["tgt"][:, 1:] != 0]
    loss_ref = R.SmoothedNLLLoss(ignore_index=0)(lp_ref, targets).mean()
    loss_ref.backward()
    ours.zero_grad()
    loss, n = ours.loss_fused(batch=batch, **kw)
    assert n == targets.numel()
    assert_close(loss.view(1), loss_ref.view(1), 1e-4, "gated branch loss")
    loss.backward()
    checked, zero = _compare_grads(ours, ref, 1e-4, "gated branch")
    must = ["multimodal_attention_gate", "image_model.fc.weight", "image_model.location_embedding.weight",
            "decoder.decoder.layer.0.crossattention.self.key.weight", "decoder.decoder.layer.1.output.dense.weight",
            "decoder.embeddings.LayerNorm.weight", "encoder.embeddings.word_embeddings.weight", "output_layer.1.layer.weight"]
    assert set(must) <= set(checked), set(must) - set(checked)
    assert set(zero) >= {"encoder_attention_w.weight", "image_attention_w.weight"}
    # tgt_langs left out (the reference trainer's masked step): the captions' own language
    kw2 = dict(kw, tgt_langs=None)
    with torch.no_grad():
        assert torch.equal(ours(batch=batch, log_softmax=True, **kw2), lp.detach())


def test_contrastive_branch_fp32_against_fp64(cuda):
    ref, ours = _pair(seed=1)
    b = _batch(seed=8)
    batch = {"images": b["images"]}
    kw = dict(src_inputs=b["src"], src_pads=b["src"] != 0, src_langs=b["langs"], tgt_langs=b["langs"], pad_idx=0,
              neg_samples=b["neg"], neg_mask=b["neg"] != 0)
    loss_ref = ref(batch=batch, **kw)
    loss_ref.backward()
    ours.zero_grad()
    loss = ours(batch=batch, **{k: ([v] if k in ("neg_samples", "neg_mask") else v) for k, v in kw.items()})
    assert loss.dim() == 0
    assert_close(loss.view(1), loss_ref.view(1), 1e-4, "contrastive loss")
    loss.backward()
    checked, zero = _compare_grads(ours, ref, 1e-4, "contrastive branch")
    must = ["encoder_attention_w.weight", "image_attention_w.weight", "image_model.fc.weight", "image_model.location_embedding.weight",
            "encoder.embeddings.word_embeddings.weight", "encoder.encoder.layer.1.output.dense.weight"]
    assert set(must) <= set(checked), set(must) - set(checked)
    assert any(k.startswith("output_layer") for k in zero) and "multimodal_attention_gate" in zero
    assert any(k.startswith("decoder.decoder.layer.0.crossattention") for k in zero) and len(zero) > 20
    # the attention biases: zero in exact arithmetic (shift invariance of the softmax), rounding noise here
    for name in ("encoder_attention_w.bias", "image_attention_w.bias"):
        assert float(dict(ours.named_parameters())[name].grad.abs().max()) < 1e-6
    # the same step twice from the same state: bit-identical gradients of the pooling weights
    g1 = ours.encoder_attention_w.weight.grad.clone()
    ours.zero_grad()
    l2, n = ours.loss_fused(batch=batch, **kw)
    assert n == 0 and torch.equal(l2, loss.detach())
    l2.backward()
    assert torch.equal(ours.encoder_attention_w.weight.grad, g1)


class _TorchTail:
    """The contrastive tail as a composition of torch operators in the compute dtype (what the fused tail replaces)."""

    @staticmethod
    def apply(anchor, enc, src_mask, neg, neg_mask, img, model):
        dt = enc.dtype

        def pool(x, lin, mask):
            scores = (x @ lin.weight[0].to(dt)) + lin.bias[0].to(dt)
            if mask is not None:
                scores = scores.masked_fill(~mask.bool(), -10000.0)
            v = torch.einsum("bfd,bf->bd", x, torch.softmax(scores, dim=1))
            return v / (torch.norm(v, dim=-1, p=2).unsqueeze(-1) + 1e-4)
        txt = torch.cat([pool(enc, model.encoder_attention_w, src_mask), pool(neg.to(dt), model.encoder_attention_w, neg_mask)])
        im = pool(img.to(dt), model.image_attention_w, None)
        cross = im @ txt.t()
        B = im.size(0)
        return (torch.sum(torch.log(torch.sum(torch.exp(cross), dim=-1) + 1e-4) - (torch.diagonal(cross[:, :B], 0) + 1e-4)) / B).float()


def _torch_gated_mix(model, gate_param, a, b):
    s = torch.sigmoid(gate_param.to(a.dtype) + 1e-7)
    return s * a + (1 - s) * b.to(a.dtype)


def _distance(ours, ref, head):
    """max over the head quantity (loss / log-probs) and every gradient tensor of its max-norm relative error."""
    per = {"head": head}
    ref_params = dict(ref.named_parameters())
    for k, p in ours.named_parameters():
        rp = ref_params.get(k)
        if rp is None or rp.grad is None or _zero_in_exact_arithmetic(k):
            continue
        per[k] = rel_err(p.grad, rp.grad)
    worst = max(per, key=per.get)
    return per[worst], worst, per


def test_bf16_fused_paths_against_torch_composition(cuda, monkeypatch):
    """bf16 compute: the fused tail (imt_attn_pool_* + imt_contrastive) and the fused gated mix against a composition of torch
    operators for the same steps in bf16 on the same stacks, both measured against the fp64 oracle.  The fused path may be at
    most 1.5 x as far from fp64 as the composition (the margin tests/test_gpu_decode_oracle.py gives the one-launch step);
    both distances go to profiles/multimodal_parity.json."""
    import imagetranslate_amd.image_model as IM
    import imagetranslate_amd.seq2seq as S2S
    report = {}
    for branch in ("contrastive", "gated"):
        ref, ours = _pair(seed=2)
        ours.set_compute_dtype(torch.bfloat16)
        b = _batch(seed=10)
        batch = {"images": b["images"]}
        if branch == "contrastive":
            kw = dict(src_inputs=b["src"], src_pads=b["src"] != 0, src_langs=b["langs"], tgt_langs=b["langs"], pad_idx=0,
                      neg_samples=b["neg"], neg_mask=b["neg"] != 0)
            loss_ref = ref(batch=batch, **kw)
        else:
            kw = _gated_kw(b, True)
            lp_ref = ref(batch=batch, log_softmax=True, **kw)
            loss_ref = R.SmoothedNLLLoss(ignore_index=0)(lp_ref, b["tgt"][:, 1:][b["tgt"][:, 1:] != 0]).mean()
        loss_ref.backward()
        dist = {}
        for path in ("fused", "torch_ops"):
            with monkeypatch.context() as mp:
                if path == "torch_ops":
                    mp.setattr(IM, "_ContrastiveTailFn", _TorchTail)
                    mp.setattr(S2S, "gated_mix", _torch_gated_mix)   # where the decoder's stream loop looks it up
                ours.zero_grad()
                loss = ours.loss_fused(batch=batch, **kw)[0]
                loss.backward()
                d, worst, per = _distance(ours, ref, rel_err(loss.view(1), loss_ref.view(1)))
                dist[path] = d
                report[branch + "/" + path] = {"distance": d, "worst": worst, "loss": per["head"]}
        print("\n[bf16 %s] fused %.3e (%s) | torch ops %.3e (%s)" % (branch, dist["fused"], report[branch + "/fused"]["worst"],
                                                                     dist["torch_ops"], report[branch + "/torch_ops"]["worst"]))
        report[branch + "/ratio"] = dist["fused"] / dist["torch_ops"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "multimodal_parity.json"), "w") as fw:
        json.dump({"what": "max-norm relative distance from the fp64 oracle, worst of loss and every gradient tensor; toy model, "
                           "bf16 compute", "results": report}, fw, indent=1, sort_keys=True)
        fw.write("\n")
    for branch in ("contrastive", "gated"):
        f, t = report[branch + "/fused"]["distance"], report[branch + "/torch_ops"]["distance"]
        assert f <= 1.5 * t, "%s: fused %.3e from fp64, the torch composition %.3e" % (branch, f, t)


# ------------------------------------------------------------------------------------------------ beam search
def _search_inputs(B=4, S=10, seed=3):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(6, 1000, (B, S), generator=g)
    lens = torch.tensor([10, 7, 4, 9])[:B]
    mask = torch.arange(S)[None, :] < lens[:, None]
    src[~mask] = 0
    src[:, 0] = 5
    for r in range(B):
        src[r, lens[r] - 1] = 4
    return dict(src_inputs=src, src_sizes=lens, first_tokens=torch.full((B,), 5, dtype=torch.long), src_mask=mask,
                src_langs=torch.zeros(B, dtype=torch.long), tgt_langs=torch.ones(B, dtype=torch.long), pad_idx=0), \
        torch.randn(B, 49, 64, generator=g)


@pytest.mark.parametrize("beam,lang_dec", [(1, False), (3, False), (1, True), (3, True)], ids=["1", "3", "1-lang_dec", "3-lang_dec"])
def test_text_and_image_beam_search_fp32_matches_oracle(cuda, beam, lang_dec):
    from imagetranslate_amd.seq_gen import BeamDecoder
    from oracle import seq_gen as OG
    ref, ours = _pair(seed=3, double=False, sharpen=True, lang_dec=lang_dec)
    inp, images = _search_inputs()
    want = M.beam_search(ref, images, beam, max_len=16, **inp)
    text_only = OG.BeamDecoder(ref, beam_width=beam)(max_len=16, **inp)
    assert [w.tolist() for w in want] != [w.tolist() for w in text_only], "the image must change the search"
    for kv in (True, False):
        got = BeamDecoder(ours, beam_width=beam, kv_cache=kv)(images=images, max_len=16, **inp)
        assert [g.tolist() for g in got] == [w.tolist() for w in want], "kv_cache=%s" % kv
    # precomputed image embeddings take the same route
    with torch.no_grad():
        emb = ours.image_model(images.cuda(), torch.float32)[0]
    got = BeamDecoder(ours, beam_width=beam)(images=images, image_embed=emb, max_len=16, **inp)
    assert [g.tolist() for g in got] == [w.tolist() for w in want]


@pytest.mark.parametrize("beam", [1, 3])
def test_text_and_image_beam_search_one_launch_against_chain(cuda, monkeypatch, beam):
    """bf16, d = 512, h = 8, 2 layers: both incremental decoders (the same stack over the text states and over the image regions)
    take the one-launch step.  Against the launch-per-operator chain under the rule of
    tests/test_gpu_object_stream.py::test_beam_search_with_objects_one_launch_against_chain: the two bf16 paths round
    pre-LayerNorm sums at different places, so a near-tie may flip late in a sentence; the first tokens agree on all but at most
    two of the sentences."""
    from imagetranslate_amd.image_model import ImageMassSeq2Seq
    from imagetranslate_amd.seq_gen import BeamDecoder
    torch.manual_seed(11)
    m = ImageMassSeq2Seq(R.SyntheticTextProcessor(1000), lang_dec=False, enc_layer=2, dec_layer=2, embed_dim=512, intermediate_dim=2048,
                         num_attention_heads=8, image_feat_dim=64)
    with torch.no_grad():
        m.multimodal_attention_gate.normal_()
    m.set_compute_dtype(torch.bfloat16)
    m = m.cuda().eval()
    B, S = 12, 10
    g = torch.Generator().manual_seed(21)
    src = torch.randint(6, 1000, (B, S), generator=g)
    lens = torch.randint(4, S + 1, (B,), generator=g)
    mask = torch.arange(S)[None, :] < lens[:, None]
    src[~mask] = 0
    args = dict(src_inputs=src, src_sizes=lens, src_mask=mask, src_langs=torch.zeros(B, dtype=torch.long),
                first_tokens=torch.full((B,), 5, dtype=torch.long), tgt_langs=torch.ones(B, dtype=torch.long), pad_idx=0, max_len=12)
    images = torch.randn(B, 49, 64, generator=g)
    outs = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("IMT_DECODE_FUSED", fused)
        outs[fused] = BeamDecoder(m, beam_width=beam, kv_cache=True)(images=images, **args)
    head = sum(int(x[:4].tolist() == y[:4].tolist()) for x, y in zip(outs["1"], outs["0"]))
    assert head >= B - 2, "the first tokens of %d of %d sentences differ between the one-launch step and the chain" % (B - head, B)
    for o in outs["1"]:
        assert int(o[0]) == 5 and 1 <= len(o) <= 12 and bool(((o >= 0) & (o < 1000)).all())
    monkeypatch.setenv("IMT_DECODE_FUSED", "1")
    plain = BeamDecoder(m, beam_width=beam, kv_cache=True)(**args)
    assert [o.tolist() for o in plain] != [o.tolist() for o in outs["1"]], "the image must change the search"


# ------------------------------------------------------------------------------------------------ trainer
def _image_training_files(tmp_path):
    from imagetranslate_amd import create_mt_batches, train_tokenizer
    from imagetranslate_amd.textprocessor import TextProcessor
    from tests.test_gpu_cli import _corpus
    d = str(tmp_path)
    src, _ = _corpus(100, 4)
    with open(os.path.join(d, "all.txt"), "w") as fw:
        fw.write("\n".join(["<xa> " + s + " </s>" for s in src]) + "\n")
    tok = os.path.join(d, "tok")
    train_tokenizer.main(["--data", os.path.join(d, "all.txt"), "--vocab_size", "200", "--model", tok])
    tp = TextProcessor(tok)
    n_img = 6
    paths = ["img%02d.jpg" % i for i in range(n_img)]
    img_dir = os.path.join(d, "images")
    os.makedirs(img_dir)
    torch.save({"paths": paths, "feats": torch.randn(n_img, 49, 64, generator=torch.Generator().manual_seed(0))},
               os.path.join(img_dir, "features.pt"))
    with open(os.path.join(d, "captions.tsv"), "w") as fw:
        for i in range(3 * n_img):
            fw.write("%s\t%s\n" % (paths[i % n_img], src[i]))
    caps = os.path.join(d, "train.cap")
    assert create_mt_batches.write_captions(tp, caps, os.path.join(d, "captions.tsv"), tp.token_id("<xa>")) == 3 * n_img
    return tok, tp, img_dir, caps


def _small_model(tp, seed=1):
    from imagetranslate_amd.image_model import ImageMassSeq2Seq
    torch.manual_seed(seed)
    return ImageMassSeq2Seq(tp, lang_dec=False, enc_layer=1, dec_layer=1, embed_dim=128, intermediate_dim=256, num_attention_heads=4,
                            image_feat_dim=64)


@pytest.mark.parametrize("mode", ["masked", "contrastive"])
def test_trainer_consumes_image_batches(cuda, tmp_path, capsys, mode):
    from imagetranslate_amd import train_image_mt as T
    from imagetranslate_amd.dataset import ImageCaptionDataset
    from imagetranslate_amd.utils import build_optimizer, mass_mask_device
    tok, tp, img_dir, caps = _image_training_files(tmp_path)
    init_dir = os.path.join(str(tmp_path), "init")
    _small_model(tp).save(init_dir)
    init = _small_model(tp).state_dict()
    # --- three steps through the command line's own path
    options = T.get_option_parser().parse_args(["--image", img_dir, "--train", caps, "--tok", tok, "--model", os.path.join(str(tmp_path), "out"),
                                                "--pretrained", init_dir, "--max-image", "4", "--img_capacity", "50", "--mmode", mode,
                                                "--step", "3", "--lr", "0.003", "--warmup", "2", "--log-steps", "1", "--fp32",
                                                "--seed", "7"])[0]
    trainer = T.train(options)
    log = capsys.readouterr().out
    assert "image batches" in log and trainer.image_steps == 3, log
    assert trainer.last_image_step[0] == mode and bool(torch.isfinite(trainer.last_image_step[1]))
    after = trainer.model.state_dict()
    moved = [k for k, v in after.items() if not torch.equal(v.cpu(), init[k])]
    for k in ("encoder.embeddings.word_embeddings.weight", "image_model.fc.weight"):
        assert k in moved, "%s did not move" % k
    out_layers = [k for k in after if k.startswith("output_layer")]
    if mode == "contrastive":
        assert "encoder_attention_w.weight" in moved and "image_attention_w.weight" in moved
        assert out_layers and not any(k in moved for k in out_layers), "the contrastive step must leave the output layers alone"
        assert "multimodal_attention_gate" not in moved
    else:
        assert "multimodal_attention_gate" in moved and any(k in moved for k in out_layers)
    # --- one step against a direct call on the same batch and seed
    data = ImageCaptionDataset(img_dir, caps, 50, tp, 4, use_neg_samples=True, neg_seed=7)
    assert len(data) >= 3
    batch = data[1]
    models = [_small_model(tp).cuda().train() for _ in range(2)]
    for m in models:
        m.set_compute_dtype(torch.float32)
    tr = T.ImageMTTrainer(models[0], mask_prob=0.5, clip=1.0, optimizer=build_optimizer(models[0], 0.003, 2), seed=7, mm_mode=mode)
    torch.manual_seed(5)
    loss_t, n_t = tr.image_step(batch)
    rng = random.Random((7 + 2) * 104729)   # the trainer's generator for image steps
    torch.manual_seed(5)
    if mode == "masked":
        mask_prob = min(rng.uniform(0.5, 1.0), 1.0 - 1e-6)
        masked = mass_mask_device(mask_prob, batch["pad_idx"], batch["captions"].cuda(), tp, seed=rng.getrandbits(62))
        loss_d, n_d = models[1].loss_fused(src_inputs=masked["src_text"], tgt_inputs=masked["to_recover"], tgt_positions=masked["positions"],
                                           src_pads=batch["caption_mask"], pad_idx=tp.pad_token_id(), src_langs=batch["langs"],
                                           tgt_langs=batch["langs"], batch=batch)
        assert n_t == n_d > 0   # the non-pad positions of to_recover[:, 1:] (a span drawn near the end can run into the padding)
    else:
        loss_d = models[1](src_inputs=batch["captions"], src_pads=batch["caption_mask"], neg_samples=batch["neg"],
                           neg_mask=batch["neg_mask"], pad_idx=tp.pad_token_id(), src_langs=batch["langs"], tgt_langs=batch["langs"],
                           batch=batch)
        assert n_t == 0
    assert bool(torch.isfinite(loss_t)) and float(loss_t) == float(loss_d.detach()), (float(loss_t), float(loss_d.detach()))
