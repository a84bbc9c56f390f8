#!/usr/bin/env python3
"""The two secondary workloads of SURVEY section 8(d) on one MI355X (the headline C1 stays in bench.py):
  C3 captioning: region features [32,49,2048] -> fc -> 6-layer decoder d=512 -> captions [32,32]   (0.265 TFLOP/step)
  C3obj        : C3 plus the object stream: detector features [32,100,1024] with a seeded random number of real detections
                 per image -> object head -> second 6-layer decoder (obj_decoder) -> sigmoid-gated mix; also the object head's
                 own forward + backward time
  C4 MASS      : monolingual src [64,256], span of int(255/2) tokens masked on the device, 6L/6L d=512 (4.27 TFLOP/step)
  multimodal   : ImageMassSeq2Seq's image steps -- the contrastive tail alone (three poolings + loss, forward + backward;
                 B=64, S=128, Nn=64, R=49, d=512, bf16) fused and as the torch-operator composition it replaces, and one gated
                 text + image step at the C1 shape; also written to profiles/multimodal_tail.json
Prints one JSON line per workload: ms/step, target tokens/s, TFLOP/s against the algorithmic FLOP counts of the survey."""
import json, os, random, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagetranslate_amd.image_model import ImageCaptioning, ImageMassSeq2Seq
from imagetranslate_amd.textprocessor import SyntheticTextProcessor
from imagetranslate_amd.utils import AdamInverseSqrtWithWarmup, mass_mask_device

V, d, ff, heads = 30000, 512, 2048, 8
tp = SyntheticTextProcessor(V)
dev = torch.device("cuda")


def timed(step, warmup=5, steps=20):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        n = step()
    torch.cuda.synchronize()
    sec = (time.perf_counter() - t0) / steps
    if "--breakdown" in sys.argv:  # per-kernel-kind table of the library's launch timer, to stderr
        from bench import profile_pass
        for r in profile_pass(step)[:14]:
            print("    %-28s %4d launches %8.3f ms/step %7.1f TFLOP/s" % (r["kind"], r["launches"], r["ms"], r["flops"] / max(r["ms"], 1e-9) / 1e9), file=sys.stderr)
    return sec, n


def c3():
    torch.manual_seed(1234)
    m = ImageCaptioning(tp, lang_dec=False, enc_layer=6, dec_layer=6, embed_dim=d, intermediate_dim=ff, use_obj=False,
                        num_attention_heads=heads, image_feat_dim=2048)
    m.set_compute_dtype(torch.bfloat16)
    m = m.to(dev).train()
    opt = AdamInverseSqrtWithWarmup(m.parameters(), lr=1e-4, betas=(0.9, 0.98), warmup_updates=4000)
    g = torch.Generator().manual_seed(1234)
    feats = torch.randn(32, 49, 2048, generator=g).to(dev)
    cap = torch.randint(6, V, (32, 32), generator=g); cap[:, 0] = 6; cap[:, -1] = 4
    cap = cap.to(dev)
    langs = torch.ones(32, dtype=torch.long)

    def step():
        loss, n = m.loss_fused(batch={"images": feats}, tgt_inputs=cap, tgt_langs=langs, tgt_mask=cap != 0, pad_idx=0)
        loss.backward()
        opt.step(max_grad_norm=1.0, zero_grad=True)
        return n
    sec, n = timed(step)
    return {"workload": "C3 captioning: feats [32,49,2048] -> 6L decoder d=512, captions [32,32]", "ms_per_step": round(1e3 * sec, 3),
            "tokens_per_s": round(n / sec, 1), "algorithmic_tflop_per_step": 0.265, "tflops": round(0.265 / sec, 1)}


def c3obj():
    torch.manual_seed(1234)
    m = ImageCaptioning(tp, lang_dec=False, enc_layer=6, dec_layer=6, embed_dim=d, intermediate_dim=ff, use_obj=True,
                        num_attention_heads=heads, image_feat_dim=2048)
    m.set_compute_dtype(torch.bfloat16)
    m = m.to(dev).train()
    opt = AdamInverseSqrtWithWarmup(m.parameters(), lr=1e-4, betas=(0.9, 0.98), warmup_updates=4000)
    g = torch.Generator().manual_seed(1234)
    feats = torch.randn(32, 49, 2048, generator=g).to(dev)
    cap = torch.randint(6, V, (32, 32), generator=g); cap[:, 0] = 6; cap[:, -1] = 4
    cap = cap.to(dev)
    langs = torch.ones(32, dtype=torch.long)
    labels = torch.zeros(32, 100, dtype=torch.long)
    for b, c in enumerate(torch.randint(1, 101, (32,), generator=g).tolist()):
        labels[b, :c] = torch.randint(1, 91, (c,), generator=g)
    labels = labels[:, :int((labels != 0).sum(1).max())]  # the loader trims to the batch's largest count
    n_obj = labels.size(1)
    xy = torch.rand(32, n_obj, 2, generator=g) * 600
    objects = {"feats": torch.randn(32, n_obj, 1024, generator=g).to(dev), "boxes": torch.cat([xy, xy + 100], -1).to(dev),
               "labels": labels.to(dev)}
    batch = {"images": feats, "objects": objects}

    def step():
        loss, n = m.loss_fused(batch=batch, tgt_inputs=cap, tgt_langs=langs, tgt_mask=cap != 0, pad_idx=0)
        loss.backward()
        opt.step(max_grad_norm=1.0, zero_grad=True)
        return n
    sec, n = timed(step)

    def head_step():
        out = m.image_model.objects_forward(objects, torch.bfloat16)
        out.backward(torch.ones_like(out))
        return 0
    head_sec, _ = timed(head_step)
    return {"workload": "C3obj captioning + object stream: C3 + objects [32,%d,1024] -> 6L obj_decoder d=512" % n_obj,
            "ms_per_step": round(1e3 * sec, 3), "tokens_per_s": round(n / sec, 1),
            "object_head_fwd_bwd_ms": round(1e3 * head_sec, 3), "object_head_share": round(head_sec / sec, 4)}


def c4():
    torch.manual_seed(1234)
    m = ImageMassSeq2Seq(tp, lang_dec=False, enc_layer=6, dec_layer=6, embed_dim=d, intermediate_dim=ff, num_attention_heads=heads)
    m.set_compute_dtype(torch.bfloat16)
    m = m.to(dev).train()
    opt = AdamInverseSqrtWithWarmup(m.parameters(), lr=1e-4, betas=(0.9, 0.98), warmup_updates=4000)
    g = torch.Generator().manual_seed(1234)
    src = torch.randint(6, V, (64, 256), generator=g); src[:, 0] = 5; src[:, -1] = 4
    pad_idx = torch.full((64,), 255, dtype=torch.long)
    langs = torch.zeros(64, dtype=torch.long)
    src_dev = src.to(dev)

    def step():
        masked = mass_mask_device(0.3, pad_idx, src_dev.clone(), tp, seed=random.getrandbits(62))
        loss, n = m.loss_fused(src_inputs=masked["src_text"], tgt_inputs=masked["to_recover"], src_langs=langs, pad_idx=0,
                               tgt_positions=masked["positions"])
        loss.backward()
        opt.step(max_grad_norm=1.0, zero_grad=True)
        return n
    sec, n = timed(step)
    return {"workload": "C4 MASS: src [64,256], 127-token span masked on device, 6L/6L d=512", "ms_per_step": round(1e3 * sec, 3),
            "tokens_per_s": round(n / sec, 1), "algorithmic_tflop_per_step": 4.273, "tflops": round(4.273 / sec, 1)}


def multimodal():
    from imagetranslate_amd import hip_ops as O
    B, S, Nn, R = 64, 128, 64, 49
    g = torch.Generator().manual_seed(1234)
    bf = torch.bfloat16
    enc, neg, img = (torch.randn(n, s, d, generator=g).to(dev, bf) for n, s in ((B, S), (Nn, S), (B, R)))
    lens = torch.randint(S // 2, S + 1, (B + Nn,), generator=g)
    mask = (torch.arange(S)[None, :] < lens[:, None]).to(dev)
    we, wi = (torch.randn(d, generator=g) * 0.05).to(dev, bf), (torch.randn(d, generator=g) * 0.05).to(dev, bf)
    be, bi = torch.zeros(1, device=dev, dtype=bf), torch.zeros(1, device=dev, dtype=bf)
    gw, gb = torch.zeros(d, device=dev), torch.zeros(1, device=dev)
    txt = torch.empty(B + Nn, d, device=dev)

    def fused():  # what image_model._ContrastiveTailFn runs, forward then backward
        _, p_e, n_e = O.attn_pool_fwd(enc, we, be, mask[:B], out=txt[:B])
        _, p_n, n_n = O.attn_pool_fwd(neg, we, be, mask[B:], out=txt[B:])
        iu, p_i, n_i = O.attn_pool_fwd(img, wi, bi, None)
        loss, d_img, d_txt = O.contrastive(iu, txt)
        O.attn_pool_bwd(enc, we, mask[:B], txt[:B], p_e, n_e, d_txt[:B], gw, gb)
        O.attn_pool_bwd(neg, we, mask[B:], txt[B:], p_n, n_n, d_txt[B:], gw, gb)
        O.attn_pool_bwd(img, wi, None, iu, p_i, n_i, d_img, gw, gb)
        return 0

    leaves = [t.clone().requires_grad_() for t in (enc, neg, img, we, be, wi, bi)]

    def torch_ops():  # src/image_model.py:240-263 with torch operators in bf16
        e, n, i, w1, b1, w2, b2 = leaves

        def pool(x, w, b, m):
            sc = x @ w + b
            if m is not None:
                sc = sc.masked_fill(~m, -10000.0)
            v = torch.einsum("bfd,bf->bd", x, torch.softmax(sc, dim=1))
            return v / (torch.norm(v, dim=-1, p=2).unsqueeze(-1) + 1e-4)
        t = torch.cat([pool(e, w1, b1, mask[:B]), pool(n, w1, b1, mask[B:])])
        im = pool(i, w2, b2, None)
        cross = im @ t.t()
        loss = torch.sum(torch.log(torch.sum(torch.exp(cross), dim=-1) + 1e-4) - (torch.diagonal(cross[:, :B], 0) + 1e-4)) / B
        for leaf in leaves:
            leaf.grad = None
        loss.backward()
        return 0
    f_runs, t_runs = [], []
    for _ in range(5):  # the two versions alternate in one process: a difference is read against their own spread
        f_runs.append(timed(fused, warmup=10, steps=200)[0])
        t_runs.append(timed(torch_ops, warmup=10, steps=200)[0])
    f_sec, t_sec = sorted(f_runs)[2], sorted(t_runs)[2]
    x_bytes = 2.0 * d * (B * S + Nn * S + B * R)
    plans = {"text S=%d" % S: O.attn_pool_plan(bf, S, d), "image R=%d" % R: O.attn_pool_plan(bf, R, d)}

    torch.manual_seed(1234)
    m = ImageMassSeq2Seq(tp, lang_dec=False, enc_layer=6, dec_layer=6, embed_dim=d, intermediate_dim=ff, num_attention_heads=heads,
                         image_feat_dim=2048)
    m.set_compute_dtype(bf)
    m = m.to(dev).train()
    opt = AdamInverseSqrtWithWarmup(m.parameters(), lr=1e-4, betas=(0.9, 0.98), warmup_updates=4000)
    src = torch.randint(6, V, (64, 128), generator=g).to(dev)
    tgt = torch.randint(6, V, (64, 128), generator=g).to(dev)
    feats = torch.randn(64, 49, 2048, generator=g).to(dev)
    langs = torch.ones(64, dtype=torch.long)

    def gated_step():
        loss, n = m.loss_fused(src_inputs=src, src_pads=src != 0, tgt_inputs=tgt, src_langs=langs, tgt_langs=langs, pad_idx=0,
                               batch={"images": feats})
        loss.backward()
        opt.step(max_grad_norm=1.0, zero_grad=True)
        return n
    g_sec, n = timed(gated_step)
    out = {"workload": "multimodal: contrastive tail B=64 S=128 Nn=64 R=49 d=512 bf16 (fwd + bwd); gated text + image step at C1",
           "tail_fused_ms": round(1e3 * f_sec, 4), "tail_torch_ops_ms": round(1e3 * t_sec, 4), "tail_speedup": round(t_sec / f_sec, 2),
           "tail_fused_ms_min_max": [round(1e3 * min(f_runs), 4), round(1e3 * max(f_runs), 4)],
           "tail_torch_ops_ms_min_max": [round(1e3 * min(t_runs), 4), round(1e3 * max(t_runs), 4)],
           "tail_x_megabytes": round(x_bytes / 1e6, 2), "pool_plans": plans,
           "gated_step_ms": round(1e3 * g_sec, 3), "gated_step_tokens_per_s": round(n / g_sec, 1)}
    os.makedirs(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"), exist_ok=True)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "multimodal_tail.json"), "w") as fw:
        json.dump(out, fw, indent=1, sort_keys=True)
        fw.write("\n")
    return out


if __name__ == "__main__":
    random.seed(0)
    want = [a for a in sys.argv[1:] if not a.startswith("--")]
    for fn in (c3, c3obj, c4, multimodal):
        if want and fn.__name__ not in want:
            continue
        print(json.dumps(fn()), flush=True)
