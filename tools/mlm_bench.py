"""BERT masking for the masked LM: (a) imt_mlm_mask alone at B 64 x S 128 and B 64 x S 512 (p 0.15, V 30000) against the same
procedure as torch operators on the same device -- rand < p, the mask ANDs, a boolean index for the originals, nonzero for the
positions, where for the 80/10/10 replacement -- and against imt_select_plan on the same positions with the same number selected
(the floor for an ordered one-workgroup compaction: it draws nothing and replaces nothing); (b) a whole LM training step (6 layers,
d 512, 8 heads, ff 2048, V 30000, B 64, S 128, bf16; host batch -> device copy -> masking -> loss_fused -> backward -> clip + Adam)
with the kernel and with the torch-operator masking, in masked tokens per second.

(a) device-event medians, the paths alternating in one process after warm-up.  The kernel is timed twice: with the count from the
host (``mask_text_count``: nothing read back, what the trainer does) and with the count read back (one 4-byte copy, what the
operator chain cannot avoid: a boolean index and nonzero each wait for their sizes).  The host time of ``mask_text_count`` is
reported beside them.  (b) host clock around blocks of steps that end in a device synchronise, the two variants alternating.
Usage: python tools/mlm_bench.py OUT.json [timed calls] [timed steps per block]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagetranslate_amd import hip_ops as O  # noqa: E402
from imagetranslate_amd.lm import LM  # noqa: E402
from imagetranslate_amd.textprocessor import SyntheticTextProcessor  # noqa: E402
from imagetranslate_amd.train_lm import LMTrainer  # noqa: E402
from imagetranslate_amd.utils import _mlm_selected, build_optimizer, mask_text_count, mask_text_device  # noqa: E402
from tools.caption2image_bench import _stats, _timed  # noqa: E402

P, V = 0.15, 30000


def batch(B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    texts = torch.randint(7, V, (B, S), generator=g)
    lens = torch.randint(S // 2, S + 1, (B,), generator=g)
    pads = torch.arange(S)[None] < lens[:, None]
    texts[torch.arange(B), lens - 1] = 4
    texts[~pads] = 0
    return texts, pads, torch.zeros(B, dtype=torch.int64)


def torch_mask(texts, pads, tp, p=P):
    """mask_text as torch operators on the device (torch's generator in place of the counter-based one): returns what
    mask_text_device returns, out of place."""
    sel = (torch.rand(texts.shape, device=texts.device) < p) & pads
    targets = texts[sel]
    idx = torch.nonzero(sel.view(-1), as_tuple=False).view(-1).to(torch.int32)
    u = torch.rand(texts.shape, device=texts.device)
    rnd = torch.randint(len(tp.special_tokens), tp.vocab_size(), texts.shape, device=texts.device)
    new = torch.where(sel & (u < 0.8), torch.full_like(texts, tp.mask_token_id()), torch.where(sel & (u < 0.9), rnd, texts))
    return {"mask": sel, "targets": targets, "idx": idx, "texts": new}


def kernel_alone(tp, B, S, calls):
    texts, pads, _ = batch(B, S)
    seed = 1234
    n = mask_text_count(P, pads, texts, tp, seed)
    t0 = time.perf_counter()
    for _ in range(20):
        mask_text_count(P, pads, texts, tp, seed)
    count_ms = (time.perf_counter() - t0) / 20 * 1e3
    d_texts, d_pads = texts.cuda(), pads.cuda()
    work = d_texts.clone()
    sel = torch.from_numpy(_mlm_selected(P, pads.numpy(), texts.numpy(), 4, seed)).cuda()
    fns = [lambda: mask_text_device(P, d_pads, work, tp, seed, count=n),
           lambda: mask_text_device(P, d_pads, work, tp, seed),
           lambda: torch_mask(d_texts, d_pads, tp),
           lambda: O.select_plan(sel, d_texts, col0=0, count=n)]
    names = ["imt_mlm_mask_host_count", "imt_mlm_mask_count_read_back", "torch_ops", "imt_select_plan_floor"]
    times = _timed(fns, calls, warmup=10)
    med = {k: statistics.median(t) for k, t in zip(names, times)}
    row = {"B": B, "S": S, "positions": B * S, "selected": n, "mask_text_count_host_ms": round(count_ms, 4)}
    for k, t in zip(names, times):
        row[k] = _stats(t)
    row["torch_ops_over_kernel_host_count"] = round(med["torch_ops"] / med["imt_mlm_mask_host_count"], 2)
    row["torch_ops_over_kernel_read_back"] = round(med["torch_ops"] / med["imt_mlm_mask_count_read_back"], 2)
    row["kernel_host_count_over_select_plan"] = round(med["imt_mlm_mask_host_count"] / med["imt_select_plan_floor"], 2)
    return row


def train_step_bench(tp, steps, blocks=5):
    torch.manual_seed(0)
    model = LM(tp, enc_layer=6, embed_dim=512, intermediate_dim=2048, num_attention_heads=8)
    model = model.set_compute_dtype(torch.bfloat16).cuda().train()
    trainer = LMTrainer(model=model, mask_prob=P, optimizer=build_optimizer(model, 1e-4, 4000), clip=1, seed=1)
    data = [dict(zip(("texts", "pad_mask", "langs"), batch(64, 128, seed=s))) for s in range(8)]

    def kernel_step(i):
        return trainer.lm_step(data[i % len(data)], i)[1]

    def torch_step(i):
        b = data[i % len(data)]
        dev = model._device
        m = torch_mask(b["texts"].to(dev), b["pad_mask"].to(dev), tp)
        loss, n = model.loss_fused(m["texts"], b["pad_mask"], b["langs"], m["idx"], m["targets"])
        loss.backward()
        trainer._finish_micro_step(1)
        return n

    out = {"kernel": [], "torch_ops": []}
    tokens = {"kernel": 0, "torch_ops": 0}
    for name, fn in (("kernel", kernel_step), ("torch_ops", torch_step)):
        for i in range(10):
            fn(i)
    torch.cuda.synchronize()
    for blk in range(blocks):
        for name, fn in (("kernel", kernel_step), ("torch_ops", torch_step)):
            torch.cuda.synchronize()
            t0, n = time.perf_counter(), 0
            for i in range(steps):
                n += fn(blk * steps + i)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out[name].append(dt / steps * 1e3)
            tokens[name] += n
    res = {"config": "6 layers, d 512, h 8, ff 2048, V 30000, B 64, S 128, bf16, p 0.15", "steps_per_block": steps, "blocks": blocks}
    for name in out:
        ms = statistics.median(out[name])
        per_step = tokens[name] / (steps * blocks)
        res[name] = {"ms_per_step_median": round(ms, 4), "ms_per_step_blocks": [round(x, 4) for x in out[name]],
                     "masked_tokens_per_step": round(per_step, 1), "masked_tokens_per_s": round(per_step / ms * 1e3)}
    res["torch_ops_over_kernel"] = round(res["torch_ops"]["ms_per_step_median"] / res["kernel"]["ms_per_step_median"], 4)
    return res


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "mlm.json"
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 40
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    tp = SyntheticTextProcessor(V)
    res = {"bench": "mlm_mask", "device": torch.cuda.get_device_name(0),
           "kernel_alone": [kernel_alone(tp, 64, 128, calls), kernel_alone(tp, 64, 512, calls)],
           "train_step": train_step_bench(tp, steps),
           "method": "(a) device events, medians, the four paths alternating in one process after 10 warm-up rounds; (b) host clock "
                     "around blocks of steps ending in a device synchronise, the two variants alternating, after 10 warm-up steps each"}
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fw:
        fw.write(text + "\n")


if __name__ == "__main__":
    main()
