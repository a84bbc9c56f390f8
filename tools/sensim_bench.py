"""Tail of SenSim at B 64, 320 negatives per side, S 32, d 768, bf16: four attention poolings to unit vectors plus the two-sided
contrastive loss, forward and backward, on the fused kernels (imt_attn_pool_fwd / _bwd, imt_sensim_loss) against the same steps as
torch operators on the same tensors, alternating the two in one process.  Device-event medians after warm-up; the loss call is
also timed alone.  Prints one JSON document and writes it to <out dir>/sensim_tail.json.
Usage: python tools/sensim_bench.py [out dir] [timed calls]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagetranslate_amd import hip_ops as O  # noqa: E402
from tools.caption2image_bench import _stats, _timed  # noqa: E402

B, NEG, S, D = 64, 320, 32, 768


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev, bf = torch.device("cuda"), torch.bfloat16
    g = torch.Generator().manual_seed(0)
    rows = (NEG, B, NEG, B)   # source negatives, sources, target negatives, targets
    xs = [torch.randn(n, S, D, generator=g).to(dev, bf) for n in rows]
    masks = [(torch.arange(S)[None, :] < torch.randint(S // 2, S + 1, (n,), generator=g)[:, None]).to(dev) for n in rows]
    w = (torch.randn(D, generator=g) * 0.05).to(dev, bf)
    b = torch.zeros(1, device=dev, dtype=bf)
    gw, gb = torch.zeros(D, device=dev), torch.zeros(1, device=dev)
    one = torch.ones(1, device=dev)
    assert O.attn_pool_plan(bf, S, D) == 1

    def fused():
        scat = torch.empty((NEG + B, D), device=dev, dtype=torch.float32)
        tcat = torch.empty((NEG + B, D), device=dev, dtype=torch.float32)
        outs = ((scat, 0, NEG), (scat, NEG, NEG + B), (tcat, 0, NEG), (tcat, NEG, NEG + B))
        saved = [O.attn_pool_fwd(x, w, b, m, out=buf[lo:hi]) for x, m, (buf, lo, hi) in zip(xs, masks, outs)]
        loss, d_s, d_t = O.sensim_loss(scat, tcat, B)
        grads = (d_s, d_s, d_t, d_t)
        dxs = [O.attn_pool_bwd(x, w, m, buf[lo:hi], sv[1], sv[2], du[lo:hi], gw, gb, du_scale=one)
               for x, m, (buf, lo, hi), sv, du in zip(xs, masks, outs, saved, grads)]
        return loss, dxs

    leaves = [t.clone().requires_grad_() for t in xs + [w, b]]

    def torch_ops():
        for t in leaves:
            t.grad = None
        wl, bl = leaves[4], leaves[5]

        def pool(x, mask):
            scores = (x @ wl + bl).masked_fill(~mask, -10000.0)
            v = torch.einsum("bfd,bf->bd", x, torch.softmax(scores, dim=1))
            return v / (torch.norm(v, dim=-1, p=2).unsqueeze(-1) + 1e-4)
        sneg, src, tneg, tgt = (pool(x, m) for x, m in zip(leaves[:4], masks))
        scat, tcat = torch.cat([sneg, src]), torch.cat([tneg, tgt])
        cross = torch.cat([src @ tcat.t(), tgt @ scat.t()], dim=1)
        loss = torch.sum(torch.log(torch.sum(torch.exp(cross), dim=-1) + 1e-4) - (torch.sum(src * tgt, dim=-1) + 1e-4)) / B
        loss.backward()
        return loss, [t.grad for t in leaves[:4]]

    # the loss call alone, on unit vectors the poolings produced
    scat0 = torch.cat([O.attn_pool_fwd(xs[0], w, b, masks[0])[0], O.attn_pool_fwd(xs[1], w, b, masks[1])[0]])
    tcat0 = torch.cat([O.attn_pool_fwd(xs[2], w, b, masks[2])[0], O.attn_pool_fwd(xs[3], w, b, masks[3])[0]])
    t_fused, t_torch = _timed([fused, torch_ops], calls)
    (t_loss,) = _timed([lambda: O.sensim_loss(scat0, tcat0, B)], calls)
    res = {
        "bench": "sensim_tail", "dtype": "bf16", "device": torch.cuda.get_device_name(0),
        "workload": "B=%d, %d negatives per side, S=%d d=%d: four poolings to unit vectors + two-sided contrastive loss, forward and "
                    "backward" % (B, NEG, S, D),
        "method": "device events, medians, fused and torch operators alternating in one process after 10 warm-up rounds",
        "launches_fused": 4 + 2 + 4 * 2,
        "tail_fused": _stats(t_fused), "tail_torch_ops": _stats(t_torch),
        "speedup_median": round(statistics.median(t_torch) / statistics.median(t_fused), 3),
        "sensim_loss": dict(_stats(t_loss), flops=6 * B * 2 * (NEG + B) * D),
    }
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "sensim_tail.json"), "w") as fw:
        fw.write(text + "\n")


if __name__ == "__main__":
    main()
