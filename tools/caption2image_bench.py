"""Tail of Caption2Image at B 64, S 32, d 768, bf16: dropout + sentence pooling + the 49 d-wide linear layer + L2 loss, forward
and backward, on the fused kernels (imt_sent_pool_fwd / _bwd, imt_gemm, imt_l2_dist) against the same steps as torch operators
on the same tensors, alternating the two in one process.  Device-event medians after warm-up; the pooling kernels are also timed
alone and their algorithmic bytes (x read once per pass -- the sentence fits in LDS at this shape --, dx written, the small
outputs) are set against the rate of a large device-to-device copy measured in the same process.  Prints one JSON document and
writes it to <out dir>/caption2image_tail.json.  Usage: python tools/caption2image_bench.py [out dir] [timed calls]"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagetranslate_amd import hip_ops as O  # noqa: E402

B, S, D, REGIONS, P, SEED = 64, 32, 768, 49, 0.1, 1234


def _timed(fns, calls, warmup=10):
    """Alternate the callables; per callable the list of device-event times (ms)."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)] for _ in fns]
    for i in range(calls):
        for k, f in enumerate(fns):
            ev[k][i][0].record()
            f()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    return [[a.elapsed_time(b) for a, b in row] for row in ev]


def _stats(ms):
    q = statistics.quantiles(ms, n=10)
    return {"median_ms": round(statistics.median(ms), 5), "p10_ms": round(q[0], 5), "p90_ms": round(q[-1], 5), "calls": len(ms)}


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev, bf = torch.device("cuda"), torch.bfloat16
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, S, D, generator=g).to(dev, bf)
    lens = torch.randint(S // 2, S + 1, (B,), generator=g)
    mask = (torch.arange(S)[None, :] < lens[:, None]).to(dev)
    w = (torch.randn(D, generator=g) * 0.05).to(dev, bf)
    b = torch.zeros(1, device=dev, dtype=bf)
    W = (torch.randn(REGIONS * D, D, generator=g) * 0.02).to(dev, bf)
    Wb = torch.zeros(REGIONS * D, device=dev, dtype=bf)
    target = (torch.randn(B, REGIONS * D, generator=g) * 0.2).to(dev, bf)
    gW = torch.zeros(REGIONS * D, D, device=dev)
    gWb, gw, gb = torch.zeros(REGIONS * D, device=dev), torch.zeros(D, device=dev), torch.zeros(1, device=dev)
    assert O.attn_pool_plan(bf, S, D) == 1

    def fused():
        v, probs = O.sent_pool_fwd(x, w, b, mask, dropout_p=P, dropout_seed=SEED)
        y = O.gemm(v, W, O.IMT_NT, bias=Wb)
        loss, dy = O.l2_dist(y, target)
        dv = O.gemm(dy, W, O.IMT_NN)
        sk = O.dw_split_k(B, REGIONS * D, D, 256)
        O.gemm(dy, v, O.IMT_TN, out=gW, accumulate=(sk == 1), split_k=sk, a_colsum=gWb)
        dx = O.sent_pool_bwd(x, w, mask, probs, dv, gw, gb, dropout_p=P, dropout_seed=SEED)
        return loss, dx

    leaves = [t.clone().requires_grad_() for t in (x, w, b, W, Wb)]

    def torch_ops():
        for t in leaves:
            t.grad = None
        xl, wl, bl, Wl, Wbl = leaves
        xd = F.dropout(xl, p=P)
        scores = (xd @ wl + bl).masked_fill(~mask, -10000.0)
        v = torch.einsum("bfd,bf->bd", xd, torch.softmax(scores, dim=1))
        loss = torch.dist(F.linear(v, Wl, Wbl), target, 2) / B
        loss.backward()
        return loss, xl.grad

    # the pooling kernels alone, and a large copy as the memory-rate yardstick
    v0, probs0 = O.sent_pool_fwd(x, w, b, mask, dropout_p=P, dropout_seed=SEED)
    dv0 = torch.randn(B, D, generator=g).to(dev, bf)
    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    t_fused, t_torch = _timed([fused, torch_ops], calls)
    t_fwd, t_bwd, t_copy = _timed([lambda: O.sent_pool_fwd(x, w, b, mask, dropout_p=P, dropout_seed=SEED),
                                   lambda: O.sent_pool_bwd(x, w, mask, probs0, dv0, gw, gb, dropout_p=P, dropout_seed=SEED),
                                   lambda: dst.copy_(src)], calls)
    xb = B * S * D * 2
    fwd_bytes = xb + B * S + B * D * 2 + B * S * 4
    bwd_bytes = 2 * xb + B * S + B * S * 4 + B * D * 2 + 2 * (B * D + B) * 4   # x read, dx written, partials written and folded
    copy_rate = 2 * src.numel() / (statistics.median(t_copy) * 1e-3)
    res = {
        "bench": "caption2image_tail", "dtype": "bf16", "device": torch.cuda.get_device_name(0),
        "workload": "B=%d S=%d d=%d, dropout %.1f + pooling + linear %d x %d + L2 loss, forward and backward" % (B, S, D, P, REGIONS * D, D),
        "method": "device events, medians, fused and torch operators alternating in one process after 10 warm-up rounds",
        "tail_fused": _stats(t_fused), "tail_torch_ops": _stats(t_torch),
        "speedup_median": round(statistics.median(t_torch) / statistics.median(t_fused), 3),
        "sent_pool_fwd": dict(_stats(t_fwd), algorithmic_bytes=fwd_bytes,
                              bytes_per_s=round(fwd_bytes / (statistics.median(t_fwd) * 1e-3), 1)),
        "sent_pool_bwd": dict(_stats(t_bwd), algorithmic_bytes=bwd_bytes,
                              bytes_per_s=round(bwd_bytes / (statistics.median(t_bwd) * 1e-3), 1)),
        "device_copy_256MiB": dict(_stats(t_copy), bytes_per_s=round(copy_rate, 1)),
    }
    res["sent_pool_fwd"]["share_of_copy_rate"] = round(res["sent_pool_fwd"]["bytes_per_s"] / copy_rate, 4)
    res["sent_pool_bwd"]["share_of_copy_rate"] = round(res["sent_pool_bwd"]["bytes_per_s"] / copy_rate, 4)
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "caption2image_tail.json"), "w") as fw:
        fw.write(text + "\n")


if __name__ == "__main__":
    main()
