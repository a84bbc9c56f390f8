"""Lexical-proposal tail of Seq2Seq (attention over the proposed words' embeddings + gate + LayerNorm) in bf16: the fused kernel
pair (Seq2Seq.attend_proposal: imt_proposal_attn_fwd / _bwd) against the same function as torch operators
(Seq2Seq._attend_proposal_torch) on the same tensors, alternating the two in one process.  Training shapes B 64, T - 1 127, d 512
with P 16 and P 128, forward + backward; the beam-search shape rows 64 x 5, rows_per_group 5, P 128, forward only (no gradient
exists there).  Device-event medians after warm-up.  Writes <out dir>/proposal_tail.json (times, nothing fixed in advance) and
<out dir>/proposal_parity.json (the bf16 errors of both paths against fp64, per tensor: tests/proposal_oracle.bf16_errors).
Usage: python tools/proposal_bench.py [out dir] [timed calls]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagetranslate_amd.seq2seq import Seq2Seq  # noqa: E402
from imagetranslate_amd.textprocessor import SyntheticTextProcessor  # noqa: E402

B, T1, D, BEAM, V = 64, 127, 512, 5, 30000


def _timed(fns, calls, warmup=5):
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
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev, bf = torch.device("cuda"), torch.bfloat16
    torch.manual_seed(0)
    model = Seq2Seq(SyntheticTextProcessor(V), lang_dec=False, enc_layer=1, dec_layer=1, embed_dim=D, intermediate_dim=D,
                    num_attention_heads=8, use_proposals=True).cuda().train()
    model.set_compute_dtype(bf)
    g = torch.Generator().manual_seed(0)
    res = {"bench": "proposal_tail", "dtype": "bf16", "device": torch.cuda.get_device_name(0),
           "method": "device events, medians, fused and torch operators alternating in one process after 5 warm-up rounds",
           "shapes": {}}
    for name, P, beam in (("train_P16", 16, False), ("train_P128", 128, False), ("beam5_P128", 128, True)):
        props = torch.randint(6, V, (B, P), generator=g)
        lens = torch.randint(1, P + 1, (B,), generator=g)
        props[torch.arange(P)[None] >= lens[:, None]] = 0
        props = props.to(dev)
        shape = (B * BEAM, D) if beam else (B, T1, D)
        x = torch.randn(shape, generator=g).to(dev, bf)
        dy = torch.randn(shape, generator=g).to(dev, bf)

        def run(fn, **kw):
            if beam:
                with torch.no_grad():
                    return fn(x, props, 0, **kw)
            xl = x.clone().requires_grad_()
            fn(xl, props, 0, **kw).backward(dy)
            return xl.grad

        fused = lambda: run(model.attend_proposal, **({"rows_per_group": BEAM} if beam else {}))
        torch_ops = lambda: run(model._attend_proposal_torch)
        t_fused, t_torch = _timed([fused, torch_ops], calls)
        res["shapes"][name] = {
            "workload": ("rows=%d rows_per_group=%d P=%d d=%d, forward" % (B * BEAM, BEAM, P, D)) if beam else
                        ("B=%d T-1=%d P=%d d=%d, forward and backward" % (B, T1, P, D)),
            "fused": _stats(t_fused), "torch_ops": _stats(t_torch),
            "speedup_median": round(statistics.median(t_torch) / statistics.median(t_fused), 3)}
        model.zero_grad()
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "proposal_tail.json"), "w") as fw:
        fw.write(text + "\n")
    # accuracy of both paths in bf16 against fp64 on the bf16-rounded inputs (the figures tests/test_gpu_proposal.py asserts on)
    from tests.proposal_oracle import bf16_errors
    parity = {"bench": "proposal_parity", "dtype": "bf16", "reference": "fp64 on the bf16-rounded states, table and upstream gradient",
              "error": "max |a - ref| / max |ref| per tensor", "cases": {}}
    for shape in ((3, 5, 7, 128), (2, 70, 130, 512)):
        parity["cases"]["G%d_r%d_P%d_d%d" % shape] = bf16_errors(*shape)
    text = json.dumps(parity, indent=1, sort_keys=True)
    print(text)
    with open(os.path.join(out_dir, "proposal_parity.json"), "w") as fw:
        fw.write(text + "\n")


if __name__ == "__main__":
    main()
