"""k nearest neighbours of N unit vectors among M (d 768, k 4; N = M = 16384 and 65536; bf16 and fp32): imt_knn_rows (the 256-tile
GEMM loop with a top-k epilogue, no [N, M] matrix) against the same search as torch operators on the same tensors -- x @ y.T in
blocks of at most 16384 x 16384, topk per block, a topk over the key blocks' lists -- alternating the two in one process, and
against the plain 256-tile product of the same operands from imt_gemm (fp32 output; at N = 65536 on the first 16384 queries, the
rate is what is compared): the gap in FLOP/s is the epilogue's price.  Device-event medians after warm-up.  The torch product of
bf16 operands is rounded to bf16 before its topk; the fused kernel ranks the fp32 sums.
Usage: python tools/knn_bench.py OUT.json [timed calls]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagetranslate_amd import hip_ops as O  # noqa: E402
from tools.caption2image_bench import _stats, _timed  # noqa: E402

D, K = 768, 4
SIZES = (16384, 65536)
BLOCK = 16384


def torch_knn(x, y, k):
    vals, idxs = [], []
    for r0 in range(0, x.shape[0], BLOCK):
        xv = x[r0:r0 + BLOCK]
        cv, ci = [], []
        for c0 in range(0, y.shape[0], BLOCK):
            v, i = torch.topk(xv @ y[c0:c0 + BLOCK].t(), k, dim=1)
            cv.append(v)
            ci.append(i + c0)
        if len(cv) > 1:
            cv, ci = torch.cat(cv, dim=1), torch.cat(ci, dim=1)
            v, at = torch.topk(cv, k, dim=1)
            i = ci.gather(1, at)
        vals.append(v)
        idxs.append(i)
    return torch.cat(vals), torch.cat(idxs)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "knn_rows.json"
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    results = []
    for n in SIZES:
        base_x = torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=-1).to(dev)
        base_y = torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=-1).to(dev)
        for dtype, name in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
            x, y = base_x.to(dtype), base_y.to(dtype)
            rows = min(n, BLOCK)
            c = torch.empty((rows, n), device=dev, dtype=torch.float32)
            fused = lambda: O.knn_rows(x, y, K)
            comp = lambda: torch_knn(x, y, K)
            gemm = lambda: O.gemm(x[:rows], y, O.IMT_NT, out=c)
            fv, fi = fused()
            tv, ti = comp()
            agree = float((fi == ti).float().mean())
            t_fused, t_comp, t_gemm = _timed([fused, comp, gemm], calls, warmup=3)
            flops, gflops = 2.0 * n * n * D, 2.0 * rows * n * D
            mf, mc, mg = (statistics.median(t) for t in (t_fused, t_comp, t_gemm))
            results.append({
                "N": n, "M": n, "d": D, "k": K, "dtype": name,
                "knn_rows": dict(_stats(t_fused), tflops=round(flops / mf / 1e9, 2)),
                "torch_ops": dict(_stats(t_comp), tflops=round(flops / mc / 1e9, 2)),
                "imt_gemm_256_tile": dict(_stats(t_gemm), rows=rows, tflops=round(gflops / mg / 1e9, 2)),
                "speedup_median_vs_torch_ops": round(mc / mf, 3),
                "rate_vs_plain_gemm": round((flops / mf) / (gflops / mg), 3),
                "indices_equal_to_torch_ops": round(agree, 6),
            })
            del c
    res = {"bench": "knn_rows", "device": torch.cuda.get_device_name(0), "results": results,
           "method": "device events, medians, the three paths alternating in one process after 3 warm-up rounds",
           "workload": "all-pairs inner products of unit vectors + the %d best per row" % K}
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fw:
        fw.write(text + "\n")


if __name__ == "__main__":
    main()
