#!/usr/bin/env python3
"""The 256-tile kernel with its in-loop DMA or its MFMAs switched off: what each half of the K loop costs alone, HBM-cold
operands.  The bits are gemm_xl.hpp's xl_k_loop `dbg` (bit 0 no tile products, bit 1 no in-loop DMA), set through IMT_GEMM_DBG,
which the library reads once: this script starts one child process per setting.  GPU only; results in
profiles/r03_gemm_xl_ring.txt."""
import os, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [(8192, 2048, 512), (8192, 2048, 2048), (8192, 2048, 8192)]
def t(M, N, K, reps=30):
    import torch
    from imagetranslate_amd import hip_ops as O
    g = torch.Generator(device="cuda").manual_seed(1)
    sets = []
    for _ in range(10):
        A = torch.randn((M, K), device="cuda", generator=g).bfloat16()
        B = (torch.randn((N, K), device="cuda", generator=g) * .05).bfloat16()
        sets.append((A, B, torch.empty(M, N, device="cuda", dtype=torch.bfloat16)))
    for A, B, o in sets[:2]: O.gemm(A, B, O.IMT_NT, out=o, force_general=6)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(reps):
        A, B, o = sets[r % 10]; O.gemm(A, B, O.IMT_NT, out=o, force_general=6)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps
if len(sys.argv) > 1:  # child: one setting, one line of times
    print(" ".join("%.2f" % t(*s) for s in SHAPES))
    sys.exit(0)
res = {}
for name, bits in (("full", "0"), ("DMA only", "1"), ("MFMA only", "2")):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=dict(os.environ, IMT_GEMM_DBG=bits), check=True,
                         capture_output=True, text=True, timeout=300).stdout
    res[name] = [float(x) for x in out.split()]
for i, (M, N, K) in enumerate(SHAPES):
    nt = K // 64
    print("NT %d x %d x %d: " % (M, N, K) + " | ".join("%s %.1f us (%.2f per 64-deep K tile)" % (n, v[i], v[i] / nt) for n, v in res.items()), flush=True)
