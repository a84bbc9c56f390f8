"""Word alignment of B sentence pairs (d 512; B 512 with S = T = 64, B 256 with S = T = 128; bf16 and fp32): imt_align_pairs (one
launch, no [B, S, T] matrix) against the same function as torch operators on the same tensors -- F.normalize twice, torch.bmm
into a [B, S, T] fp32 tensor, the range mask, max over dim 2 and dim 1, gather + compare -- alternating the two in one process.
Then the share of a whole ``align_batch`` call (two encoder passes of a 6-layer d = 512 model + the kernel + the copy of the
links to the host) that the kernel takes.  Device-event medians after warm-up; the ranges are the framed-sentence ones
(1, len - 1).  torch.max returns SOME index of the maximum, the kernel the lowest: the agreement of the links is reported, not
asserted.
Usage: python tools/align_bench.py OUT.json [timed calls]"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagetranslate_amd import align_pairs as AP  # noqa: E402
from imagetranslate_amd import hip_ops as O  # noqa: E402
from tools.caption2image_bench import _stats, _timed  # noqa: E402

D = 512
SHAPES = ((512, 64, 64), (256, 128, 128))


def torch_align(x, y, xr, yr, min_sim):
    """The torch-operator chain (it materialises the similarities and both normalised operands)."""
    S, T = x.shape[1], y.shape[1]
    sim = torch.bmm(F.normalize(x.float(), dim=-1), F.normalize(y.float(), dim=-1).transpose(1, 2))
    i, j = torch.arange(S, device=x.device), torch.arange(T, device=x.device)
    ok = ((i[None] >= xr[:, :1]) & (i[None] < xr[:, 1:]))[:, :, None] & ((j[None] >= yr[:, :1]) & (j[None] < yr[:, 1:]))[:, None, :]
    sim = sim.masked_fill(~ok, float("-inf"))
    fv, fi = sim.max(dim=2)
    bv, bi = sim.max(dim=1)
    keep = (bi.gather(1, fi) == i[None]) & (fv >= min_sim)
    return torch.where(keep, fi, torch.full_like(fi, -1)), fi, fv, bi, bv


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "align_pairs.json"
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    results = []
    for B, S, T in SHAPES:
        bx, by = torch.randn(B, S, D, generator=g).to(dev), torch.randn(B, T, D, generator=g).to(dev)
        xr = torch.tensor([[1, S - 1]] * B, dtype=torch.int32, device=dev)
        yr = torch.tensor([[1, T - 1]] * B, dtype=torch.int32, device=dev)
        for dtype, name in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
            x, y = bx.to(dtype), by.to(dtype)
            fused = lambda: O.align_pairs(x, y, xr, yr, 0.0)
            chain = lambda: torch_align(x, y, xr, yr, 0.0)
            agree = float((fused()[0] == chain()[0]).float().mean())
            t_fused, t_chain = _timed([fused, chain], calls, warmup=10)
            mf, mc = statistics.median(t_fused), statistics.median(t_chain)
            flops = 2.0 * B * S * T * D
            read = float(B * (S + T) * D * x.element_size())
            results.append({
                "B": B, "S": S, "T": T, "d": D, "dtype": name,
                "align_pairs": dict(_stats(t_fused), tflops=round(flops / mf / 1e9, 2), operand_gb_per_s=round(read / mf / 1e6, 1)),
                "torch_ops": dict(_stats(t_chain), tflops=round(flops / mc / 1e9, 2)),
                "speedup_median_vs_torch_ops": round(mc / mf, 3),
                "links_equal_to_torch_ops": round(agree, 6),
            })
    # the kernel's share of a whole align_batch call
    from imagetranslate_amd.seq2seq import Seq2Seq
    from imagetranslate_amd.textprocessor import SyntheticTextProcessor
    tp = SyntheticTextProcessor(8000)
    torch.manual_seed(0)
    model = Seq2Seq(tp, lang_dec=False, enc_layer=6, dec_layer=1, embed_dim=D, intermediate_dim=4 * D, num_attention_heads=8)
    model = model.cuda().eval()
    shares = []
    for dtype, name in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        model.set_compute_dtype(dtype)
        for B, S, T in SHAPES:
            ids = lambda n, w: [[5] + torch.randint(7, 8000, (w - 2,), generator=g).tolist() + [4] for _ in range(n)]
            src, dst = ids(B, S), ids(B, T)
            whole = lambda: AP.align_batch(model, src, dst, 0, 1, tp.pad_token_id(), 0.0)
            _, raw = AP.align_batch(model, src, dst, 0, 1, tp.pad_token_id(), 0.0, return_raw=True)
            kern = lambda: O.align_pairs(raw["x"], raw["y"], raw["x_range"], raw["y_range"], 0.0)
            t_whole, t_kern = _timed([whole, kern], max(10, calls // 5), warmup=3)
            mw, mk = statistics.median(t_whole), statistics.median(t_kern)
            shares.append({"B": B, "S": S, "T": T, "d": D, "dtype": name, "encoder_layers": 6, "align_batch": _stats(t_whole),
                           "align_pairs": _stats(t_kern), "kernel_share_of_align_batch": round(mk / mw, 4)})
    res = {"bench": "align_pairs", "device": torch.cuda.get_device_name(0), "results": results, "align_batch": shares,
           "method": "device events, medians, the paths alternating in one process after warm-up rounds",
           "workload": "cosine of every token pair of B sentence pairs, arg-max in both directions, mutual links"}
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fw:
        fw.write(text + "\n")


if __name__ == "__main__":
    main()
