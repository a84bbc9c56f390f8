"""Scoring tail and whole Seq2Seq.score at the C1 size (B 64, S = T = 128, V 30000, d 512, bf16), plain and ragged:
the fused projection + log-sum-exp kernel (imt_score_rows) against today's chain (output layer GEMM -> log-softmax ->
gather -> per-sentence mean) on the SAME decoder rows, alternating the two in one process.

  (a) tail alone: decoder rows -> per-sentence scores, device-event medians of >= 50 timed calls each after warm-up;
  (b) whole score() against forward(log_softmax=True) + gather + per-sentence mean;
  (c) growth of torch.cuda.max_memory_allocated during each;
plus the algorithmic bytes / FLOPs of the tail from the shapes.  Prints one JSON line and writes it to
<out dir>/score_tail.json.  Usage: python tools/score_bench.py [out dir] [timed calls]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import CONFIGS, build_model, make_batch  # noqa: E402
from imagetranslate_amd import hip_ops as O  # noqa: E402
from imagetranslate_amd.param_store import store_of  # noqa: E402
from imagetranslate_amd.seq2seq import DecoderStream, _LogSoftmaxFn  # noqa: E402


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
    return {"median_ms": round(statistics.median(ms), 4), "p10_ms": round(q[0], 4), "p90_ms": round(q[-1], 4),
            "min_ms": round(min(ms), 4), "calls": len(ms)}


def _peak_growth(f):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = f()
    torch.cuda.synchronize()
    grow = torch.cuda.max_memory_allocated() - base
    del out
    return int(grow)


def run_config(name, calls):
    c = CONFIGS[name]
    dev = torch.device("cuda")
    model = build_model(c, torch.bfloat16, dev).eval()
    b = make_batch(c, 1234, dev)
    args = (b["src_texts"], b["dst_texts"], b["src_pad_mask"], b["dst_pad_mask"], b["src_langs"], b["dst_langs"])
    tgt, tmask = b["dst_texts"], b["dst_pad_mask"]
    with torch.no_grad():
        sel_idx, targets = model._selection(tgt, tmask)
        enc = model.encode(args[0], args[2], model._lang_grid(args[4], args[0].size(1), dev))[0]
        streams = [DecoderStream(model._decoder_for(1), enc, args[2], None)]
        rows = model._decode(streams, tgt, tmask, model._lang_grid(args[5], tgt.size(1), dev), sel_idx=sel_idx).contiguous()
    counts = tmask[:, 1:].sum(1, dtype=torch.int64)
    offsets = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=offsets[1:])
    seg_of_row = torch.repeat_interleave(torch.arange(counts.numel(), device=dev), counts)
    out_layer = model.output_layer[1]
    store = store_of(out_layer).ensure()
    w, bias = store.views(torch.bfloat16, out_layer.layer.weight, out_layer.layer.bias)
    V, K = w.shape
    N = rows.shape[0]

    def tail_fused():
        return O.score_rows(rows, w, bias, targets, seg_offsets=offsets, normalize=True)[2]

    def chain_scores(lp):
        picked = lp.gather(1, targets.unsqueeze(1)).squeeze(1)
        return torch.zeros(counts.numel(), device=dev, dtype=torch.float32).index_add_(0, seg_of_row, picked) / counts

    def tail_chain():
        with torch.no_grad():
            return chain_scores(_LogSoftmaxFn.apply(out_layer(rows)))

    def whole_fused():
        return model.score(*args)

    def whole_chain():
        with torch.no_grad():
            return chain_scores(model(*args, log_softmax=True))

    diff = float((tail_fused() - tail_chain()).abs().max())
    t_fused, t_chain = _timed([tail_fused, tail_chain], calls)
    w_fused, w_chain = _timed([whole_fused, whole_chain], max(20, calls // 2), warmup=3)
    tiles = (V + 255) // 256
    res = {
        "rows": N, "V": V, "K": K, "sentences": int(counts.numel()),
        "tail_fused": _stats(t_fused), "tail_chain": _stats(t_chain),
        "tail_speedup_median": round(statistics.median(t_chain) / statistics.median(t_fused), 3),
        "score_fused": _stats(w_fused), "score_chain": _stats(w_chain),
        "peak_memory_growth_bytes": {"tail_fused": _peak_growth(tail_fused), "tail_chain": _peak_growth(tail_chain),
                                     "score_fused": _peak_growth(whole_fused), "score_chain": _peak_growth(whole_chain)},
        "tail_algorithmic": {
            "flops": 2.0 * N * V * K,
            "fused_bytes": (N * K + V * K + V) * 2 + N * (2 * 8 * tiles + 2 * 4 + 8 + 4),
            "chain_bytes": (N * K + V * K + V) * 2 + N * V * 2 + N * V * 2 + N * V * 4 + N * (8 + 4 + 4),
        },
        "max_abs_score_difference_fused_vs_chain": diff,
    }
    del model
    return res


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 300
    assert calls >= 50, "at least 50 timed calls each"
    res = {"bench": "score_tail", "dtype": "bf16", "device": torch.cuda.get_device_name(0),
           "method": "device events, fused and chain alternating in one process", "c1": run_config("c1", calls),
           "c1ragged": run_config("c1ragged", calls)}
    line = json.dumps(res)
    print(line)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "score_tail.json"), "w") as fw:
        fw.write(line + "\n")


if __name__ == "__main__":
    main()
