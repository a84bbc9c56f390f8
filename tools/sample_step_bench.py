#!/usr/bin/env python3
"""imt_sample_step against imt_beam_step on the C1 decoding shape (64 sentences x width 5, V = 30000, bf16 model, source 128).

  kernel alone   one process, ONE set of logits for all three calls, alternating sample(topk 0) / beam 5 / sample(topk 10); every
                 call bracketed by device events; median and p10 / p90 of 200 rounds.  (imt_beam_step is two launches, row top-k +
                 merge; the library's own per-launch profiler gives them apart.)
  whole step     BeamDecoder searches of 8 and 40 steps on the C1 model, alternating the three modes; the per-step time is the
                 difference over the 32 further steps (decoder step + projection + selection step, without the encoder and the set-up), median of 7.

Usage: python tools/sample_step_bench.py [out.json]      GPU only."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imagetranslate_amd.hip_ops as O  # noqa: E402
from bench import CONFIGS, build_model  # noqa: E402
from imagetranslate_amd import _lib as L  # noqa: E402
from imagetranslate_amd.seq_gen import BeamDecoder  # noqa: E402

B, WIDTH, V, S, T_MAX, STEP, ROUNDS = 64, 5, 30000, 128, 150, 40, 200


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(q * (len(xs) - 1))))]


def summary(xs):
    return {"median_us": round(statistics.median(xs), 2), "p10_us": round(pct(xs, 0.1), 2), "p90_us": round(pct(xs, 0.9), 2), "n": len(xs)}


def kernel_alone():
    rows = B * WIDTH
    g = torch.Generator(device="cuda").manual_seed(0)
    z = lambda *s, dtype: torch.zeros(*s, dtype=dtype, device="cuda")
    logits = torch.randn(rows, V, device="cuda", generator=g) * 3
    scores, sizes = torch.randn(rows, device="cuda", generator=g), torch.full((rows,), float(STEP), device="cuda")
    eos_in, max_lens = z(rows, dtype=torch.uint8), torch.full((B,), 140, dtype=torch.int64, device="cuda")
    hist = torch.randint(6, V, (rows, T_MAX), device="cuda", generator=g)
    slots = torch.arange(rows, dtype=torch.int32, device="cuda").unsqueeze(1).expand(rows, T_MAX).contiguous()
    cs, ci = z(rows, WIDTH, dtype=torch.float32), z(rows, WIDTH, dtype=torch.int32)
    o_scores, o_sizes, o_eos = z(rows, dtype=torch.float32), z(rows, dtype=torch.float32), z(rows, dtype=torch.uint8)
    o_hist, o_slots = z(rows, T_MAX, dtype=torch.int64), z(rows, T_MAX, dtype=torch.int32)
    o_parent, o_tok, cnt = z(rows, dtype=torch.int32), z(rows, dtype=torch.int64), z(T_MAX, dtype=torch.int32)
    keep = [logits, scores, sizes, eos_in, max_lens, hist, slots, cs, ci, o_scores, o_sizes, o_eos, o_hist, o_slots, o_parent, o_tok, cnt]

    def common(a):
        a.B, a.rep, a.V, a.step, a.t_max = B, WIDTH, V, STEP, T_MAX
        a.logits, a.ld = logits.data_ptr(), V
        a.scores_in, a.eos_in, a.max_lens = scores.data_ptr(), eos_in.data_ptr(), max_lens.data_ptr()
        a.hist_in, a.slots_in, a.pad_idx, a.eos = hist.data_ptr(), slots.data_ptr(), 0, 4
        a.scores_out, a.eos_out, a.hist_out, a.slots_out = o_scores.data_ptr(), o_eos.data_ptr(), o_hist.data_ptr(), o_slots.data_ptr()
        a.parent_out, a.tokens_out, a.eos_count = o_parent.data_ptr(), o_tok.data_ptr(), cnt.data_ptr()
        return a

    beam = common(L.BeamArgs())
    beam.beam, beam.sizes_in, beam.sizes_out, beam.len_penalty_ratio = WIDTH, sizes.data_ptr(), o_sizes.data_ptr(), 0.8
    beam.cand_scores, beam.cand_idx = cs.data_ptr(), ci.data_ptr()
    samples = {}
    for topk in (0, 10):
        a = common(L.SampleArgs())
        a.n, a.temperature, a.topk, a.seed = WIDTH, 1.0, topk, 1234
        samples[topk] = a
    calls = [("sample_topk0", lambda: O.sample_step(samples[0])), ("beam5", lambda: O.beam_step(beam)),
             ("sample_topk10", lambda: O.sample_step(samples[10]))]
    for _ in range(10):
        for _, f in calls:
            f()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in calls}
    for _ in range(ROUNDS):
        marks = []
        for name, f in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            marks.append((name, e0, e1))
        torch.cuda.synchronize()
        for name, e0, e1 in marks:
            times[name].append(e0.elapsed_time(e1) * 1e3)
    out = {name: summary(xs) for name, xs in times.items()}
    # the launches apart, by the library's profiler (events around every launch)
    lib = L.load()
    out["per_launch_mean_us"] = {}
    for name, f in calls:
        lib.imt_prof_enable(1)
        for _ in range(ROUNDS):
            f()
        torch.cuda.synchronize()
        rows_p = (L.ProfRow * 16)()
        n = lib.imt_prof_report(rows_p, 16)
        lib.imt_prof_enable(0)
        out["per_launch_mean_us"][name] = {r.kind.decode(): round(1e3 * r.total_ms / r.launches, 2) for r in rows_p[:n]}
    del keep
    return out


def whole_step():
    cfg = CONFIGS["c1"]
    model = build_model(cfg, torch.bfloat16, torch.device("cuda")).eval()
    g = torch.Generator().manual_seed(1234)
    src = torch.randint(6, cfg["V"], (B, S), generator=g)
    src[:, 0], src[:, -1] = 5, 4
    args = dict(src_inputs=src.cuda(), src_sizes=torch.full((B,), S), first_tokens=torch.full((B,), 5),
                src_mask=torch.ones(B, S, dtype=torch.bool).cuda(), src_langs=torch.zeros(B, dtype=torch.long).cuda(),
                tgt_langs=torch.ones(B, dtype=torch.long).cuda(), pad_idx=0, unpad_output=False)
    decs = [("sample_topk0", BeamDecoder(model, sampling=True, nsamples=WIDTH)),
            ("beam5", BeamDecoder(model, beam_width=WIDTH)),
            ("sample_topk10", BeamDecoder(model, sampling=True, nsamples=WIDTH, sampling_topk=10))]

    def run(dec, max_len):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = dec(max_len=max_len, **args)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, out[0].numel() - 1  # (time, steps run: fewer than asked if every row hit EOS)

    for _, dec in decs:
        run(dec, 9)
    per_step = {name: [] for name, _ in decs}
    for _ in range(7):
        for name, dec in decs:
            (t_long, n_long), (t_short, n_short) = run(dec, 41), run(dec, 9)
            per_step[name].append((t_long - t_short) / max(n_long - n_short, 1))
    return {name: summary(xs) for name, xs in per_step.items()}


def main():
    assert torch.cuda.is_available(), "GPU only"
    res = {"shape": {"B": B, "width": WIDTH, "V": V, "source": S, "dtype": "bf16", "config": "c1"},
           "kernel_alone": kernel_alone(), "whole_step": whole_step()}
    k = res["kernel_alone"]
    margin = k["beam5"]["p90_us"] - k["beam5"]["p10_us"]
    res["bar"] = {"rule": "sample median <= beam5 median + beam5 (p90 - p10)", "margin_us": round(margin, 2),
                  "met": {name: k[name]["median_us"] <= k["beam5"]["median_us"] + margin for name in ("sample_topk0", "sample_topk10")}}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fw:
            fw.write(text + "\n")


if __name__ == "__main__":
    main()
