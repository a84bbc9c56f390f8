"""The measured values behind tests/test_gpu_resume.py, written to profiles/resume_parity.json (needs the GPU):

  * spread: the same 12 uninterrupted toy steps run six times from the same seed -- the worst per-tensor rel_err of five
    repeats against the first over weights and both moments, over all tensors and without the attention key biases (their gradient is zero in
    exact arithmetic: rounding noise that Adam normalises, tests/test_gpu_resume.py).  No resume code is involved: this is what
    the float atomics of the training step do.
  * resumed: 6 steps + snapshot + fresh objects + load + 6 steps, against the uninterrupted run (same measure).
  * control: the same second half from the weights alone (fresh optimizer).
  * snapshot: wall time of one snapshot (save_train_state) at C1 size (6+6 layers, d 512, 30k ids, bf16) beside the step time
    of the same model on one synthetic batch of 64 x 128.

Usage: python tools/resume_measure.py [--out profiles/resume_parity.json] [--no-c1]"""
import argparse
import json
import os
import pathlib
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parity():
    from tests import test_gpu_resume as T
    from tests.util import TOL
    runs = []
    for _ in range(6):  # the spread is itself a sample: five repeats against the first run, the worst of them counts
        t = T.make(T.SEED)
        T.run(t, 12)
        runs.append(T.buffers(t))
    both = lambda got, want: {"all_tensors": T.distance(got, want, skip=None), "without_key_biases": T.distance(got, want)}
    samples = [both(r, runs[0]) for r in runs[1:]]
    spread = {which: {name: max(s[which][name] for s in samples) for name in ("weights", "exp_avg", "exp_avg_sq")}
              for which in ("all_tensors", "without_key_biases")}
    with tempfile.TemporaryDirectory() as d:
        out = T.continuation(pathlib.Path(d), 6, 12)
    resumed = both(out["resumed"]["buffers"], out["whole"]["buffers"])
    control = both(out["control"]["buffers"], out["whole"]["buffers"])
    from tests.util import rel_err

    def worst(got, want, n=6):
        return {name: sorted(((rel_err(got[name][k], want[name][k]), k) for k in want[name]), reverse=True)[:n] for name in want}

    return {"steps": 12, "snapshot_after": 6, "project_bar_fp32": TOL[torch.float32], "test_bar": T.BAR, "left_out": list(T.NOISE_ONLY),
            "spread_same_seed_twice": spread, "spread_samples_without_key_biases": [s["without_key_biases"] for s in samples],
            "worst_tensors": {"spread": worst(runs[1], runs[0]), "resumed": worst(out["resumed"]["buffers"], out["whole"]["buffers"])},
            "resumed_vs_uninterrupted": resumed, "weights_only_control_vs_uninterrupted": control,
            "exact": {"visited": out["resumed"]["visited"] == out["whole"]["visited"],
                      "lr": out["resumed"]["lr"] == out["whole"]["lr"], "torch_rng": bool(torch.equal(out["resumed"]["rng"], out["whole"]["rng"]))}}


def snapshot_time():
    from imagetranslate_amd.checkpoint import load_train_state, save_train_state
    from imagetranslate_amd.parallel import train_step
    from imagetranslate_amd.seq2seq import Seq2Seq
    from imagetranslate_amd.textprocessor import SyntheticTextProcessor
    from imagetranslate_amd.trainer import Trainer
    from imagetranslate_amd.utils import build_optimizer
    torch.manual_seed(1)
    B, S, V = 64, 128, 30000
    model = Seq2Seq(SyntheticTextProcessor(V), lang_dec=False, enc_layer=6, dec_layer=6, embed_dim=512, intermediate_dim=2048,
                    num_attention_heads=8)
    model.set_compute_dtype(torch.bfloat16)
    model = model.cuda().train()
    opt = build_optimizer(model, 1e-4, 4000)
    trainer = Trainer(model, opt)
    src, tgt = torch.randint(7, V, (B, S)), torch.randint(7, V, (B, S))
    batch = {"src_texts": src, "dst_texts": tgt, "src_pad_mask": src != 0, "dst_pad_mask": tgt != 0,
             "src_langs": torch.zeros(B, dtype=torch.long), "dst_langs": torch.ones(B, dtype=torch.long)}
    batch = {k: v.cuda() for k, v in batch.items()}
    for _ in range(5):
        train_step(model, opt, batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        train_step(model, opt, batch)
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) / 20 * 1e3
    times, load_ms = [], None
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "train_state.pt")
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            save_train_state(path, trainer)
            times.append((time.perf_counter() - t0) * 1e3)
        size = os.path.getsize(path)
        t0 = time.perf_counter()
        load_train_state(path, trainer)
        torch.cuda.synchronize()
        load_ms = (time.perf_counter() - t0) * 1e3
    return {"model": "6+6 layers, d 512, ff 2048, 30000 ids, bf16 compute", "file_bytes": size, "step_ms": step_ms,
            "snapshot_ms": times, "load_ms": load_ms, "save_steps_default": 10000,
            "share_of_training_time_at_default_cadence": min(times) / (10000 * step_ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resume_parity.json"))
    ap.add_argument("--no-c1", action="store_true")
    args = ap.parse_args()
    result = {"parity": parity()}
    if not args.no_c1:
        result["snapshot"] = snapshot_time()
    with open(args.out, "w") as fp:
        json.dump(result, fp, indent=1)
        fp.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
