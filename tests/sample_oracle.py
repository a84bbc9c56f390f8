"""fp64 restatement of one ``imt_sample_step`` (include/imt_hip.h) in numpy -- TEST INFRASTRUCTURE ONLY.

The draws come from ``oracle.batch_oracle.counter_uniform`` (the generator of csrc/common.hpp, bit for bit) evaluated on
whole index arrays.  Besides the kernel's outputs ``sample_step_reference`` returns the GAP between the best and the second-best
perturbed value of every unmasked draw: an fp32 kernel can be compared token for token with this oracle wherever that gap is
well above fp32 rounding of the perturbed values (the tests use 1e-4, the threshold of ``tests/util.beam_reference_is_unambiguous``).
The kept set itself needs no such margin: it is decided by comparisons of the fp32 logits, which are exact.
"""
import numpy as np
import torch

from oracle.batch_oracle import counter_uniform

U_MIN = np.float32(2.0 ** -25)


def uniforms(seed: int, stream: int, index: np.ndarray) -> np.ndarray:
    """``counter_uniform`` over an array of indices (< 2^32), clamped from below like the kernel: float32, same shape."""
    u = counter_uniform(int(seed), int(stream), np.asarray(index, dtype=np.uint64))
    return np.maximum(np.asarray(u, dtype=np.float32), U_MIN)


def kept_mask(x32: np.ndarray, topk: int) -> np.ndarray:
    """[R, V] bool: the first ``topk`` indices of every row by (value descending, index ascending); all of them when off."""
    R, V = x32.shape
    if topk <= 0 or topk >= V:
        return np.ones((R, V), dtype=bool)
    order = np.argsort(-x32, axis=1, kind="stable")  # stable: equal values keep their index order
    kept = np.zeros((R, V), dtype=bool)
    np.put_along_axis(kept, order[:, :topk], True, axis=1)
    return kept


def sample_step_reference(logits, scores_in, eos_in, max_lens, hist_in, slots_in, step, B, n, rep, V, t_max, temperature, topk,
                          seed, pad, eos):
    """One step on CPU tensors (``logits`` [B*rep, V] fp32, the rest as in imt_sample_args).  Returns a dict of torch tensors:
    tokens, scores (fp64), eos, hist, slots, parent, eos_count (the step's increment), masked, gap (inf on masked rows)."""
    x32 = logits.detach().cpu().numpy().astype(np.float32)
    assert x32.shape == (B * rep, V)
    out_rows = np.arange(B * n)
    b, k = out_rows // n, out_rows % n
    parent = b * rep + (0 if rep == 1 else k)
    eos_p = eos_in.numpy().astype(bool)[parent]
    over = (max_lens.numpy()[b] < step + 1) if step > 1 else np.zeros(B * n, dtype=bool)
    masked = eos_p | over

    xr32 = x32[parent]
    x = xr32.astype(np.float64)
    kept = kept_mask(xr32, topk)
    index = out_rows[:, None].astype(np.uint64) * np.uint64(V) + np.arange(V, dtype=np.uint64)[None, :]
    u = uniforms(seed, step, index).astype(np.float64)
    val = x / np.float64(np.float32(temperature)) - np.log(-np.log(u))
    val[~kept] = -np.inf
    tok = np.argmax(val, axis=1)  # the first maximum: the lowest index
    if V > 1:
        top2 = -np.partition(-val, 1, axis=1)[:, :2]
        gap = top2[:, 0] - top2[:, 1]
    else:
        gap = np.full(B * n, np.inf)
    mx = x.max(axis=1)
    lse = mx + np.log(np.exp(x - mx[:, None]).sum(axis=1))
    scores = scores_in.numpy().astype(np.float64)[parent]
    new_scores = np.where(masked, scores, scores + x[out_rows, tok] - lse)
    tokens = np.where(masked, pad, tok).astype(np.int64)
    new_eos = np.where(masked, eos_p, eos_p | (tokens == eos))

    hist = torch.zeros((B * n, t_max), dtype=torch.int64)
    hist[:, :step] = hist_in[torch.from_numpy(parent), :step]
    hist[:, step] = torch.from_numpy(tokens)
    slots = None
    if slots_in is not None:
        slots = torch.zeros((B * n, t_max), dtype=torch.int32)
        slots[:, :step] = slots_in[torch.from_numpy(parent), :step]
        slots[:, step] = torch.arange(B * n, dtype=torch.int32)
    return dict(tokens=torch.from_numpy(tokens), scores=torch.from_numpy(new_scores), eos=torch.from_numpy(new_eos),
                hist=hist, slots=slots, parent=torch.from_numpy(parent.astype(np.int32)), eos_count=int(new_eos.sum()),
                masked=torch.from_numpy(masked), gap=torch.from_numpy(np.where(masked, np.inf, gap)),
                kept=torch.from_numpy(kept))
