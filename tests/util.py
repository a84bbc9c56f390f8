import os

import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHARD_BYTES = 900 * 1024  # tensor bytes per shard of a sharded fixture (every committed file stays under 1 MiB)


def save_sharded(obj: dict, out_dir: str, shard_bytes: int = SHARD_BYTES):
    """torch.save of a nested dict as out_dir/NN.pt shards of at most `shard_bytes` tensor bytes each (a single larger
    tensor gets a shard of its own); load_sharded puts it back together."""
    items = []

    def walk(d, path):
        for k, v in d.items():
            if isinstance(v, dict):
                walk(v, path + (k,))
            else:
                items.append((path + (k,), v.clone() if torch.is_tensor(v) else v))
    walk(obj, ())
    shards, cur, size = [], [], 0
    for path, v in items:
        n = v.numel() * v.element_size() if torch.is_tensor(v) else 0
        if cur and size + n > shard_bytes:
            shards.append(cur)
            cur, size = [], 0
        cur.append((path, v))
        size += n
    shards.append(cur)
    os.makedirs(out_dir, exist_ok=True)
    for i, sh in enumerate(shards):
        torch.save({"paths": [list(p) for p, _ in sh], "values": [v for _, v in sh]}, os.path.join(out_dir, "%02d.pt" % i))


def load_sharded(out_dir: str) -> dict:
    obj = {}
    for f in sorted(os.listdir(out_dir)):
        if not f.endswith(".pt"):
            continue
        sh = torch.load(os.path.join(out_dir, f), weights_only=True)
        for path, v in zip(sh["paths"], sh["values"]):
            d = obj
            for k in path[:-1]:
                d = d.setdefault(k, {})
            d[path[-1]] = v
    return obj


def load_toy():
    """The whole-model fixture of the toy configuration (tests/golden/make_golden.py make_toy), stored in shards."""
    return load_sharded(os.path.join(GOLD, "toy_seq2seq"))


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """max |a-b| / max |b| (b = reference), computed in fp64 on CPU."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    denom = max(float(b.abs().max()), 1e-30)
    return float((a - b).abs().max()) / denom


def assert_close(a, b, tol, what=""):
    assert a.shape == b.shape, "%s shape %s vs %s" % (what, tuple(a.shape), tuple(b.shape))
    assert torch.isfinite(a.detach().float()).all(), "%s has non-finite values" % what
    e = rel_err(a, b)
    assert e <= tol, "%s: rel err %.3e > tol %.1e" % (what, e, tol)
    return e


def truth_errors(a: torch.Tensor, truth: torch.Tensor):
    """(max |a-t| / max |t|,  max over entries with |t| >= 1 % of max |t| of |a-t| / |t|) against an fp64 ground truth."""
    a = a.detach().double().cpu()
    t = truth.detach().double().cpu()
    assert a.shape == t.shape, (tuple(a.shape), tuple(t.shape))
    m = float(t.abs().max())
    if m == 0.0:
        return float(a.abs().max()), 0.0
    d = (a - t).abs()
    big = t.abs() >= 1e-2 * m
    return float(d.max()) / m, float((d[big] / t.abs()[big]).max())


def fp64_truth_report(name, ours, oracle32, truth, tol, elem_tol, log=None):
    """north_star's bar, measured against an fp64 run of the oracle: the HIP fp32 result within ``tol`` of the truth in the
    max norm and within ``elem_tol`` element-wise on the entries above 1 % of the maximum; the fp32 oracle's own distance
    from the truth is printed beside it (and written to ``log``), so that a bar is evidenced, not asserted."""
    e_o, r_o = truth_errors(ours, truth)
    e_f, r_f = truth_errors(oracle32, truth)
    line = "%-62s hip-fp32 %.2e (elem %.2e) | oracle-fp32 %.2e (elem %.2e)" % (name, e_o, r_o, e_f, r_f)
    print(line)
    if log is not None:
        log.append(line)
    assert torch.isfinite(ours.detach().float()).all(), name
    assert e_o <= tol, "%s: %.3e > %.1e against the fp64 truth (fp32 oracle: %.3e)" % (name, e_o, tol, e_f)
    assert r_o <= elem_tol, "%s: element-wise %.3e > %.1e against the fp64 truth (fp32 oracle: %.3e)" % (name, r_o, elem_tol, r_f)
    return e_o, e_f


TOL = {torch.float32: 1e-4, torch.bfloat16: 2.5e-2}


# ------------------------------------------------------------------------------------------- beam-search fixtures
def beam_state_dict(sd, scale: float = 4.0, eos_bias: float = 5.0, eos: int = 4):
    """Toy weights for beam search: the N(0, 0.02) fixture weights give near-uniform next-token distributions, so
    matrices are scaled up and the EOS logit biased -- hypotheses then finish at different steps and the EOS /
    length-limit / PAD bookkeeping of src/seq_gen.py:193-227 is exercised."""
    out = {}
    for k, v in sd.items():
        v = v.clone()
        if v.dim() > 1 and v.is_floating_point():
            v = v * scale
        if k.startswith("output_layer") and k.endswith("layer.bias"):
            v[eos] = eos_bias
        out[k] = v
    return out


def beam_inputs():
    B, S = 6, 12
    g = torch.Generator().manual_seed(1)
    src = torch.randint(6, 1000, (B, S), generator=g)
    lens = torch.tensor([12, 10, 8, 12, 5, 7])
    mask = torch.arange(S)[None, :] < lens[:, None]
    src[~mask] = 0
    src[:, 0] = 5
    for b in range(B):
        src[b, lens[b] - 1] = 4
    return dict(src_inputs=src, src_sizes=lens, first_tokens=torch.full((B,), 5, dtype=torch.long), src_mask=mask,
                src_langs=torch.zeros(B, dtype=torch.long), tgt_langs=torch.ones(B, dtype=torch.long))


def caption_beam_inputs():
    B = 5
    g = torch.Generator().manual_seed(3)
    return dict(images=torch.randn(B, 49, 64, generator=g), first_tokens=torch.full((B,), 5, dtype=torch.long),
                tgt_langs=torch.ones(B, dtype=torch.long))


# ------------------------------------------------------------------------------------------- imt_beam_step helpers
def ref_beam_step(logits, scores, sizes, eos_in, max_lens, hist, step, B, beam, rep, V, ratio, pad, eos, dtype=None,
                  return_sorted=False):
    """The reference's step (src/seq_gen.py:193-227) on CPU tensors with the oracle's stable top-k (value descending, flat
    index ascending).  ``dtype=torch.float64`` does every score computation (log_softmax, the zeroing, scores + lp, the
    division by pow((sizes + 6) / 6, ratio)) in double precision; ``return_sorted`` adds the sentences' candidate scores in
    selection order ([B, rep * V]) for beam_reference_is_unambiguous."""
    sizes_in = sizes
    if dtype is not None:
        logits, scores, sizes = logits.to(dtype), scores.to(dtype), sizes.to(dtype)
    lp = torch.log_softmax(logits, -1)
    over = (max_lens < step + 1)
    lp[eos_in.bool()] = 0
    if step > 1:
        lp[over.repeat_interleave(rep)] = 0
    total = scores.unsqueeze(-1) + lp
    if beam > 1:
        total = total / torch.pow((sizes + 6.0) / 6.0, ratio).unsqueeze(-1)
    vals, order = torch.sort(total.view(B, -1), dim=1, descending=True, stable=True)
    top, idx = vals[:, :beam].contiguous(), order[:, :beam].contiguous()
    if step > 1:
        idx[over] = pad
        flat = idx.view(-1)
        flat[eos_in.bool()] = pad
        parent = idx // V
    else:
        parent = torch.zeros_like(idx)
    word = idx % V
    prow = (torch.arange(B)[:, None] * rep + parent).view(-1)
    new_hist = torch.cat([hist[prow, :step], word.view(-1, 1)], 1)
    new_sizes = sizes_in[prow] + (word.view(-1) != pad)
    new_eos = (new_hist == eos).any(1)
    out = (top.view(-1), new_sizes, new_eos, new_hist, prow)
    return out + (vals,) if return_sorted else out


def beam_reference_is_unambiguous(vals, beam, gap=1e-4):
    """The condition on the INPUTS under which an fp32 kernel can be compared token for token with the fp64 reference:
    among each sentence's best beam + 1 candidates (``vals``: [B, n] fp64, selection order) every adjacent pair is either
    bit-equal -- a constructed tie, decided by the index alone -- or at least ``gap`` apart.  A run of ties that reaches
    past the best beam + 1 is followed to its end and the step below it checked too (nothing within rounding of the
    selected candidates but outside them).  Returns (ok, smallest non-zero gap seen)."""
    ok, smallest = True, float("inf")
    for row in vals:
        n = min(beam + 1, row.numel())
        n = int((row >= row[n - 1]).sum())          # through the end of the tie run of the last one (row is sorted)
        d = row[:min(n + 1, row.numel())]
        d = d[:-1] - d[1:]
        d = d[d != 0]
        if d.numel():
            smallest = min(smallest, float(d.min()))
            ok = ok and bool((d >= gap).all())
    return ok, smallest


def bind_search_step(a, logits, scores, eos_in, max_lens, hist, slots_in, step, B, width, rep, V, t_max, pad, eos,
                     ld=None, offset=0, pad_fill=0.0, out_fill=0):
    """What imt_beam_args and imt_sample_args share (every field but the hypotheses per sentence -- ``width`` -- bears the same
    name in both), set in ``a`` from copies of the given CPU tensors.  The logits rows are laid out ``ld`` (default V) floats
    apart in a device buffer, starting ``offset`` floats into it (the buffer itself is 16-byte aligned); the columns [V, ld) of
    every row hold ``pad_fill``.  The history and slot outputs start out as ``out_fill``, every other output as zero.  Returns
    (the output buffers by name, the device inputs: keep them until the step has run)."""
    dev = "cuda"
    rows, r_out = B * rep, B * width
    ld = V if ld is None else ld
    assert ld >= V and logits.shape == (rows, V)
    z = lambda *s, dtype: torch.zeros(*s, dtype=dtype, device=dev)
    buf = torch.full((offset + rows * ld,), pad_fill, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    d_logits = buf[offset:].view(rows, ld)
    d_logits[:, :V] = logits.cuda()
    ins = dict(scores_in=scores.cuda(), eos_in=eos_in.to(torch.uint8).cuda(), max_lens=max_lens.cuda(), hist_in=hist.cuda(),
               slots_in=slots_in.cuda())
    outs = dict(scores=z(r_out, dtype=torch.float32), eos=z(r_out, dtype=torch.uint8),
                hist=torch.full((r_out, t_max), out_fill, dtype=torch.int64, device=dev),
                slots=torch.full((r_out, t_max), out_fill, dtype=torch.int32, device=dev),
                parent=z(r_out, dtype=torch.int32), tokens=z(r_out, dtype=torch.int64), eos_count=z(t_max, dtype=torch.int32))
    a.B, a.rep, a.V, a.step, a.t_max = B, rep, V, step, t_max
    a.logits, a.ld, a.pad_idx, a.eos = d_logits.data_ptr(), ld, pad, eos
    for name, t in ins.items():
        setattr(a, name, t.data_ptr())
    for name, t in outs.items():
        setattr(a, name if name == "eos_count" else name + "_out", t.data_ptr())
    return outs, (buf, ins)


def call_beam_step(logits, scores, sizes, eos_in, max_lens, hist, slots_in, step, B, beam, rep, V, t_max, ratio, pad, eos,
                   **layout):
    """One imt_beam_step through the C ABI on copies of the given CPU tensors; returns the output buffers.  ``layout``: the
    ``ld`` / ``offset`` / ``pad_fill`` / ``out_fill`` of bind_search_step."""
    import imagetranslate_amd.hip_ops as O
    from imagetranslate_amd import _lib as L
    a = L.BeamArgs()
    outs, keep = bind_search_step(a, logits, scores, eos_in, max_lens, hist, slots_in, step, B, beam, rep, V, t_max, pad, eos,
                                  **layout)
    d_sizes = sizes.cuda()
    outs["sizes"] = torch.zeros(B * beam, dtype=torch.float32, device="cuda")
    outs["cand_scores"] = torch.zeros(B * rep, beam, dtype=torch.float32, device="cuda")
    outs["cand_idx"] = torch.zeros(B * rep, beam, dtype=torch.int32, device="cuda")
    a.beam, a.len_penalty_ratio = beam, ratio
    a.sizes_in, a.sizes_out = d_sizes.data_ptr(), outs["sizes"].data_ptr()
    a.cand_scores, a.cand_idx = outs["cand_scores"].data_ptr(), outs["cand_idx"].data_ptr()
    O.beam_step(a)
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in outs.items()}


def call_sample_step(logits, scores, eos_in, max_lens, hist, slots_in, step, B, n, rep, V, t_max, temperature, topk, seed,
                     pad=0, eos=4, **layout):
    """One imt_sample_step through the C ABI, as call_beam_step."""
    import imagetranslate_amd.hip_ops as O
    from imagetranslate_amd import _lib as L
    a = L.SampleArgs()
    outs, keep = bind_search_step(a, logits, scores, eos_in, max_lens, hist, slots_in, step, B, n, rep, V, t_max, pad, eos, **layout)
    a.n, a.temperature, a.topk, a.seed = n, temperature, topk, seed
    O.sample_step(a)
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in outs.items()}
