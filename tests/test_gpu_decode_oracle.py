"""The one-launch decoder step (csrc/decode_fused.hip) and the bf16 beam search against the oracle.

Both decoders run on weights that are bf16 numbers to begin with, so the fp64 oracle (oracle/reference_model.py) differs
from the product only in the precision of the activations.  The weights are sharpened the way tests/util.py's
beam_state_dict does it (matrices scaled, biases and LayerNorm parameters moved off 0 / 1): with the N(0, 0.02) initial
weights attention is near-uniform, and a wrong slot or a dropped key group would move the output less than bf16 noise.

* Step level: a whole sequence of decoding steps over consistent beam histories (every row extends a random row of its
  sentence from the step before, the slot tables are what imt_beam_step maintains), both bf16 paths (the one launch and
  the per-operator chain) against the last position of the fp64 oracle decoder run on each row's token path, and the
  k|v the step wrote into the self-attention cache against the oracle's key / value projections.  The one launch runs
  twice from a zeroed cache and must repeat itself bit for bit (it has no floating-point atomics).
* The sticky status word of the one-launch step is clean in a search that issues no step.
"""
import ctypes

import pytest
import torch

from oracle import reference_model as R
from oracle import seq_gen as OG
from tests.util import rel_err, truth_errors

pytestmark = pytest.mark.gpu
V = 1000
SCALE = 2.0   # matrices x 2: attention far from uniform, bf16 rounding still well inside HID_TOL through 12 layers

# Bounds against the fp64 truth, measured on MI355X at SCALE = 2 (worst over all cases and checked steps, one launch /
# chain): hidden states 1.25e-2 / 1.62e-2 in the max norm relative to max |truth| and 0.66 / 0.84 element-wise on the
# entries above 1 % of the maximum (relative error of the small entries); cache k|v 1.72e-2 (12 layers).  At SCALE = 3
# the 6- and 12-layer stacks amplify bf16 rounding past TOL[bf16] on both paths alike.
HID_TOL = 2e-2
HID_ELEM_TOL = 1.0
KV_TOL = 2.5e-2
REL_FLOOR = 1.5e-2   # one launch <= max(REL_FLOOR, 1.5 x chain): at 2 rows the chain can be luckier than 1e-2 / 1.5


def _models(d, ff, layers, seed, out_scale=1.0, eos_bias=0.0):
    """(oracle R.Seq2Seq, product Seq2Seq) on one set of sharpened, bf16-representable weights."""
    import imagetranslate_amd.seq2seq as S
    torch.manual_seed(seed)
    tp = R.SyntheticTextProcessor(V)
    kw = dict(lang_dec=False, enc_layer=1, dec_layer=layers, embed_dim=d, intermediate_dim=ff, num_attention_heads=d // 64)
    ref = R.Seq2Seq(tp, **kw)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for p in ref.parameters():   # (tied parameters once)
            if p.dim() > 1:
                p.mul_(SCALE)
            else:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        for ol in ref.output_layer:
            ol.layer.weight.mul_(out_scale)
            ol.layer.bias[tp.sep_token_id()] += eos_bias
        for p in ref.parameters():
            p.copy_(p.bfloat16().float())
    ours = S.Seq2Seq(tp, **kw)
    ours.load_state_dict(ref.state_dict())
    return ref.eval(), ours.cuda().eval()


def _histories(B, beam, T, g):
    """Consistent beam histories: anc[t] [rows_t, t + 1] is the row of step j that row r of step t descends from (its own
    index at j = t); step 0 has one row per sentence.  slots[t] is the slot table of step t, exactly as imt_beam_step
    leaves it (ancestors' rows for positions < t, the row itself at t)."""
    r_max = B * beam
    anc, slots = [], []
    a = torch.arange(B).view(B, 1)
    for t in range(T):
        rep = 1 if t == 0 else beam
        rows = B * rep
        if t > 0:
            prev_rep = 1 if t == 1 else beam
            parent = (torch.arange(rows) // beam) * prev_rep + torch.randint(0, prev_rep, (rows,), generator=g)
            a = torch.cat([a[parent], torch.arange(rows).view(rows, 1)], 1)
        tab = torch.zeros(r_max, T, dtype=torch.int32)
        tab[:rows, :t + 1] = a.to(torch.int32)
        anc.append(a.clone())
        slots.append(tab)
    return anc, slots


def _run_steps(monkeypatch, ours, mode, enc, mask, B, beam, T, toks, slots, keep):
    """Every step 0 .. T-1 through _Incremental in bf16 (mode "1": the one launch, "0": the chain) from a zeroed cache;
    the hidden states of the steps in `keep` and the whole self cache at the end."""
    from imagetranslate_amd import _lib as L
    from imagetranslate_amd.param_store import store_of
    from imagetranslate_amd.seq_gen import _Incremental
    monkeypatch.setenv("IMT_DECODE_FUSED", mode)
    ours.set_compute_dtype(torch.bfloat16)
    store = store_of(ours.decoder).ensure()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    r_max, d = B * beam, enc.size(-1)
    inc = _Incremental(L.load(), ours.decoder, store, torch.bfloat16, store.params_for(torch.bfloat16), enc, mask, B, beam, T, st)
    inc.cache.zero_()
    types = torch.ones(r_max, dtype=torch.long, device="cuda")
    d_toks = toks.cuda()
    d_slots = [s.cuda() for s in slots]
    out = torch.zeros(r_max, d, device="cuda", dtype=torch.bfloat16)
    outs = {}
    for t in range(T):
        rows = B * (1 if t == 0 else beam)
        inc.step(t, rows, 1 if t == 0 else beam, d_toks[t, :rows].contiguous(), types[:rows], d_slots[t], out)
        if t in keep:
            outs[t] = out[:rows].clone()
    inc.check()
    torch.cuda.synchronize()
    return outs, inc.cache.view(torch.bfloat16).view(len(ours.decoder.decoder.layer), r_max, T, 3 * d).clone()


def _truth(ref64, enc64, mask, B, beam, t, toks, anc):
    """fp64 oracle: last position of the decoder on the token path of every row of step t, and the self-attention keys /
    values of every layer along the path (forward hooks)."""
    a = anc[t]
    rows = a.size(0)
    rep = 1 if t == 0 else beam
    sent = torch.arange(rows) // rep
    ids = toks[torch.arange(t + 1)[None, :], a].cuda()                  # token of (step j, ancestor at j)
    kv = []
    hooks = []
    for layer in ref64.decoder.decoder.layer:
        sa = layer.attention.self
        box = {}
        hooks.append(sa.key.register_forward_hook(lambda m, i, o, box=box: box.__setitem__("k", o)))
        hooks.append(sa.value.register_forward_hook(lambda m, i, o, box=box: box.__setitem__("v", o)))
        kv.append(box)
    try:
        with torch.no_grad():
            h = ref64.decoder(encoder_states=enc64[sent.cuda()], input_ids=ids,
                              encoder_attention_mask=None if mask is None else mask[sent.cuda()].double(),
                              tgt_attention_mask=torch.ones(ids.shape, device="cuda", dtype=torch.float64),
                              token_type_ids=torch.ones_like(ids))
    finally:
        for hk in hooks:
            hk.remove()
    return h[:, -1], [(b["k"], b["v"]) for b in kv]


def _log_probs(ref64, h):
    lin = ref64.output_layer[1].layer
    return torch.log_softmax(h.double() @ lin.weight.detach().t() + lin.bias.detach(), -1)


# (id, d, ff, layers, B, beam, Tk, masked, T, checked steps)
STEP_CASES = [
    ("d512_L2_B8_T100", 512, 2048, 2, 8, 5, 40, True, 100, (0, 1, 2, 38, 39, 40, 41, 42, 60, 78, 79, 80, 81, 82, 99)),
    ("d512_L6_c1_T48", 512, 2048, 6, 64, 5, 128, True, 48, (0, 1, 39, 40, 41, 47)),
    ("d768_L3_caption_T64", 768, 3072, 3, 6, 5, 49, False, 64, (0, 1, 39, 40, 41, 63)),
    ("d512_ff512", 512, 512, 2, 5, 3, 33, True, 12, (0, 1, 5, 11)),
    ("d512_ff1536", 512, 1536, 2, 5, 3, 33, True, 12, (0, 1, 5, 11)),
    ("d768_ff768", 768, 768, 2, 5, 3, 33, True, 12, (0, 1, 5, 11)),
    ("d768_ff1152", 768, 1152, 2, 5, 3, 33, True, 12, (0, 1, 5, 11)),
    ("d512_L12_smallR", 512, 2048, 12, 2, 3, 17, True, 10, (0, 1, 9)),
    ("d512_beam1", 512, 2048, 2, 7, 1, 40, True, 45, (0, 1, 39, 40, 41, 44)),
    ("d512_B100_attn_loop", 512, 2048, 2, 100, 5, 24, True, 6, (0, 1, 5)),
    ("d512_B2_beam3_T150", 512, 2048, 2, 2, 3, 20, True, 150, (0, 1, 39, 40, 41, 79, 80, 81, 119, 120, 121, 144, 145, 149)),
]


@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_one_launch_step_against_the_fp64_oracle(cuda, monkeypatch, case):
    """Hidden states of every checked step, one launch and chain, within an absolute bound of the fp64 oracle on the token
    path of each row (the two bf16 paths share attn_decode_wave, so agreeing with each other proves nothing about it);
    the one launch no worse than 1.5 x the chain; the cache's k|v against the oracle's projections; the one launch
    repeats itself bit for bit."""
    name, d, ff, layers, B, beam, Tk, masked, T, checked = case
    monkeypatch.setenv("IMT_DECODE_FUSED", "1")
    ref, ours = _models(d, ff, layers, seed=len(name) + layers)
    ref64 = ref.double().cuda()
    g = torch.Generator().manual_seed(7 + B + T)
    enc = torch.randn(B, Tk, d, generator=g).bfloat16()
    mask = None
    if masked:
        mask = torch.ones(B, Tk, dtype=torch.uint8)
        for b in range(B):
            mask[b, Tk - (b % 5) * max(1, Tk // 10):] = 0
        mask[:, 0] = 1
        mask = mask.cuda()
    anc, slots = _histories(B, beam, T, g)
    toks = torch.randint(6, V, (T, B * beam), generator=g)          # own token of every (step, row)
    keep = set(c for c in checked if c < T)
    enc_d = enc.cuda().contiguous()
    fused, cache_f = _run_steps(monkeypatch, ours, "1", enc_d, mask, B, beam, T, toks, slots, keep)
    fused2, cache_f2 = _run_steps(monkeypatch, ours, "1", enc_d, mask, B, beam, T, toks, slots, keep)
    chain, cache_c = _run_steps(monkeypatch, ours, "0", enc_d, mask, B, beam, T, toks, slots, keep)
    monkeypatch.setenv("IMT_DECODE_FUSED", "1")
    assert torch.equal(cache_f, cache_f2), "the one-launch step does not repeat itself (self cache)"
    enc64 = enc.double().cuda()
    rows_err = []
    for t in sorted(keep):
        assert torch.equal(fused[t], fused2[t]), "step %d: the one-launch step does not repeat itself (hidden states)" % t
        assert torch.isfinite(fused[t].float()).all(), "step %d" % t
        h, kv = _truth(ref64, enc64, mask, B, beam, t, toks, anc)
        e_f, r_f = truth_errors(fused[t], h)
        e_c, r_c = truth_errors(chain[t], h)
        lp_err = float((_log_probs(ref64, fused[t]) - _log_probs(ref64, h)).abs().max())
        a = anc[t]
        e_kv = 0.0
        for l, (k, v) in enumerate(kv):
            for cache in (cache_f, cache_c):
                got = cache[l][a, torch.arange(t + 1)[None, :]]            # [rows, t + 1, 3d]: the row's ancestors' positions
                e_kv = max(e_kv, rel_err(got[..., d:2 * d], k), rel_err(got[..., 2 * d:], v))
        rows_err.append((t, a.size(0), e_f, r_f, e_c, r_c, e_kv, lp_err))
    worst = [max(r[i] for r in rows_err) for i in range(2, 8)]
    print("\n[fp64] %-22s fused %.2e (elem %.2e)  chain %.2e (elem %.2e)  k|v %.2e  log-prob %.2e" % ((name,) + tuple(worst)))
    for t, rows, e_f, r_f, e_c, r_c, e_kv, lp_err in rows_err:
        where = "%s step %d (%d rows, %d keys)" % (name, t, rows, t + 1)
        assert e_f <= HID_TOL and r_f <= HID_ELEM_TOL, "%s: one launch %.3e (elem %.3e) from fp64, chain %.3e (elem %.3e)" % (where, e_f, r_f, e_c, r_c)
        assert e_c <= HID_TOL and r_c <= HID_ELEM_TOL, "%s: chain %.3e (elem %.3e) from fp64" % (where, e_c, r_c)
        assert e_f <= max(REL_FLOOR, 1.5 * e_c), "%s: one launch %.3e, chain %.3e from fp64" % (where, e_f, e_c)
        assert e_kv <= KV_TOL, "%s: self-cache k|v %.3e from the fp64 projections" % (where, e_kv)


# ------------------------------------------------------------------------------------------------ the status word
def _search_args(B, Sx, seed, first=5):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(6, V, (B, Sx), generator=g)
    lens = torch.randint(Sx // 2, Sx + 1, (B,), generator=g)
    lens[0] = Sx
    mask = torch.arange(Sx)[None, :] < lens[:, None]
    src[~mask] = 0
    src[:, 0] = 5
    return dict(src_inputs=src, src_sizes=lens, first_tokens=torch.full((B,), first, dtype=torch.long), src_mask=mask,
                src_langs=torch.zeros(B, dtype=torch.long), tgt_langs=torch.ones(B, dtype=torch.long))


def _on(inp, dev):
    return {k: v.to(dev) if k != "src_sizes" else v for k, v in inp.items()}


def test_search_without_a_step_reports_no_abandoned_launch(cuda, monkeypatch):
    """A search that issues no decoding step -- beam 1 with every first token EOS, or max_len 1 -- still ends with
    imt_decode_check.  The status word lives in the workspace and used to be cleared only by a step at position 0, so it
    read whatever the caching allocator left there: poisoned first, the search must return the first tokens (what the
    oracle returns) instead of raising 'a one-launch decoder step was abandoned'."""
    from imagetranslate_amd import _lib as L
    from imagetranslate_amd.param_store import store_of
    from imagetranslate_amd.seq_gen import BeamDecoder
    monkeypatch.setenv("IMT_DECODE_FUSED", "1")
    ref, ours = _models(512, 2048, 2, seed=21)
    ours.set_compute_dtype(torch.bfloat16)
    B, Sx = 16, 12
    desc, _keep = ours.decoder._desc(store_of(ours.decoder).ensure(), torch.bfloat16)
    lib = L.load()
    for beam, first, max_len in ((1, 4, None), (5, 5, 1), (1, 5, 1)):
        inp = _search_args(B, Sx, seed=beam, first=first)
        ws_bytes = lib.imt_decode_workspace_bytes(ctypes.byref(desc), B * beam)
        assert ws_bytes > 0
        poison = [torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(8)]
        torch.cuda.synchronize()
        del poison   # back to the caching allocator, 0xFF inside
        for unpad in (True, False):
            got = BeamDecoder(ours, beam_width=beam)(pad_idx=0, max_len=max_len, unpad_output=unpad, **_on(inp, "cuda"))
            exp = OG.BeamDecoder(ref, beam_width=beam)(pad_idx=0, max_len=max_len, unpad_output=unpad, **inp)
            assert [x.tolist() for x in got] == [e.tolist() for e in exp], (beam, first, max_len, unpad)
            if not unpad:
                assert all(x.tolist() == [first] for x in got)


def test_decode_check_reports_a_set_status_word(cuda, monkeypatch):
    """imt_decode_check raises when the status word is set (here: the whole workspace filled with 0xFF, no step
    launched), and a freshly built _Incremental reads clean."""
    from imagetranslate_amd import _lib as L
    from imagetranslate_amd.param_store import store_of
    from imagetranslate_amd.seq_gen import _Incremental
    monkeypatch.setenv("IMT_DECODE_FUSED", "1")
    _, ours = _models(512, 1024, 2, seed=22)
    ours.set_compute_dtype(torch.bfloat16)
    store = store_of(ours.decoder).ensure()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    enc = torch.randn(3, 9, 512, device="cuda").bfloat16()
    inc = _Incremental(L.load(), ours.decoder, store, torch.bfloat16, store.params_for(torch.bfloat16), enc, None, 3, 4, 5, st)
    inc.check()
    inc.ws.fill_(0xFF)
    with pytest.raises(L.ImtError, match="abandoned"):
        inc.check()

