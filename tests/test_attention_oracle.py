"""tests/attention_oracle.py checked on the CPU: its explicit backward against torch autograd through an independently written
fp64 softmax attention, its magnitudes, the properties the edge tests' input generator promises for every case, and the
definition of the bound (tests/test_gpu_attention_edges.py holds the kernels to it)."""
import pytest
import torch

from tests import attention_oracle as AO

H = AO.H


def _autograd_attention(q, k, v, do, B, Tq, Tk, dh, mask, keep, inv_keep):
    """O, dQ, dK, dV by autograd: per (batch, head) slices, torch.softmax, no shared code with the oracle."""
    qd, kd, vd = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    scale = AO.kernel_scale(dh)
    rows = []
    for b in range(B):
        heads = []
        for h in range(H):
            cs = slice(h * dh, (h + 1) * dh)
            s = qd[b * Tq:(b + 1) * Tq, cs] @ kd[b * Tk:(b + 1) * Tk, cs].t() * scale
            s = s + torch.where(mask[b], torch.zeros((), dtype=torch.float64), torch.full((), -10000.0, dtype=torch.float64))
            p = torch.softmax(s, dim=-1)
            if keep is not None:
                p = p * keep[b, h].double() * inv_keep
            heads.append(p @ vd[b * Tk:(b + 1) * Tk, cs])
        rows.append(torch.cat(heads, dim=1))
    o = torch.cat(rows, dim=0)
    o.backward(do.double())
    return o.detach(), qd.grad, kd.grad, vd.grad


AUTOGRAD_CASES = ["tiled-f32-dh32-17x65", "fused-bf16-dh64-100x97-kcq", "short-bf16-dh64-128x127-m3d", "long-f32-dh64-130x257-qlen_causal",
                  "short-bf16-dh64-113x17-p0.1", "fused256-bf16-dh64-193x255-kcq-p0.1", "tiled-f32-dh64-17x65-p0.5", "fused-bf16-dh64-1x1"]


@pytest.mark.parametrize("cid", AUTOGRAD_CASES)
def test_oracle_matches_autograd(cid):
    c, x = AO.BY_ID[cid], AO.make_inputs(cid)
    keep = AO.surrogate_keep(c)
    ref = AO.attention(x["q"], x["k"], x["v"], x["do"], c.B, H, c.Tq, c.Tk, c.dh, mask=x["mask"], keep=keep, inv_keep=x["inv_keep"])
    o, dq, dk, dv = _autograd_attention(x["q"], x["k"], x["v"], x["do"], c.B, c.Tq, c.Tk, c.dh, x["mask"], keep, x["inv_keep"])
    for name, want in (("O", o), ("dQ", dq), ("dK", dk), ("dV", dv)):
        got, M = ref[name], ref["M"][name]
        assert got.shape == want.shape
        err = float((got - want).abs().max())
        assert err <= 1e-12 * max(float(want.abs().max()), 1e-300), (cid, name, err)
        assert bool((M >= got.abs() * (1 - 1e-12)).all()), (cid, name, "a magnitude below the value it bounds")
    # lse and P restate the softmax: P sums to one over the keys, and is exactly zero where a row has an attendable key
    # and this one is masked
    assert float((ref["P"].sum(-1) - 1).abs().max()) < 1e-12
    live_masked = (~x["mask"] & ~x["dead"].unsqueeze(-1)).unsqueeze(1).expand_as(ref["P"])
    assert bool((ref["P"][live_masked] == 0).all())


def test_case_ids_name_their_kernels():
    fams = {c.family for c in AO.CASES}
    assert fams == {"tiled", "long", "short", "fused", "fused256", "pair"}
    for c in AO.CASES:
        if c.family in ("fused", "short"):
            assert c.bwd == "fused", c.id
        if c.family == "fused256":
            assert c.bwd == "fused256", c.id
        if c.family in ("pair", "long"):
            assert c.bwd == "pair", c.id
        if c.family == "short":   # the short forward's predicate (bf16, 64 < Tq <= 128, Tk <= 128)
            assert c.dtype == "bf16" and 64 < c.Tq <= 128 and c.Tk <= 128, c.id
        if c.family in ("tiled", "long"):
            assert c.dtype == "f32" or not (64 < c.Tq <= 128 and c.Tk <= 128), c.id


@pytest.mark.parametrize("cid", [c.id for c in AO.CASES])
def test_generator_and_bound(cid):
    """Every attendable probability >= 2^-12; at most a quarter of the query rows without an attendable key; the emulation
    within the case's bound without the margin."""
    c, x = AO.BY_ID[cid], AO.make_inputs(cid)
    do = x["do"] if x["do"] is not None else torch.zeros(c.B * c.Tq, H * c.dh)
    ref = AO.attention(x["q"], x["k"], x["v"], do, c.B, H, c.Tq, c.Tk, c.dh, mask=x["mask"])
    att = x["mask"].unsqueeze(1).expand_as(ref["P"])
    if bool(att.any()):
        assert float(ref["P"][att].min()) >= 2.0 ** -12, (cid, float(ref["P"][att].min()))
    assert float(x["dead"].double().mean()) <= 0.25, cid
    if x["do"] is not None:
        assert bool((x["do"][x["dead"].view(-1)] == 0).all())
    consts = AO.bound_constants()
    for name, r in AO.emulation_ratios(cid).items():
        assert r <= consts[(c.dtype, name)] / (AO.LSE_MARGIN if name == "lse" else AO.MARGIN[c.dtype]), (cid, name, r)


def test_bound_constants_are_of_the_expected_size():
    """The emulation's own error: at most about one u for bf16 (u = 2^-8 is a whole ulp; the stored output's rounding is half of
    one, less where the magnitudes exceed the value, plus the modelled inner roundings), a few u for a plain fp32 evaluation.
    A constant far outside that would mean the bound no longer measures rounding."""
    consts = AO.bound_constants()
    print("ATTNEDGE bound constants (margin included):", {k: round(v, 3) for k, v in sorted(consts.items())})
    for name in AO.OUTPUTS:
        assert 0.1 <= consts[("bf16", name)] / AO.MARGIN["bf16"] <= 1.5, (name, consts[("bf16", name)])
        assert 0.25 <= consts[("f32", name)] / AO.MARGIN["f32"] <= 16.0, (name, consts[("f32", name)])
