"""csrc/attention.hip at the shapes where its loops take another trip, its tiles end and its plan changes kernel, against the
fp64 restatement of tests/attention_oracle.py (tests/test_gpu_ops.py stops at 256 x 256, compares by max|a-b| / max|b| and
never looks at lse).  Per case (tests/attention_oracle.py, CASES; the id names the kernel the case is there for):

  * every element of O, dQ, dK, dV outside fully-masked query rows satisfies |got - ref| <= c * u * (M + |ref|), M the sum of
    the magnitudes of the element's terms, c from the emulation's own error (attention_oracle.bound_constants); lse likewise
    on attendable rows, with a floor of 4 ulp;
  * every output is a view into a wider buffer whose guard rows and pad columns hold a NaN bit pattern that must come back
    bit-unchanged; the packed cases read q | k | v from one [N, 3d] buffer and write dQ | dK | dV into the slices of another;
  * the backward reaches the kernel the id names (profiler kinds, as tests/test_gpu_attn_dispatch.py reads them);
  * a second launch returns the same bits;
  * under dropout the keep mask is RECOVERED from the forward (V = one-hot columns, ceil(Tk / dh) launches), never restated
    from the generator: the kept values must be P / (1 - p), lse must not change, and every backward kernel is held to the
    oracle under that mask -- which it meets only if it regenerates the mask the forward applied.

Each case prints ``ATTNEDGE <id> <kinds> <output>=<worst error / bound> ...`` before it asserts (pytest -s shows the figures;
DESIGN.md, "Attention edge tests", records them)."""
import contextlib
import math
import os

import pytest
import torch

from tests import attention_oracle as AO

pytestmark = pytest.mark.gpu

H = AO.H
SWITCHES = ("IMT_ATTN_NO_SHORT_FWD", "IMT_ATTN_NO_FUSED_BWD", "IMT_ATTN_NO_FUSED256")
NAN_BITS = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA5A5A5)}
KINDS = {"pair": lambda dt: {"attn_bwd_dq_" + dt, "attn_bwd_dkdv_" + dt}, "fused": lambda dt: {"attn_bwd_fused_bf16"},
         "fused256": lambda dt: {"attn_bwd_fused256_bf16"}}


def _ops():
    from imagetranslate_amd import hip_ops as O
    return O


@contextlib.contextmanager
def _env(names):
    for s in SWITCHES:
        os.environ.pop(s, None)
    for s in names:
        os.environ[s] = "1"
    try:
        yield
    finally:
        for s in SWITCHES:
            os.environ.pop(s, None)


def _rows_of(fn):
    """imt_prof_report rows of the launches of fn(), as {kind: launches}."""
    from imagetranslate_amd import _lib as L
    lib = L.load()
    torch.cuda.synchronize()
    lib.imt_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        rows = (L.ProfRow * 64)()
        n = lib.imt_prof_report(rows, 64)
    finally:
        lib.imt_prof_enable(0)
    return {rows[i].kind.decode(): int(rows[i].launches) for i in range(n)}


class Guard:
    """Column slices ``views`` ([rows, w] each, side by side) of a [2 + rows + 2, sum(w) + pad] buffer (pad: 8 columns, fp32 4)
    filled with a NaN bit pattern; ``check`` asserts that everything outside the slices still holds it, bit for bit."""

    def __init__(self, rows, widths, dtype, dev):
        self.rows, self.width = rows, sum(widths)
        itype, self.pattern = NAN_BITS[dtype]
        self.full = torch.empty(rows + 4, self.width + (8 if dtype == torch.bfloat16 else 4), dtype=dtype, device=dev)
        self.bits = self.full.view(itype)
        self.bits.fill_(self.pattern)
        offs = [sum(widths[:n]) for n in range(len(widths))]
        self.views = [self.full[2:2 + rows, o:o + w] for o, w in zip(offs, widths)]

    def check(self, what):
        b = self.bits.cpu().clone()
        assert bool((b[:2] == self.pattern).all()), "%s: wrote in front of the first row" % what
        assert bool((b[2 + self.rows:] == self.pattern).all()), "%s: wrote past the last row" % what
        assert bool((b[:, self.width:] == self.pattern).all()), "%s: wrote into the pad columns" % what


class GuardLse:
    """Contiguous fp32 [B, H, Tq] in the middle of a flat buffer with 8 guard elements on either side."""

    def __init__(self, B, Tq, dev):
        self.n = B * H * Tq
        self.full = torch.empty(self.n + 16, dtype=torch.float32, device=dev)
        self.bits = self.full.view(torch.int32)
        self.bits.fill_(NAN_BITS[torch.float32][1])
        self.view = self.full[8:8 + self.n].view(B, H, Tq)

    def check(self, what):
        b = self.bits.cpu()
        assert bool((b[:8] == NAN_BITS[torch.float32][1]).all()) and bool((b[8 + self.n:] == NAN_BITS[torch.float32][1]).all()), \
            "%s: wrote outside lse" % what


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _dev(t, dev):
    return None if t is None else t.to(dev)


def _recover(O, dtype, dh, B, Tq, Tk, q, k, kw):
    """Pd [B, H, Tq, Tk] (fp32, CPU) as the forward the plan picks produces it: V = one-hot columns, dh keys per launch."""
    d = H * dh
    vals = torch.zeros(B, H, Tq, Tk)
    for l in range((Tk + dh - 1) // dh):
        n = min(dh, Tk - l * dh)
        v = torch.zeros(B, Tk, H, dh)
        idx = torch.arange(n)
        v[:, l * dh + idx, :, idx] = 1.0
        out = O.attention_fwd(q, k, v.view(B * Tk, d).to(dtype).to(q.device), B, H, Tq, Tk, dh, **kw)[0]
        vals[:, :, :, l * dh:l * dh + n] = out.float().cpu().view(B, Tq, H, dh).permute(0, 2, 1, 3)[..., :n]
    return vals


def _measure(cid, name, got, ref, M, c, u, where, figures):
    assert bool(torch.isfinite(got.float()).all()), "%s %s has non-finite values" % (cid, name)
    r = AO.ratio(got, ref, M, u, where) / c
    figures.append("%s=%.3f" % (name, r))
    return r


def _lse_ratio(got, ref, M, c, where):
    got, ref = got.detach().double().cpu(), ref.double()
    bound = torch.maximum(c * AO.U["f32"] * (M.double() + ref.abs()), AO.lse_floor(ref))
    return float(((got - ref).abs() / bound)[where].max()) if bool(where.any()) else 0.0


@pytest.mark.parametrize("cid", [c.id for c in AO.CASES])
def test_attention_edges(cuda, cid):
    O = _ops()
    c, x, consts = AO.BY_ID[cid], AO.make_inputs(cid), AO.bound_constants()
    dt, u, dh, B, Tq, Tk = AO.TORCH_DTYPE[c.dtype], AO.U[c.dtype], c.dh, c.B, c.Tq, c.Tk
    d, Nq, Nk = H * dh, c.B * c.Tq, c.B * c.Tk
    if c.packed:   # self-attention: q | k | v are the column slices of one buffer
        qkv = torch.cat([x["q"], x["k"], x["v"]], dim=1).to(cuda)
        q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    else:
        q, k, v = x["q"].to(cuda), x["k"].to(cuda), x["v"].to(cuda)
    masks = dict(key_mask=_dev(x["key_mask"], cuda), query_mask=_dev(x["query_mask"], cuda), causal=x["causal"])
    kw = dict(masks, dropout_p=c.p, dropout_seed=c.seed)
    kw3 = dict(kw, mask3d=_dev(x["mask3d"], cuda))
    dims = (B, H, Tq, Tk, dh)
    figures, worst = [], {}
    live_rows = ~x["dead"]
    att = (x["mask"] & live_rows.unsqueeze(-1)).unsqueeze(1).expand(B, H, Tq, Tk)

    # ---- forward: the kernel the plan picks, and for the short forward's shapes the tiled one on the same input
    fwd_variants = [c.env] + ([c.env + (AO.NO_SHORT,)] if c.family == "short" else [])
    keep = ref = o_first = lse_first = None
    for env in fwd_variants:
        tag = "fwd[tiled]" if AO.NO_SHORT in env else "fwd"
        with _env(env):
            if c.p > 0:
                vals = _recover(O, dt, dh, B, Tq, Tk, q, k, kw3)
                this_keep = (vals != 0)
                if keep is not None:
                    assert torch.equal(this_keep, keep), "%s: the short and the tiled forward drop different elements" % cid
                keep = this_keep
            og, lg = Guard(Nq, [d], dt, cuda), GuardLse(B, Tq, cuda)
            O.attention_fwd(q, k, v, *dims, **kw3, o=og.views[0], lse=lg.view)
            og2, lg2 = Guard(Nq, [d], dt, cuda), GuardLse(B, Tq, cuda)
            O.attention_fwd(q, k, v, *dims, **kw3, o=og2.views[0], lse=lg2.view)
            if c.p > 0:
                lse_nodrop = O.attention_fwd(q, k, v, *dims, **dict(kw3, dropout_p=0.0))[1]
        og.check(cid + " O"), lg.check(cid + " lse")
        assert _bits_equal(og.views[0], og2.views[0]) and _bits_equal(lg.view, lg2.view), "%s %s: a second launch differs" % (cid, tag)
        if c.p > 0:
            assert _bits_equal(lse_nodrop, lg.view), "%s %s: lse changes under dropout" % (cid, tag)
        if ref is None:
            do_cpu = x["do"] if x["do"] is not None else torch.zeros(Nq, d)
            ref = AO.attention(x["q"], x["k"], x["v"], do_cpu, *dims, mask=x["mask"], keep=None if keep is None else keep.double(),
                               inv_keep=x["inv_keep"])
        o_got, lse_got = og.views[0], lg.view
        worst[tag + " O"] = _measure(cid, tag + ".O", o_got, ref["O"], ref["M"]["O"], consts[(c.dtype, "O")], u,
                                           AO.compared("O", B, H, Tq, Tq, dh, x["dead"]), figures)
        assert bool(torch.isfinite(lse_got).all()), cid
        r = _lse_ratio(lse_got, ref["lse"], ref["M"]["lse"], consts[(c.dtype, "lse")], AO.compared("lse", B, H, Tq, Tq, dh, x["dead"]))
        figures.append("%s.lse=%.3f" % (tag, r))
        worst[tag + " lse"] = r
        if c.p > 0:   # the kept values are P / (1 - p); dropped and masked ones exactly zero
            pd = ref["P"] * keep.double() * x["inv_keep"]
            rows = live_rows.view(B, 1, Tq, 1).expand_as(pd)
            worst[tag + " Pd"] = _measure(cid, tag + ".Pd", vals, pd, pd, consts[(c.dtype, "O")], u, rows, figures)
            assert bool(keep[att].any()) and not bool(keep[att].all()), "%s: dropout kept or dropped everything" % cid
        if o_first is None:
            o_first, lse_first = o_got, lse_got

    # ---- backward, from the o / lse the planned forward stored
    with _env(c.env):
        if c.proj:
            dy, w_o = x["dy"].to(cuda), x["w_o"].to(cuda)
            do_buf = torch.zeros(Nq, d, dtype=dt, device=cuda)
            got = {}

            def run():
                got["dQ"], got["dK"], got["dV"] = O.attention_bwd_proj(dy, w_o, q, k, v, o_first, lse_first, *dims, **kw, do_out=do_buf)
            kinds = _rows_of(run)
            again = O.attention_bwd_proj(dy, w_o, q, k, v, o_first, lse_first, *dims, **kw)
            # dO = dy W_o: fp32 sums of d products (error <= d 2^-24 of their magnitudes) rounded once to bf16 (half an ulp: at
            # most 2^-8 of the value, at the bottom of a binade)
            do_ref = x["dy"].double() @ x["w_o"].double()
            do_mag = x["dy"].double().abs() @ x["w_o"].double().abs()
            do_err = (do_buf.double().cpu() - do_ref).abs()
            assert bool((do_err <= 2.0 ** -8 * 1.001 * do_ref.abs() + d * 2.0 ** -24 * do_mag).all()), "%s: dO = dy W_o" % cid
            do_cpu = do_buf.cpu()
            guards = []
        else:
            do_cpu = x["do"]
            do_d = do_cpu.to(cuda)

            def alloc():
                if c.packed:
                    g = Guard(Nq, [d, d, d], dt, cuda)
                    return [g], g.views
                gs = [Guard(Nq, [d], dt, cuda), Guard(Nk, [d], dt, cuda), Guard(Nk, [d], dt, cuda)]
                return gs, [g.views[0] for g in gs]
            guards, (dq, dk, dv) = alloc()
            kinds = _rows_of(lambda: O.attention_bwd(do_d, q, k, v, o_first, lse_first, *dims, **kw3, dq=dq, dk=dk, dv=dv))
            got = {"dQ": dq, "dK": dk, "dV": dv}
            _, again = alloc()
            O.attention_bwd(do_d, q, k, v, o_first, lse_first, *dims, **kw3, dq=again[0], dk=again[1], dv=again[2])
    for g in guards:
        g.check(cid + " dQ | dK | dV")
    want_kinds = KINDS[c.bwd](c.dtype)
    assert set(kinds) == want_kinds and all(n == 1 for n in kinds.values()), (cid, kinds, want_kinds)
    for name, a in zip(("dQ", "dK", "dV"), again):
        assert _bits_equal(got[name], a), "%s %s: a second launch differs" % (cid, name)
    if c.proj:   # the oracle under the dO the kernel formed
        ref = AO.attention(x["q"], x["k"], x["v"], do_cpu, *dims, mask=x["mask"], keep=None if keep is None else keep.double(),
                           inv_keep=x["inv_keep"])
    for name in ("dQ", "dK", "dV"):
        worst[name] = _measure(cid, name, got[name], ref[name], ref["M"][name], consts[(c.dtype, name)], u,
                                     AO.compared(name, B, H, Tq, Tk, dh, x["dead"]), figures)
    print("ATTNEDGE %s %s %s" % (cid, "+".join(sorted(kinds)), " ".join(figures)))
    bad = {n: r for n, r in worst.items() if not r <= 1.0}
    assert not bad, "%s: worst error / bound above 1: %s" % (cid, bad)


# ------------------------------------------------------------------------------------------------ the dropout mask itself
MASK_SHAPES = [(113, 17), (128, 127), (193, 255), (257, 257)]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("Tq,Tk", MASK_SHAPES, ids=["%dx%d" % s for s in MASK_SHAPES])
def test_dropout_mask_identity_and_statistics(cuda, Tq, Tk, p):
    """The mask is a function of (b, h, i, j), Tq, Tk, the rate and the seed alone: the short and the tiled forward, bf16 and
    fp32, head_dim 32 and 64 drop the same elements.  Its statistics: kept fraction, joint rate of the two keys that share a
    draw, rows and (batch, head) slices that differ, another seed."""
    O = _ops()
    B = 2
    seed = AO.BIG_SEED + Tq if Tq % 2 else 1000 + Tq
    g = torch.Generator().manual_seed(Tq * 1000 + Tk)
    qk = {dh: ((torch.randn(B * Tq, H * dh, generator=g) * 0.5).bfloat16(), (torch.randn(B * Tk, H * dh, generator=g) * 0.5).bfloat16())
          for dh in (64, 32)}

    def recover(dtype, dh, env, seed=seed):
        with _env(env):
            return _recover(O, dtype, dh, B, Tq, Tk, qk[dh][0].to(dtype).to(cuda), qk[dh][1].to(dtype).to(cuda),
                            dict(dropout_p=p, dropout_seed=seed)) != 0
    keep = recover(torch.bfloat16, 64, ())
    variants = [("f32 dh64", torch.float32, 64, ()), ("bf16 dh32", torch.bfloat16, 32, ()), ("f32 dh32", torch.float32, 32, ())]
    if 64 < Tq <= 128 and Tk <= 128:
        variants += [("bf16 dh64 tiled", torch.bfloat16, 64, (AO.NO_SHORT,)), ("bf16 dh32 tiled", torch.bfloat16, 32, (AO.NO_SHORT,))]
    for name, dtype, dh, env in variants:
        assert torch.equal(recover(dtype, dh, env), keep), "%dx%d p=%g: %s drops other elements than bf16 dh64" % (Tq, Tk, p, name)

    q_keep = 1.0 - round(p * 65536) / 65536.0
    n = keep.numel()
    frac = float(keep.double().mean())
    a, b = keep[..., 0:Tk - 1:2], keep[..., 1:Tk:2]
    joint, q2 = float((a & b).double().mean()), q_keep * q_keep
    print("ATTNEDGE dropout %dx%d p=%g kept %.5f (want %.5f +- %.5f) pairs %.5f (want %.5f +- %.5f)"
          % (Tq, Tk, p, frac, q_keep, 4 * math.sqrt(p * (1 - p) / n), joint, q2, 4 * math.sqrt(q2 * (1 - q2) / a.numel())))
    assert abs(frac - q_keep) <= 4 * math.sqrt(p * (1 - p) / n)
    assert abs(joint - q2) <= 4 * math.sqrt(q2 * (1 - q2) / a.numel())
    rows = keep.view(-1, Tk)
    distinct = torch.unique(rows, dim=0).shape[0]
    assert distinct > 1, "every (b, h, i) row shares one mask"
    if Tk >= 127:   # (0.82^127 x rows^2: no two rows can coincide by chance)
        assert distinct == rows.shape[0], "%d of %d rows distinct" % (distinct, rows.shape[0])
    slices = keep.view(B * H, -1)
    assert torch.unique(slices, dim=0).shape[0] == B * H, "two (batch, head) slices share a mask"
    assert not torch.equal(recover(torch.bfloat16, 64, (), seed=seed + 1), keep), "another seed, the same mask"
