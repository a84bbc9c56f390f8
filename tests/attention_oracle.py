"""Checker for csrc/attention.hip: multi-head attention forward and backward restated in plain fp64 torch on the CPU, with no
project kernel behind it, plus the shapes and inputs of the attention edge tests (tests/test_gpu_attention_edges.py on the
GPU, tests/test_attention_oracle.py on the CPU).

    S = Q K^T * scale + (1 - mask) * -10000      lse = logsumexp(S)      P = exp(S - lse)
    Pd = P * keep / (1 - p)                       O = Pd V
    dV = Pd^T dO      dP = (dO V^T) * keep / (1 - p)      delta = rowsum(dO * O)      dS = P * (dP - delta)
    dQ = scale * dS K                             dK = scale * dS^T Q

``mask`` is the AND of key mask, query mask, causal (j <= i, also when Tq != Tk) and the 3-D mask; ``keep`` a given
[B, H, Tq, Tk] 0/1 tensor (the tests recover it from the forward kernel; nothing here restates the generator).

As tests/rowops_oracle.py does, every output comes with ``M``: the same expression evaluated on absolute values, the sum of
the magnitudes of the terms an element is made of.  An element-wise bound ``|got - ref| <= c * u * (M + |ref|)`` stays
meaningful where the terms cancel and on small entries next to large ones, which a bound relative to the tensor's maximum
does not.

``emulate`` is the same computation in fp32 torch with roundings to the kernels' storage type at the points where the kernels
round; the constant ``c`` of the bound is the worst ratio of ``emulate`` against the fp64 values over all cases, times a
margin (``bound_constants``)."""
import collections
import functools
import math
import zlib

import torch

MASKED = -10000.0
U = {"bf16": 2.0 ** -8, "f32": 2.0 ** -24}
TORCH_DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}
# what the kernels add to the emulation's error: bf16 -- the emulation already holds the bf16 roundings, fp32 accumulation order
# and the hardware exp remain; fp32 -- the hardware exp's argument scaling, MFMA summation order and the online rescale (the
# margin tests/test_gpu_row_edges.py uses over a plain fp32 evaluation).  lse is fp32 arithmetic on exact products for either
# input type (no bf16 rounding enters it), so it gets the fp32 margin for both.
MARGIN = {"bf16": 4.0, "f32": 16.0}
LSE_MARGIN = 16.0
OUTPUTS = ("O", "dQ", "dK", "dV")


# ------------------------------------------------------------------------------------------------ the operation
def split_heads(x, B, T, H, dh):
    """[B*T, >= H*dh] (heads merged, as the kernels take it) -> [B, H, T, dh]."""
    return x[:, :H * dh].reshape(B, T, H, dh).permute(0, 2, 1, 3)


def merge_heads(x):
    B, H, T, dh = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, H * dh)


def attend_mask(B, Tq, Tk, key_mask=None, query_mask=None, mask3d=None, causal=False):
    """bool [B, Tq, Tk]: True where query i may attend key j."""
    m = torch.ones(B, Tq, Tk, dtype=torch.bool)
    if key_mask is not None:
        m &= key_mask.cpu().bool().view(B, 1, Tk)
    if query_mask is not None:
        m &= query_mask.cpu().bool().view(B, Tq, 1)
    if causal:
        m &= torch.arange(Tk).view(1, 1, Tk) <= torch.arange(Tq).view(1, Tq, 1)
    if mask3d is not None:
        m &= mask3d.cpu().bool().view(B, Tq, Tk)
    return m


def kernel_scale(dh):
    """1 / sqrt(head_dim) as the fp32 value the kernels multiply by."""
    return float(torch.tensor(1.0 / math.sqrt(dh), dtype=torch.float32))


def kernel_inv_keep(p):
    """The keep scale 1 / (1 - p) as csrc/attention.hip forms it (p and the quotient in fp32)."""
    if p <= 0:
        return 1.0
    p32 = torch.tensor(p, dtype=torch.float32)
    return float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - p32))


def _compute(q, k, v, do, B, H, Tq, Tk, dh, mask, keep, inv_keep, scale, work, rnd, magnitudes):
    Q, K, V, dO = (split_heads(t.detach().cpu().to(work), B, T, H, dh) for t, T in ((q, Tq), (k, Tk), (v, Tk), (do, Tq)))
    add = torch.zeros(B, 1, Tq, Tk, dtype=work)
    if mask is not None:
        add = (~mask).to(work).view(B, 1, Tq, Tk) * MASKED
    S = Q @ K.transpose(-1, -2) * scale + add
    lse = torch.logsumexp(S, dim=-1)
    P = (S - lse.unsqueeze(-1)).exp()
    kp = keep.to(work) * inv_keep if keep is not None else torch.ones((), dtype=work)
    Pd = rnd(P * kp)
    O = rnd(Pd @ V)
    dV = rnd(Pd.transpose(-1, -2) @ dO)
    dP = (dO @ V.transpose(-1, -2)) * kp
    delta = (dO * O).sum(-1, keepdim=True)
    dS = rnd(P * (dP - delta))
    dQ = rnd(scale * (dS @ K))
    dK = rnd(scale * (dS.transpose(-1, -2) @ Q))
    r = {"O": merge_heads(O), "dQ": merge_heads(dQ), "dK": merge_heads(dK), "dV": merge_heads(dV), "lse": lse, "P": P}
    if magnitudes:
        aQ, aK, aV, adO = Q.abs(), K.abs(), V.abs(), dO.abs()
        M_O = Pd @ aV
        M_dV = Pd.transpose(-1, -2) @ adO
        M_dS = P * ((adO @ aV.transpose(-1, -2)) * kp + (adO * M_O).sum(-1, keepdim=True))
        M_dQ = scale * (M_dS @ aK)
        M_dK = scale * (M_dS.transpose(-1, -2) @ aQ)
        M_lse = (P * (scale * (aQ @ aK.transpose(-1, -2)))).sum(-1)   # d lse = sum_j P_j dS_j
        r["M"] = {"O": merge_heads(M_O), "dQ": merge_heads(M_dQ), "dK": merge_heads(M_dK), "dV": merge_heads(M_dV), "lse": M_lse}
    return r


def attention(q, k, v, do, B, H, Tq, Tk, dh, mask=None, keep=None, inv_keep=1.0, scale=None):
    """fp64 values of the inputs as given (already rounded to the kernel's type by the caller): a dict with O [B*Tq, H*dh],
    dQ, dK [B*Tk, H*dh], dV (heads merged), lse [B, H, Tq], P [B, H, Tq, Tk], and M, a dict of the magnitudes of O, dQ, dK,
    dV and lse.  mask: bool [B, Tq, Tk] (attend_mask) or None; keep: 0/1 [B, H, Tq, Tk] or None; inv_keep = 1 / (1 - p)."""
    scale = kernel_scale(dh) if scale is None else scale
    return _compute(q, k, v, do, B, H, Tq, Tk, dh, mask, keep, inv_keep, scale, torch.float64, lambda t: t, True)


def emulate(dtype):
    """attention() in fp32 torch with roundings to ``dtype`` where the kernels round: Pd before Pd V and Pd^T dO, O as stored
    (what delta is taken from), dS before the two products, each stored output.  (dtype fp32: a plain fp32 evaluation.)"""
    def rnd(t):
        return t.to(dtype).float()

    def run(q, k, v, do, B, H, Tq, Tk, dh, mask=None, keep=None, inv_keep=1.0, scale=None):
        scale = kernel_scale(dh) if scale is None else scale
        return _compute(q, k, v, do, B, H, Tq, Tk, dh, mask, keep, inv_keep, scale, torch.float32, rnd, False)
    return run


def compared(name, B, H, Tq, T_rows, dh, dead_rows):
    """bool mask over the merged [B*T, H*dh] output ``name`` (or [B, H, Tq] for lse): False on the fully-masked query rows of
    O, dQ and lse (their softmax is over scores that all carry -10000: fp32 keeps 2^-10 of them), True everywhere for dK, dV.
    dead_rows: bool [B, Tq]."""
    if name == "lse":
        return ~dead_rows.view(B, 1, Tq).expand(B, H, Tq)
    if name in ("O", "dQ"):
        return ~dead_rows.view(B * Tq, 1).expand(B * Tq, H * dh)
    return torch.ones(B * T_rows, H * dh, dtype=torch.bool)


def ratio(got, ref, M, u, where):
    """Worst |got - ref| / (u * (M + |ref|)) over ``where``; elements whose bound is zero must be equal and count as 0 (inf
    otherwise)."""
    got, ref, M = got.detach().double().cpu(), ref.double(), M.double()
    err = (got - ref).abs()
    unit = u * (M + ref.abs())
    sel = where & (unit > 0)
    worst = float((err[sel] / unit[sel]).max()) if bool(sel.any()) else 0.0
    if bool((err[where & (unit == 0)] != 0).any()):
        return float("inf")
    return worst


def lse_floor(lse):
    """4 ulp (fp32) of |lse|."""
    a = lse.double().abs().clamp_min(2.0 ** -126)
    return 4.0 * torch.pow(2.0, torch.floor(torch.log2(a)) - 23.0)


# ------------------------------------------------------------------------------------------------ cases
# family: the kernel the case is there for; bwd: the backward kernel(s) the plan in csrc/attention.hip must reach for it
Case = collections.namedtuple("Case", "id family dtype dh B Tq Tk mask p seed env bwd packed proj")
H = 3
NO_SHORT, NO_FUSED = "IMT_ATTN_NO_SHORT_FWD", "IMT_ATTN_NO_FUSED_BWD"
MASK_KINDS = ("klen", "qlen_causal", "causal", "m3d", "kcq")
BIG_SEED = (1 << 35) + 77


def _plan_bwd(dtype, Tq, Tk, env):
    if dtype == "f32" or NO_FUSED in env:
        return "pair"
    if Tq <= 128 and Tk <= 128:
        return "fused"
    return "fused256" if Tq <= 256 and Tk <= 256 else "pair"


def _case(family, dtype, dh, Tq, Tk, mask="none", p=0.0, seed=0, env=(), B=2, packed=False, proj=False, bwd=None):
    planned = _plan_bwd(dtype, Tq, Tk, env)
    assert bwd is None or bwd == planned, (family, dtype, Tq, Tk, bwd, planned)   # the table below names the kernel it means
    cid = "%s-%s-dh%d-%dx%d" % (family, dtype, dh, Tq, Tk)
    cid += ("-" + mask if mask != "none" else "") + ("-p%g" % p if p else "") + ("-bigseed" if seed >= 1 << 32 else "")
    cid += ("-B%d" % B if B != 2 else "") + ("-packed" if packed else "") + ("-proj" if proj else "")
    return Case(cid, family, dtype, dh, B, Tq, Tk, mask, p, seed, tuple(env), planned, packed, proj)


TILED = [(1, 1), (1, 65), (16, 64), (17, 65), (64, 128), (65, 129), (63, 191), (64, 192)]
LONG = [(257, 1), (1, 257), (130, 257), (257, 257), (300, 130)]
SHORT = [(65, 1), (65, 128), (113, 17), (128, 127), (128, 128)]
FUSED = [(1, 1), (17, 31), (64, 128), (65, 33), (128, 128)]
FUSED256 = [(1, 129), (129, 1), (129, 128), (128, 129), (193, 255), (200, 33), (256, 256)]
PAIR_ENV = [(128, 128), (193, 255)]


def _all_cases():
    cs = []
    for dh in (64, 32):
        # tiled forward, dQ, dK/dV: fp32 (dh 64 stages one 64-key sub-tile per trip, dh 32 two); bf16 reaches the tiled
        # forward with Tq <= 64 (its backward goes where the plan sends it)
        cs += [_case("tiled", "f32", dh, tq, tk, bwd="pair") for tq, tk in TILED]
        cs += [_case("tiled", "bf16", dh, tq, tk) for tq, tk in TILED if tq <= 64 or tk > 128]
        cs += [_case("long", "f32", dh, tq, tk, bwd="pair", B=3 if (tq, tk) == (130, 257) else 2) for tq, tk in LONG]
        cs += [_case("long", "bf16", dh, tq, tk, bwd="pair", B=3 if (tq, tk) == (130, 257) else 2) for tq, tk in LONG]
        cs += [_case("short", "bf16", dh, tq, tk, bwd="fused") for tq, tk in SHORT]
        cs += [_case("fused", "bf16", dh, tq, tk, bwd="fused") for tq, tk in FUSED]
        cs += [_case("fused256", "bf16", dh, tq, tk, bwd="fused256", B=3 if (tq, tk) == (200, 33) else 2) for tq, tk in FUSED256]
        cs += [_case("pair", "bf16", dh, tq, tk, env=(NO_FUSED,), bwd="pair") for tq, tk in PAIR_ENV]
    # q | k | v read from one [N, 3d] buffer, dQ | dK | dV written into the column slices of another (the model's layout)
    cs += [_case("fused", "bf16", 64, 128, 128, packed=True), _case("fused256", "bf16", 64, 256, 256, packed=True),
           _case("long", "bf16", 64, 257, 257, packed=True), _case("long", "f32", 32, 257, 257, packed=True)]
    # masks: every kind on every kernel family at a ragged shape
    for kind in MASK_KINDS:
        cs += [_case("tiled", "f32", 64, 65, 129, kind), _case("tiled", "f32", 32, 65, 129, kind),
               _case("tiled", "bf16", 64, 63, 191, kind), _case("long", "f32", 64, 130, 257, kind),
               _case("long", "bf16", 64, 130, 257, kind, bwd="pair"), _case("short", "bf16", 64, 128, 127, kind, bwd="fused"),
               _case("fused", "bf16", 64, 100, 97, kind, bwd="fused"), _case("fused256", "bf16", 64, 193, 255, kind, bwd="fused256"),
               _case("pair", "bf16", 64, 193, 255, kind, env=(NO_FUSED,), bwd="pair")]
    cs += [_case("short", "bf16", 64, 113, 17, "m3d"), _case("short", "bf16", 32, 113, 17, "m3d"), _case("short", "bf16", 32, 128, 127, "m3d")]
    # dropout: every family at an odd and an even Tk, both rates
    for p, q in ((0.1, 0.5), (0.5, 0.1)):
        cs += [_case("short", "bf16", 64, 113, 17, p=p, seed=11), _case("short", "bf16", 64, 128, 128, p=q, seed=12),
               _case("short", "bf16", 32, 128, 127, p=p, seed=13),
               _case("tiled", "bf16", 64, 17, 65, p=p, seed=14), _case("tiled", "bf16", 64, 64, 128, p=q, seed=15),
               _case("tiled", "f32", 64, 17, 65, p=q, seed=16), _case("tiled", "f32", 32, 64, 128, p=p, seed=17),
               _case("fused", "bf16", 64, 17, 31, p=p, seed=18), _case("fused", "bf16", 32, 64, 128, p=q, seed=19),
               _case("fused256", "bf16", 64, 193, 255, p=p, seed=20), _case("fused256", "bf16", 64, 256, 256, p=q, seed=21),
               _case("pair", "bf16", 64, 193, 255, p=q, seed=22, env=(NO_FUSED,)), _case("pair", "bf16", 64, 128, 128, p=p, seed=23, env=(NO_FUSED,)),
               _case("long", "bf16", 64, 257, 257, p=p, seed=24), _case("long", "bf16", 64, 300, 130, p=q, seed=25),
               _case("long", "f32", 64, 257, 257, p=q, seed=26), _case("long", "f32", 32, 300, 130, p=p, seed=27)]
    cs += [_case("short", "bf16", 64, 128, 127, p=0.1, seed=BIG_SEED), _case("long", "bf16", 64, 257, 257, p=0.5, seed=BIG_SEED + 1),
           _case("fused256", "bf16", 64, 193, 255, "kcq", p=0.1, seed=31),
           _case("fused", "bf16", 64, 128, 127, p=0.1, seed=32, proj=True), _case("fused", "bf16", 64, 65, 33, "klen", proj=True)]
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cs


CASES = _all_cases()
BY_ID = {c.id: c for c in CASES}


def _masks(c, g):
    """(key_mask [B, Tk] | None, query_mask [B, Tq] | None, mask3d [B, Tq, Tk] | None, causal) as uint8 CPU tensors."""
    B, Tq, Tk = c.B, c.Tq, c.Tk
    km = qm = m3 = None
    causal = c.mask in ("qlen_causal", "causal", "kcq")
    if c.mask in ("klen", "kcq"):
        # one batch element with a single valid key, one that ends one past a 64-key tile (where Tk reaches that far)
        lens = [1, min(65, Tk)] + [Tk] * (B - 2)
        km = (torch.arange(Tk).view(1, Tk) < torch.tensor(lens).view(B, 1)).to(torch.uint8)
    if c.mask in ("qlen_causal", "kcq"):
        lens = [Tq - Tq // 4, Tq] + [Tq - 1] * (B - 2)     # >= 3/4 Tq: at most a quarter of the rows is fully masked
        qm = (torch.arange(Tq).view(1, Tq) < torch.tensor(lens).view(B, 1)).to(torch.uint8)
    if c.mask == "m3d":
        m3 = (torch.rand(B, Tq, Tk, generator=g) < 0.7).to(torch.uint8)
        i = torch.arange(Tq)
        m3[:, i, i.clamp_max(Tk - 1)] = 1
    return km, qm, m3, causal


@functools.lru_cache(maxsize=None)
def make_inputs(cid):
    """The inputs of a case, on the CPU and rounded to its dtype: q, k ~ 0.5 N(0, 1) (every attendable probability stays
    >= 2^-12: a kept entry cannot round to zero in bf16), v, dO ~ N(0, 1); dO is zero on fully-masked query rows.  Shared
    among the tests and never modified."""
    c = BY_ID[cid]
    g = torch.Generator().manual_seed(zlib.crc32(cid.encode()))
    dt, d = TORCH_DTYPE[c.dtype], H * c.dh
    q = (torch.randn(c.B * c.Tq, d, generator=g) * 0.5).to(dt)
    k = (torch.randn(c.B * c.Tk, d, generator=g) * 0.5).to(dt)
    v = torch.randn(c.B * c.Tk, d, generator=g).to(dt)
    do = torch.randn(c.B * c.Tq, d, generator=g).to(dt)
    km, qm, m3, causal = _masks(c, g)
    mask = attend_mask(c.B, c.Tq, c.Tk, km, qm, m3, causal)
    dead = ~mask.any(-1)                                   # [B, Tq]: no attendable key
    do[dead.view(-1)] = 0
    r = dict(q=q, k=k, v=v, do=do, key_mask=km, query_mask=qm, mask3d=m3, causal=causal, mask=mask, dead=dead,
             inv_keep=kernel_inv_keep(c.p))
    if c.proj:   # dO = dy W_o is formed by the kernel under test; the test takes dO from what it stored
        r["dy"] = torch.randn(c.B * c.Tq, d, generator=g).to(dt)
        r["w_o"] = (torch.randn(d, d, generator=g) / math.sqrt(d)).to(dt)
        r["do"] = None
    return r


def surrogate_keep(c):
    """A Bernoulli(1 - p) [B, H, Tq, Tk] mask from a CPU generator: stands in for the kernels' mask where only the size of
    the rounding error matters (bound_constants), never where values are compared with a kernel's."""
    if c.p <= 0:
        return None
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()) ^ 0x5eed)
    return (torch.rand(c.B, H, c.Tq, c.Tk, generator=g) >= c.p).to(torch.float64)


@functools.lru_cache(maxsize=None)
def emulation_ratios(cid):
    """{output: worst |emulate - fp64| / (u * (M + |fp64|))} of one case, lse included (against u = 2^-24)."""
    c, x = BY_ID[cid], make_inputs(cid)
    do = x["do"] if x["do"] is not None else (x["dy"].double() @ x["w_o"].double()).to(TORCH_DTYPE[c.dtype])
    keep = surrogate_keep(c)
    args = (x["q"], x["k"], x["v"], do, c.B, H, c.Tq, c.Tk, c.dh)
    ref = attention(*args, mask=x["mask"], keep=keep, inv_keep=x["inv_keep"])
    emu = emulate(TORCH_DTYPE[c.dtype])(*args, mask=x["mask"], keep=keep, inv_keep=x["inv_keep"])
    out = {}
    for name in OUTPUTS + ("lse",):
        where = compared(name, c.B, H, c.Tq, c.Tk, c.dh, x["dead"])
        out[name] = ratio(emu[name], ref[name], ref["M"][name], U["f32"] if name == "lse" else U[c.dtype], where)
    return out


@functools.lru_cache(maxsize=None)
def bound_constants():
    """{(dtype, output): c}: margin x the worst emulation ratio over ALL cases of that dtype.  Computed, not written down."""
    worst = {}
    for c in CASES:
        for name, r in emulation_ratios(c.id).items():
            worst[(c.dtype, name)] = max(worst.get((c.dtype, name), 0.0), r)
    return {(dt, name): r * (LSE_MARGIN if name == "lse" else MARGIN[dt]) for (dt, name), r in worst.items()}
