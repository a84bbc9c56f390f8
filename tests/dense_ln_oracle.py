"""fp64 restatement of y = LayerNorm(dropout(alpha x W^T + b) + resid), the operation behind imt_gemm_bias_residual_ln
(csrc/gemm_ln.hip) and imt_gemm(..., ln_out=...) (csrc/gemm.hip), plus the case lists and the input data of
tests/test_gpu_dense_ln_edges.py (checked on the CPU by tests/test_dense_ln_oracle.py).

    pre64 = keep * inv_keep * (alpha * x W^T + b) + resid        (the keep mask is an ARGUMENT, never restated here)
    pre   = pre64 rounded ONCE, to nearest even, to the compute type: what the kernels store and imt_layernorm_bwd reads
    mean, rstd, y = LayerNorm statistics and output of that ROUNDED pre, in fp64 (biased variance)

The LayerNorm bounds are the ones of tests/test_gpu_row_edges.py::test_layernorm_fwd_bwd (rowops_oracle.layernorm_bounds: one
definition for both files).  Exact data: operands from gemm_oracle.integer_operands, integer bias / residual, p = 0.5
(inv_keep = 2), alpha a power of two -- every fp32 partial sum is exact in any K order, so fp32 ``pre`` must equal the
oracle bit for bit and bf16 ``pre`` the oracle rounded once; gamma and beta are real-valued."""
import collections
import functools

import torch

from tests import gemm_oracle as GO
from tests import rowops_oracle as RO

F32, BF16 = torch.float32, torch.bfloat16
DT = {"bf16": BF16, "f32": F32}
P_DROP, INV_KEEP = 0.5, 2.0
SEED = 0x2545F4914F6CDD1D
ALPHA, ALPHA_DEV = 0.25, 0.5   # the `alpha` epilogue of imt_gemm: alpha with alpha_dev, both powers of two


def bk(dtype):
    """K elements per 128-byte K tile."""
    return 64 if dtype == "bf16" else 32


def al(dtype):
    """Elements per 16-byte chunk."""
    return 8 if dtype == "bf16" else 4


# ------------------------------------------------------------------------------------------------ the oracle
def reference(x, W, dtype, gamma, beta, eps, *, bias=None, resid=None, keep=None, alpha=1.0):
    """dict(pre64, mag, pre, mean, rstd, y): ``pre`` in ``dtype`` (pre64 rounded once), everything else fp64; ``mag`` the
    summed magnitude of the terms of pre64 (for gemm_oracle.bound on real-valued data).  ``keep``: bool [M, N], p = 0.5."""
    x, W = x.double(), W.double()
    v, mag = float(alpha) * (x @ W.t()), abs(float(alpha)) * (x.abs() @ W.abs().t())
    if bias is not None:
        v, mag = v + bias.double()[None, :], mag + bias.double().abs()[None, :]
    if keep is not None:
        assert keep.dtype == torch.bool and keep.shape == v.shape
        v, mag = torch.where(keep, INV_KEEP * v, torch.zeros_like(v)), torch.where(keep, INV_KEEP * mag, torch.zeros_like(mag))
    if resid is not None:
        v, mag = v + resid.double(), mag + resid.double().abs()
    pre = v.to(dtype)
    res = layernorm(pre, gamma, beta, eps)
    res.update(pre64=v, mag=mag, pre=pre)
    return res


def layernorm(pre, gamma, beta, eps):
    """dict(mean, rstd, y) in fp64 of the rows ``pre`` taken as they are."""
    p, g, b = pre.double(), gamma.double(), beta.double()
    mean = p.mean(-1, keepdim=True)
    var = ((p - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / (var + float(torch.tensor(eps, dtype=F32))).sqrt()   # eps travels as a float
    return dict(mean=mean.squeeze(-1), rstd=rstd.squeeze(-1), y=(p - mean) * rstd * g + b)


def bounds(pre, ref, dtype):
    """(y, mean, rstd) bounds of rowops_oracle.layernorm_bounds for the rows ``pre``."""
    return RO.layernorm_bounds(pre, ref["y"], ref["rstd"], dtype)


def pre_bound(ref, dtype):
    """Element-wise bound of |pre - pre64| on REAL-valued data: gemm_oracle.bound of a plain epilogue."""
    return GO.bound(dict(out=ref["pre64"], mag=ref["mag"]), GO.AUX_NONE, dtype)


def fp32_evaluation(x, W, dtype, gamma, beta, eps, *, bias=None, resid=None, keep=None, alpha=1.0, pre=None):
    """The same formula in plain fp32 torch on the CPU: dict(pre, mean, rstd, y), ``y`` rounded to ``dtype`` as a kernel stores
    it.  ``pre``: normalise these rows instead of the fp32 product (real-valued data: the oracle's rounded rows)."""
    v = torch.tensor(alpha, dtype=F32) * (x.float() @ W.float().t())
    if bias is not None:
        v = v + bias.float()[None, :]
    if keep is not None:
        v = torch.where(keep, v * INV_KEEP, torch.zeros_like(v))
    if resid is not None:
        v = v + resid.float()
    own = v.to(dtype)
    p = (own if pre is None else pre).float()
    mean = p.sum(-1, keepdim=True) / p.shape[-1]
    var = ((p - mean) ** 2).sum(-1, keepdim=True) / p.shape[-1]
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
    y = ((p - mean) * rstd * gamma.float() + beta.float()).to(dtype)
    return dict(pre=own, mean=mean.squeeze(-1), rstd=rstd.squeeze(-1), y=y)


def worst_ratio(got, ref, bound):
    """Worst |got - ref| / bound over all elements (inf for a non-finite result, or a non-zero error where the bound is zero)."""
    got = got.detach().double().cpu()
    ref, bound = ref.double().expand_as(got), bound.double().expand_as(got)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)   # x / 0 = inf
    return float(ratio.max()) if ratio.numel() else 0.0


# ------------------------------------------------------------------------------------------------ epilogues
# name -> (bias, dropout, residual)
EPILOGUES = collections.OrderedDict([("none", (0, 0, 0)), ("bias", (1, 0, 0)), ("resid", (0, 0, 1)), ("bias_resid", (1, 0, 1)),
                                     ("bias_drop_resid", (1, 1, 1)), ("drop", (0, 1, 0))])
BDR = "bias_drop_resid"


# ------------------------------------------------------------------------------------------------ A: imt_gemm_bias_residual_ln
# data: "int" exact integers | "degenerate" rows DEGENERATE_ROWS of x zero, no bias, the residual row constant | "gauss" real-valued
FusedCase = collections.namedtuple("FusedCase", "id dtype N nt M epi eps data")
DEGENERATE_ROWS = (5, 32)   # of M = 33: a row in the middle of the first tile and the one live row of the last
INSTANCES = {128: (1, 1, 4), 256: (2, 1, 4), 384: (3, 1, 3), 512: (4, 2, 4)}   # N -> (NTW, SPLIT, NST)

# (N, M, nt, eps): bias + dropout + residual on exact data.  ns = nt * SPLIT slots are streamed, the prologue issues NST - 1,
# slot q waits for min(NST - 2, ns - 1 - q) newer ones; workgroup b starts at K tile (b / 8) % nt.
_FUSED_SHAPES = [
    # ---- N = 128: (NTW, SPLIT, NST) = (1, 1, 4)
    (128, 1, 1, 1e-12),    # ns = 1 < NST - 1: two of the three prologue issues are skipped, vmcnt(0) at once; every row but 0 clamped
    (128, 31, 2, 1e-5),    # ns = 2 < NST - 1; the last row of the tile is past M: zero-filled A, clamped residual row
    (128, 32, 3, 1e-12),   # ns = NST - 1: the prologue fills the ring, no in-loop issue; newer = 2, 1, 0; NaN guard row right behind A
    (128, 33, 4, 1e-5),    # ns = NST: the first in-loop issue (slot 3 at q = 0); one live row in the second workgroup
    (128, 289, 5, 1e-12),  # one slot reused; 10 workgroups: 8 and 9 start at K tile 1 and wrap (k >= nt)
    (128, 769, 3, 1e-5),   # 25 workgroups, phases 0, 1, 2, 0; every phase != 0 wraps
    (128, 33, 9, 1e-12),   # every slot reused twice: newer = 2 at the head for seven steps, then 1, 0 at the tail
    # ---- N = 256: (2, 1, 4)
    (256, 1, 2, 1e-5),     # ns = 2 < NST - 1
    (256, 31, 1, 1e-12),   # ns = 1
    (256, 32, 4, 1e-5),    # ns = NST
    (256, 33, 3, 1e-12),   # ns = NST - 1
    (256, 289, 9, 1e-5),   # every slot reused twice, blocks 8 and 9 rotated by one tile
    (256, 769, 5, 1e-12),  # phases 0..3 of 5: phase 3 wraps after two tiles
    # ---- N = 384: (3, 1, 3)
    (384, 1, 1, 1e-12),    # ns = 1 < NST - 1 = 2
    (384, 31, 2, 1e-5),    # ns = NST - 1: newer = 1, 0
    (384, 32, 3, 1e-12),   # ns = NST: first in-loop issue
    (384, 33, 7, 1e-5),    # every slot reused twice
    (384, 289, 4, 1e-12),  # one reuse; blocks 8, 9 at phase 1
    (384, 769, 2, 1e-5),   # phases 0, 1, 0, 1 with ns = NST - 1
    # ---- N = 512: (4, 2, 4): two slots (weight halves) per K tile
    (512, 1, 1, 1e-5),     # ns = 2 < NST - 1: both halves of the one tile, hstep
    (512, 31, 2, 1e-12),   # ns = 4 = NST: first in-loop issue is the second half of tile 1
    (512, 32, 3, 1e-5),    # ns = 6: slots 0, 1 reused
    (512, 33, 5, 1e-12),   # ns = 10: every slot reused twice
    (512, 289, 3, 1e-12),  # blocks 8, 9 rotated: the halves of tile 1 first
    (512, 769, 5, 1e-5),   # phases 0..3, the largest shape of the file
]
SWEEP_M, SWEEP_NT = 33, 2    # the shape of the epilogue sweep, the degenerate rows and the real-valued case of every instance


def _fused_cases():
    out = []
    for dtype in ("bf16", "f32"):
        for (N, M, nt, eps) in _FUSED_SHAPES:
            out.append(FusedCase("N%d_M%d_nt%d_%s" % (N, M, nt, dtype), dtype, N, nt, M, BDR, eps, "int"))
        for N in INSTANCES:
            # rows whose pre-LN value is constant: y == beta exactly, rstd = 1 / sqrt(eps); both eps over the instances
            out.append(FusedCase("N%d_degenerate_%s" % (N, dtype), dtype, N, SWEEP_NT, SWEEP_M, "resid", 1e-12 if N in (128, 384) else 1e-5, "degenerate"))
            # Gaussian operands: the only data on which statistics of the UNROUNDED pre-LN value would show
            out.append(FusedCase("N%d_gauss_%s" % (N, dtype), dtype, N, 3, 61, BDR, 1e-12, "gauss"))
    return out


FUSED_CASES = _fused_cases()
SWEEP_CASES = [FusedCase("N%d_sweep_%s" % (N, dtype), dtype, N, SWEEP_NT, SWEEP_M, None, 1e-12 if N in (256, 512) else 1e-5, "int")
               for dtype in ("bf16", "f32") for N in INSTANCES]


# ------------------------------------------------------------------------------------------------ B: imt_gemm(..., ln=...)
# epi: "bias" | "bias_drop_resid" | "alpha" (alpha with alpha_dev) | "bias_resid" | "bias_gelu"; ws: a split-K workspace is passed;
# kinds: the profiler kinds the call must launch; refused: the message the call must fail with AFTER those launches (None: succeeds)
GemmCase = collections.namedtuple("GemmCase", "id dtype M N K epi ws kinds refused")
LN_KIND = "layernorm_fwd"


def _gemm_cases():
    out = []

    def add(tag, dtype, M, N, K, epi, ws, kinds, refused=None):
        out.append(GemmCase("%s_%dx%dx%d_%s_%s" % (tag, M, N, K, epi, dtype), dtype, M, N, K, epi, ws, kinds, refused))

    # ---- split-K workspace, bf16: the epilogue launch normalises (splitk_ws_ln_fused; nt >= 8 K tiles and <= 32 output tiles split)
    fused = ["gemm_ws_bf16_nt", "gemm_splitk_epilogue_ln"]
    k8, k16 = 8 * bk("bf16"), 16 * bk("bf16")
    add("fused", "bf16", 1, 128, k8, "bias", True, fused)                 # NCH 1, lanes 32..63 clamped to column N - 4; three waves leave early
    add("fused", "bf16", 3, 256, k8, BDR, True, fused)                    # NCH 1, every lane live; one wave leaves early
    add("fused", "bf16", 4, 260, k8, "alpha", True, fused)                # NCH 2, one live lane in the second chunk; a whole workgroup
    add("fused", "bf16", 5, 768, k8, BDR, True, fused)                    # NCH 3 full; M % 4 = 1
    add("fused", "bf16", 61, 1024, k8, "bias", True, fused)               # NCH 4 full, the limit; 16 workgroups, the last with one row
    add("fused", "bf16", 5, 516, k8, "alpha", True, fused)                # NCH 3 with a clamped last chunk (one live lane)
    add("fused", "bf16", 3, 772, k8, BDR, True, fused)                    # NCH 4 with a clamped last chunk
    add("fused", "bf16", 61, 260, k16, BDR, True, fused)                  # nt = 16: the long-K rule splits as well
    # N > 1024 does not fuse: the epilogue launch stores C, and the LayerNorm launch behind it refuses rows that long
    add("nofuse", "bf16", 5, 1028, k16, "bias", True, ["gemm_ws_bf16_nt", "gemm_splitk_epilogue"], "layernorm: d=1028 > 1024")
    # ---- the same shapes in fp32: c_dtype == IMT_F32 never fuses.  nt = 8 is not split at all (the short-K rule is the fused
    # launch's), nt = 16 is split and normalised by a LayerNorm launch
    single32, split32 = ["gemm_ws_f32_nt", LN_KIND], ["gemm_ws_f32_nt", "gemm_splitk_epilogue", LN_KIND]
    k8, k16 = 8 * bk("f32"), 16 * bk("f32")
    add("fp32", "f32", 1, 128, k8, "bias", True, single32)
    add("fp32", "f32", 3, 256, k8, BDR, True, single32)
    add("fp32", "f32", 4, 260, k8, "alpha", True, single32)
    add("fp32", "f32", 5, 768, k8, BDR, True, single32)
    add("fp32", "f32", 61, 1024, k8, "bias", True, single32)
    add("fp32", "f32", 5, 516, k8, "alpha", True, single32)
    add("fp32", "f32", 3, 772, k8, BDR, True, single32)
    add("fp32", "f32", 61, 260, k16, BDR, True, split32)                  # split-K, not fused: epilogue launch + LayerNorm launch
    add("nofuse", "f32", 5, 1028, k16, "bias", True, ["gemm_ws_f32_nt", "gemm_splitk_epilogue"], "layernorm: d=1028 > 1024")
    # ---- LayerNorm behind the product
    for dtype in ("bf16", "f32"):
        one = "gemm_ws_%s_nt" % dtype
        add("behind_single", dtype, 300, 384, 3 * bk(dtype), BDR, False, [one, LN_KIND])
        # ragged K at the smallest K the strategy takes: 16 whole tiles + one 16-byte chunk; bias and residual ride on the tail
        add("behind_ragged", dtype, 61, 256, 16 * bk(dtype) + al(dtype), "bias_resid", False, ["gemm_sbuf_%s_nt" % dtype, one, LN_KIND])
        # split-K with a GELU aux: splitk_ws_ln_fused is false in both types
        add("behind_splitk_gelu", dtype, 61, 256, 16 * bk(dtype), "bias_gelu", True, [one, "gemm_splitk_epilogue", LN_KIND])
    return out


GEMM_CASES = _gemm_cases()

# ------------------------------------------------------------------------------------------------ C: the three paths on one data set
ContractCase = collections.namedtuple("ContractCase", "id dtype M N K")
CONTRACT_CASES = [ContractCase("contract_N%d_%s" % (N, dtype), dtype, 61, N, 16 * bk(dtype)) for dtype in ("bf16", "f32") for N in INSTANCES]


# ------------------------------------------------------------------------------------------------ data (CPU, computed once, never modified)
@functools.lru_cache(maxsize=None)
def inputs(dtype, M, N, K, data="int"):
    """dict(x, W, bias, resid, gamma, beta, dy): fp32 CPU tensors holding values of ``dtype``."""
    T = DT[dtype]
    g = torch.Generator().manual_seed(100003 * M + 101 * N + K)
    if data == "gauss":
        x = torch.randn(M, K, generator=g)
        W = torch.randn(N, K, generator=g) / K ** 0.5
        bias = torch.randn(N, generator=g) * 0.2
        resid = torch.randn(M, N, generator=g)
    else:
        x, W = GO.integer_operands(GO.NT, M, N, K, 100003 * M + 101 * N + K)
        bias = torch.randint(-4, 5, (N,), generator=g).float()
        resid = torch.randint(-3, 4, (M, N), generator=g).float()
        if data == "degenerate":
            for r in DEGENERATE_ROWS:
                x[r] = 0.0
                resid[r] = 3.0
    gamma = torch.randn(N, generator=g)
    beta = torch.randn(N, generator=g) * 0.3
    dy = torch.randn(M, N, generator=g)
    return {k: v.to(T).float() for k, v in dict(x=x, W=W, bias=bias, resid=resid, gamma=gamma, beta=beta, dy=dy).items()}


def epilogue_terms(epi, d, keep):
    """kwargs of ``reference`` / ``fp32_evaluation`` for epilogue ``epi`` on the data ``d`` under the mask ``keep``."""
    if epi == "alpha":
        return dict(alpha=ALPHA * ALPHA_DEV)
    b, drop, r = EPILOGUES[epi]
    return dict(bias=d["bias"] if b else None, keep=keep if drop else None, resid=d["resid"] if r else None)


def uses_dropout(epi):
    return epi in EPILOGUES and bool(EPILOGUES[epi][1])
