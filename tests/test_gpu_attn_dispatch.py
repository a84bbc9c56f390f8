"""Which kernel imt_attention_bwd / imt_attention_bwd_proj launch for a shape: one row per threshold of the host-side plan in
csrc/attention.hip (fp32 -> the dQ + dK/dV pair; bf16: Tq, Tk <= 128 -> the fused kernel, <= 256 -> its 256-key sibling,
beyond -> the pair; the IMT_ATTN_NO_FUSED_BWD / IMT_ATTN_NO_FUSED256 switches), with the flop and byte figures each launch
declares to the profiler (bench.py's roofline reads them).

The expected kinds and figures were recorded from the library BEFORE the host section was rewritten as validate / plan /
launch; they pin the dispatch, not the numerics (those stay with test_gpu_ops.py / test_gpu_attn_bwd_proj.py).

Two things this file cannot pin:
  * the forward's choice: the short and the tiled forward kernel both report as attn_fwd_bf16, so the profiler does not
    tell them apart.  The rule is one predicate in attention.hip (bf16, 64 < Tq <= 128, Tk <= 128, 32-bit dropout indices,
    IMT_ATTN_NO_SHORT_FWD unset) and is compared by eye;
  * the 32-bit-index boundary ((double)B * H * Tq * Tk < 2^32): it needs 2^32 score elements, 262 144 (batch, head) pairs
    at 128 x 128 and gigabytes per operand."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

B, H = 2, 2
FUSED, FUSED256 = "attn_bwd_fused_bf16", "attn_bwd_fused256_bf16"
DQ, DKDV = "attn_bwd_dq_", "attn_bwd_dkdv_"

# (dtype, head_dim, Tq, Tk, options, {kind: (launches, flops, bytes)}).  options: mask3d (an explicit [B, Tq, Tk] mask: the
# MASK3D instance of the same kernel) / env (this switch is set for the call) / proj (hip_ops.attention_bwd_proj: dO = dy W_o
# formed inside the fused kernel, reported under its kind with the projection's work added)
CASES = [
    ("bf16", 64, 1, 1, {}, {FUSED: (1, 2560, 4096)}),
    ("bf16", 64, 128, 128, {}, {FUSED: (1, 41943040, 524288)}),
    ("bf16", 64, 129, 128, {}, {FUSED256: (1, 42270720, 526336)}),
    ("bf16", 64, 128, 129, {}, {FUSED256: (1, 42270720, 526336)}),
    ("bf16", 64, 256, 256, {}, {FUSED256: (1, 167772160, 1048576)}),
    ("bf16", 64, 257, 256, {}, {DQ + "bf16": (1, 101056512, 787968), DKDV + "bf16": (1, 134742016, 787968)}),
    ("bf16", 64, 256, 257, {}, {DQ + "bf16": (1, 101056512, 787968), DKDV + "bf16": (1, 134742016, 787968)}),
    ("bf16", 32, 1, 1, {}, {FUSED: (1, 1280, 2048)}),
    ("bf16", 32, 128, 128, {}, {FUSED: (1, 20971520, 262144)}),
    ("bf16", 32, 129, 128, {}, {FUSED256: (1, 21135360, 263168)}),
    ("bf16", 32, 128, 129, {}, {FUSED256: (1, 21135360, 263168)}),
    ("bf16", 32, 256, 256, {}, {FUSED256: (1, 83886080, 524288)}),
    ("bf16", 32, 257, 256, {}, {DQ + "bf16": (1, 50528256, 393984), DKDV + "bf16": (1, 67371008, 393984)}),
    ("bf16", 32, 256, 257, {}, {DQ + "bf16": (1, 50528256, 393984), DKDV + "bf16": (1, 67371008, 393984)}),
    ("bf16", 64, 128, 128, {"mask3d": 1}, {FUSED: (1, 41943040, 524288)}),
    ("bf16", 64, 200, 200, {"mask3d": 1}, {FUSED256: (1, 102400000, 819200)}),
    ("f32", 64, 64, 64, {}, {DQ + "f32": (1, 6291456, 393216), DKDV + "f32": (1, 8388608, 393216)}),
    ("f32", 64, 128, 128, {}, {DQ + "f32": (1, 25165824, 786432), DKDV + "f32": (1, 33554432, 786432)}),
    ("f32", 32, 64, 64, {}, {DQ + "f32": (1, 3145728, 196608), DKDV + "f32": (1, 4194304, 196608)}),
    ("f32", 32, 128, 128, {}, {DQ + "f32": (1, 12582912, 393216), DKDV + "f32": (1, 16777216, 393216)}),
    ("bf16", 64, 128, 128, {"env": "IMT_ATTN_NO_FUSED_BWD"}, {DQ + "bf16": (1, 25165824, 393216), DKDV + "bf16": (1, 33554432, 393216)}),
    ("bf16", 64, 200, 200, {"env": "IMT_ATTN_NO_FUSED_BWD"}, {DQ + "bf16": (1, 61440000, 614400), DKDV + "bf16": (1, 81920000, 614400)}),
    ("bf16", 64, 200, 200, {"env": "IMT_ATTN_NO_FUSED256"}, {DQ + "bf16": (1, 61440000, 614400), DKDV + "bf16": (1, 81920000, 614400)}),
    ("bf16", 64, 128, 128, {"env": "IMT_ATTN_NO_FUSED256"}, {FUSED: (1, 41943040, 524288)}),
    ("bf16", 64, 128, 128, {"proj": 1}, {FUSED: (1, 50331648, 557056)}),
]


def _case_id(c):
    return "%s_dh%d_%dx%d%s" % (c[0], c[1], c[2], c[3], "".join("_%s" % (v if isinstance(v, str) else k) for k, v in sorted(c[4].items())))


def _rows_of(fn):
    """imt_prof_report rows of the launches of fn(), as {kind: (launches, flops, bytes)}."""
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
    return {rows[i].kind.decode(): (int(rows[i].launches), rows[i].flops, rows[i].bytes) for i in range(n)}


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_attention_bwd_dispatch(cuda, case):
    from imagetranslate_amd import hip_ops as O
    dtype_name, dh, Tq, Tk, opt, want = case
    dtype = {"bf16": torch.bfloat16, "f32": torch.float32}[dtype_name]
    g = torch.Generator().manual_seed(100 * Tq + Tk + dh)
    d = H * dh

    def mk(rows, scale=0.8):
        return (torch.randn(rows, d, generator=g) * scale).to(dtype).cuda()

    q, k, v, do = mk(B * Tq), mk(B * Tk), mk(B * Tk), mk(B * Tq)
    kw = {}
    if "mask3d" in opt:
        kw["mask3d"] = (torch.rand(B, Tq, Tk, generator=g) > 0.3).to(torch.uint8).cuda()
    o, lse = O.attention_fwd(q, k, v, B, H, Tq, Tk, dh, **kw)
    if "proj" in opt:
        w_o = mk(d, 0.06)
        call = lambda: O.attention_bwd_proj(do, w_o, q, k, v, o, lse, B, H, Tq, Tk, dh)
    else:
        call = lambda: O.attention_bwd(do, q, k, v, o, lse, B, H, Tq, Tk, dh, **kw)
    switches = ("IMT_ATTN_NO_FUSED_BWD", "IMT_ATTN_NO_FUSED256")
    for s in switches:
        os.environ.pop(s, None)
    if "env" in opt:
        os.environ[opt["env"]] = "1"
    try:
        got = _rows_of(call)
    finally:
        for s in switches:
            os.environ.pop(s, None)
    print("dispatch %s -> %s" % (_case_id(case), sorted(got.items())))
    assert got == want, (_case_id(case), got, want)
