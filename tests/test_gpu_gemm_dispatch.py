"""Which kernel imt_gemm / imt_gemm_grouped_tn launch for a shape: one row per threshold of the host-side policy in
csrc/gemm.hip (tile counts, K lengths, epilogue options, split-K workspace, forced variants, the share-CUs knob).

The expected kinds were recorded from the library BEFORE the policy was split into validate / plan / run; they pin the
dispatch, not the numerics (those stay with test_gpu_ops.py / test_gpu_c1.py).  Operands are views of one shared pool of
random bf16 numbers -- only the shapes matter here."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LN = "layernorm_fwd"  # the LayerNorm launch behind a GEMM that cannot normalise in its own launch


def _kinds_of(fn):
    """Kernel kinds (imt_prof_report rows) launched by fn(), as {kind: launches}."""
    from imagetranslate_amd import _lib as L
    lib = L.load()
    torch.cuda.synchronize()
    lib.imt_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        rows = (L.ProfRow * 256)()
        n = lib.imt_prof_report(rows, 256)
    finally:
        lib.imt_prof_enable(0)
    return {rows[i].kind.decode(): int(rows[i].launches) for i in range(n)}


@pytest.fixture(scope="module")
def pool(cuda):
    g = torch.Generator(device=cuda).manual_seed(5)
    return torch.randn(2048 * 65792, device=cuda, dtype=torch.bfloat16, generator=g)


def _view(pool, rows, cols):
    return pool[: rows * cols].view(rows, cols)


def _operands(pool, layout, M, N, K):
    from imagetranslate_amd import hip_ops as O
    if layout == O.IMT_NT:
        return _view(pool, M, K), _view(pool, N, K)
    if layout == O.IMT_NN:
        return _view(pool, M, K), _view(pool, K, N)
    return _view(pool, K, M), _view(pool, K, N)


# (layout, M, N, K, options, expected kinds).  options: resid / gelu / ln / ws (split-K workspace) / colsum / share (share-CUs
# knob) / force (imt_gemm_args.force_general) / split_k / slabs (IMT_AUX_SPLITK_WS with that many splits) / refused (the call
# fails with this message after the launches listed)
CASES = [
    ("NT", 256, 256, 968, {}, ["gemm_sbuf_bf16_nt"]),
    ("NT", 256, 256, 1032, {}, ["gemm_sbuf_bf16_nt", "gemm_ws_bf16_nt"]),
    ("NT", 256, 256, 64, {}, ["gemm_sbuf_bf16_nt"]),
    ("TN", 256, 256, 64, {}, ["gemm_dbuf_bf16_tn"]),
    ("NT", 2048, 2048, 128, {}, ["gemm_ws_bf16_nt"]),
    ("NT", 2048, 2048, 128, {"share": 1}, ["gemm_sbuf_bf16_nt"]),
    ("NT", 2048, 2048, 1024, {"share": 1}, ["gemm_ws_bf16_nt"]),
    ("NT", 2048, 1536, 128, {"share": 1}, ["gemm_ws_bf16_nt"]),
    ("NT", 32896, 128, 128, {}, ["gemm_sbuf_bf16_nt"]),
    ("NT", 32896, 128, 960, {}, ["gemm_sbuf_bf16_nt"]),
    ("NT", 32896, 128, 1024, {}, ["gemm_ws_bf16_nt"]),
    ("TN", 32896, 128, 128, {}, ["gemm_ws_bf16_tn"]),
    ("NT", 18688, 1792, 128, {}, ["gemm_sbuf_bf16_nt"]),
    ("NT", 16384, 2048, 128, {}, ["gemm_xl_bf16_nt"]),
    ("NT", 16384, 2048, 1024, {}, ["gemm_ws_bf16_nt"]),
    ("NT", 57088, 256, 128, {"resid": 1}, ["gemm_sbuf_bf16_nt"]),
    ("NT", 8192, 1792, 128, {"resid": 1}, ["gemm_xl_bf16_nt"]),
    ("NT", 8192, 1792, 128, {"gelu": 1}, ["gemm_xl_bf16_nt"]),
    ("NT", 8192, 1792, 128, {}, ["gemm_sbuf_bf16_nt"]),
    ("TN", 4096, 3584, 2048, {}, ["gemm_xl_bf16_tn"]),
    ("TN", 4096, 3584, 2048, {"colsum": 1}, ["gemm_xl_bf16_tn"]),
    ("TN", 4096, 3584, 1984, {}, ["gemm_ws_bf16_tn"]),
    ("TN", 4096, 4096, 2048, {}, ["gemm_xl_bf16_tn"]),
    ("TN", 57088, 256, 2048, {}, ["gemm_ws_bf16_tn"]),
    ("TN", 65792, 256, 2048, {}, ["gemm_ws_bf16_tn"]),
    ("NT", 1024, 2048, 1024, {"ws": 1}, ["gemm_ws_bf16_nt", "gemm_splitk_epilogue"]),
    ("NT", 5504, 384, 1024, {"ws": 1}, ["gemm_ws_bf16_nt"]),
    ("NT", 1024, 2048, 960, {"ws": 1}, ["gemm_ws_bf16_nt"]),
    ("NT", 1024, 512, 512, {"ws": 1, "resid": 1, "ln": 1}, ["gemm_ws_bf16_nt", "gemm_splitk_epilogue_ln"]),
    ("NT", 1024, 512, 448, {"ws": 1, "resid": 1, "ln": 1}, ["gemm_ws_bf16_nt", LN]),
    ("NT", 1152, 512, 512, {"ws": 1, "resid": 1, "ln": 1}, ["gemm_ws_bf16_nt", LN]),
    # N > 1024: the epilogue launch does not normalise, and the LayerNorm launch behind it is called but refuses rows that long
    ("NT", 320, 1152, 1024, {"ws": 1, "resid": 1, "ln": 1, "refused": "layernorm: d=1152 > 1024"}, ["gemm_ws_bf16_nt", "gemm_splitk_epilogue"]),
    ("NT", 320, 512, 2048, {"ws": 1, "resid": 1, "ln": 1}, ["gemm_ws_bf16_nt", "gemm_splitk_epilogue_ln"]),
    ("TN", 256, 256, 1024, {"split_k": 4}, ["gemm_dbuf_bf16_tn"]),
    ("NT", 512, 512, 136, {"force": 6}, ["gemm_sbuf_bf16_nt"]),
    ("NT", 512, 512, 64, {"force": 2}, ["gemm_dbuf_bf16_nt"]),
    ("NT", 512, 512, 256, {"force": 4}, ["gemm_dbuf_bf16_nt"]),
    ("NN", 512, 512, 4104, {"slabs": 4}, ["gemm_sbuf_bf16_nn", "gemm_xl_bf16_nn", "gemm_splitk_reduce"]),
]


def _case_id(c):
    return "%s_%dx%dx%d%s" % (c[0], c[1], c[2], c[3], "".join("_%s%s" % (k, v if isinstance(v, int) and v != 1 else "") for k, v in sorted(c[4].items())))


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_gemm_dispatch(cuda, pool, case):
    from imagetranslate_amd import _lib as L
    from imagetranslate_amd import hip_ops as O
    name, M, N, K, opt, expected = case
    layout = {"NT": O.IMT_NT, "NN": O.IMT_NN, "TN": O.IMT_TN}[name]
    A, B = _operands(pool, layout, M, N, K)
    bf16, f32 = torch.bfloat16, torch.float32
    kw = {}
    if "resid" in opt:
        kw["resid"] = _view(pool, M, N)
    if "gelu" in opt:
        kw.update(aux=torch.empty(M, N, device=cuda, dtype=bf16), aux_mode=O.IMT_AUX_GELU_FWD)
    if "ws" in opt:
        kw["splitk_ws"] = O.splitk_workspace(cuda)
    if "ln" in opt:
        kw["ln"] = dict(gamma=torch.ones(N, device=cuda, dtype=bf16), beta=torch.zeros(N, device=cuda, dtype=bf16),
                        out=torch.empty(M, N, device=cuda, dtype=bf16), mean=torch.empty(M, device=cuda, dtype=f32),
                        rstd=torch.empty(M, device=cuda, dtype=f32),
                        tickets=torch.zeros((M + 127) // 128, device=cuda, dtype=torch.int32), eps=1e-12)
    if "colsum" in opt:  # the weight-gradient form: fp32 gradient accumulated in place, bias gradient beside it
        kw.update(out=torch.zeros(M, N, device=cuda, dtype=f32), accumulate=True, a_colsum=torch.zeros(M, device=cuda, dtype=f32))
    if "split_k" in opt:
        kw.update(out=torch.zeros(M, N, device=cuda, dtype=f32), split_k=opt["split_k"])
    if "slabs" in opt:
        kw.update(out=torch.empty(M, N, device=cuda, dtype=bf16), aux=torch.empty(opt["slabs"] * M, N, device=cuda, dtype=f32),
                  aux_mode=O.IMT_AUX_SPLITK_WS, split_k=opt["slabs"])
    if "force" in opt:
        kw["force_general"] = opt["force"]
    errors = []

    def call():
        try:
            O.gemm(A, B, layout, **kw)
        except L.ImtError as e:
            errors.append(str(e))

    lib = L.load()
    prev = lib.imt_set_gemm_share_cus(opt.get("share", 0))
    try:
        kinds = _kinds_of(call)
    finally:
        lib.imt_set_gemm_share_cus(prev)
    if "refused" in opt:
        assert len(errors) == 1 and opt["refused"] in errors[0], errors
    else:
        assert not errors, errors
    want = {}
    for k in expected:
        want[k] = want.get(k, 0) + 1
    print("dispatch %s -> %s" % (_case_id(case), sorted(kinds.items())))
    assert kinds == want, (_case_id(case), kinds, want)


def _grouped(pool, cuda, shapes):
    return [dict(A=_view(pool, K, M), B=_view(pool, K, N), out=torch.zeros(M, N, device=cuda, dtype=torch.float32)) for (M, N, K) in shapes]


def test_grouped_dispatch_one_launch(cuda, pool):
    """A groupable list of weight gradients is one launch of the grouped kernel."""
    from imagetranslate_amd import hip_ops as O
    problems = _grouped(pool, cuda, [(256, 256, 256), (512, 128, 256), (128, 384, 256), (256, 128, 256)])
    kinds = _kinds_of(lambda: O.gemm_grouped_tn(problems))
    print("dispatch grouped4 -> %s" % sorted(kinds.items()))
    assert kinds == {"gemm_bf16_tn_grouped": 1}, kinds


def test_grouped_dispatch_too_many_tiles(cuda, pool):
    """More than 640 output tiles in the list (2 x 26 x 13 = 676): every member goes through imt_gemm on its own."""
    from imagetranslate_amd import hip_ops as O
    problems = _grouped(pool, cuda, [(3328, 1664, 128), (3328, 1664, 128)])
    kinds = _kinds_of(lambda: O.gemm_grouped_tn(problems))
    print("dispatch grouped>640 -> %s" % sorted(kinds.items()))
    assert kinds == {"gemm_ws_bf16_tn": 2}, kinds
