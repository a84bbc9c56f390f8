"""csrc/objects.hip kernel by kernel, and the two entry points of csrc/pool.hip that were run at one shape (imt_contrastive,
imt_l2_dist), at the sizes where their loops wrap, their row chunks repeat and their launch caps bind -- through the C ABI, on
given inputs (no GEMM in front), fp32 and bf16, element by element against fp64.  tests/test_gpu_object_stream.py reaches these
kernels through ImageHead.objects_forward at d = 128 / 512 and 111 rows, by ``max|a-b| / max|b|`` at 2.5e-2.

Bounds.  Copies are bit-exact.  A value that is one rounding of an exact result is held to one ulp of the output dtype
(2^-23 / 2^-7 of its magnitude).  A sum is held to ``tol x (sum of the magnitudes of its terms)``, where ``tol`` is computed in
the test as in tests/test_gpu_row_edges.py: 16 x the worst ``|error| / magnitude`` of the same formula evaluated in plain fp32
torch on the CPU against fp64, over all outputs of the case, capped at 1e-5; bf16 outputs get one bf16 ulp on top.  Every output
has a sentinel row (four sentinel elements for vectors) that must come back bit-unchanged.  Each check prints its worst
error / bound before it asserts (``ROWEDGE <case> <what> <ratio>``, pytest -s); DESIGN.md, "Batch and object-stream edge tests",
lists case -> path reached -> measured ratio."""
import functools

import pytest
import torch

from tests import caption2image_oracle as C
from tests import multimodal_oracle as M
from tests.object_stream_oracle import object_rows
from tests.test_gpu_object_stream import _keep_mask
from tests.test_gpu_row_edges import BF16, BF16_ULP, DTYPES, F32, SENT, Guarded, _bits_equal, _name, _within

pytestmark = pytest.mark.gpu

ULP = {F32: 2.0 ** -23, BF16: BF16_ULP}   # an upper bound of ulp(x) / |x| in either format
FEAT, LABELS, PARTS = 1024, 91, 64


def _ops():
    from imagetranslate_amd import hip_ops as O
    from imagetranslate_amd import _lib as L
    return O, L, L.load()


def _tol(pairs, what):
    """16 x the worst |fp32 CPU value - fp64 value| / magnitude over the (value32, value64, magnitude) triples, capped at 1e-5."""
    worst = 0.0
    for v32, v64, mag in pairs:
        nz = mag > 0
        if bool(nz.any()):
            worst = max(worst, float(((v32.double() - v64).abs()[nz] / mag[nz]).max()))
    tol = min(16.0 * worst, 1e-5)
    print("ROWEDGE %s fp32-cpu-worst %.3e tol %.3e" % (what, worst, tol))
    return tol


def _out_bound(tol, mag, ref, dtype):
    return tol * mag + (BF16_ULP * ref.abs() if dtype == BF16 else 0.0)


# ------------------------------------------------------------------------------------------------ obj_rows
OBJ_D = [4, 260, 1028]                                   # Kp 1088 / 1344 / 2112; 260 and 1028: d % 256 = 4, all three boundaries inside a trip
OBJ_R = ["R1", "R5", "R0w", "R0"]
OBJ_TYPES = [(F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32)]   # (feature dtype, compute dtype)


def _locs_bound(boxes, live, t):
    """Bound of the seven locs against object_rows in fp64.  The four quotients are one rounding of an exact value each: one
    ulp of the output dtype of their own magnitude, as the contract of the test asks.  w = x2/800 - x1/800 subtracts two
    quotients already ROUNDED to fp32 (src/image_model.py:61-69 does the same), so it carries half an fp32 ulp of each operand
    whatever the output dtype, h likewise and w * h both: the only departure from "one ulp of the output" is that fp32-level
    term, 2^-23 x the operands' magnitudes.  A bf16 output is the fp32 value rounded once: one bf16 ulp of the VALUE on top
    (in fp32 the value's own rounding is inside the operand term, since |w| <= |x1| + |x2|).  A narrow box keeps a bound far
    below its width: subtracting quotients rounded to bf16, or storing 0, does not pass."""
    x1, y1, x2, y2 = (boxes.double()[:, i] / 800 for i in range(4))
    wd, ht = x2 - x1, y2 - y1
    sx, sy = x1.abs() + x2.abs(), y1.abs() + y2.abs()
    quot = ULP[t] * torch.stack([x1.abs(), x2.abs(), y1.abs(), y2.abs()], -1)
    operands = ULP[F32] * torch.stack([sx, sy, ht.abs() * sx + wd.abs() * sy + (wd * ht).abs()], -1)
    own = (ULP[BF16] if t == BF16 else 0.0) * torch.stack([wd.abs(), ht.abs(), (wd * ht).abs()], -1)
    return torch.cat([quot, operands + own], -1) * live.unsqueeze(-1)


@pytest.mark.parametrize("tf,t", OBJ_TYPES, ids=["f32", "bf16", "f32feat-bf16", "bf16feat-f32"])
def test_obj_rows_locs_of_many_boxes(cuda, tf, t):
    """67 live rows (17 blocks of 4, the last with three), half of them narrow boxes (w, h below 8 of 800 at x, y up to 600):
    the rows on which the bound of the differences is far below one ulp of the operands in bf16."""
    O, L, lib = _ops()
    R, d = 67, 4
    K, Kp = d + FEAT + 7, O.obj_padded_k(d)
    tag = "obj_rows-locs-R67-%s/%s" % (_name(tf), _name(t))
    g = torch.Generator().manual_seed(167)
    labels = torch.randint(1, LABELS, (R,), generator=g)
    feats = torch.randn(R, FEAT, generator=g).to(tf)
    xy, wh = torch.rand(R, 2, generator=g) * 600, torch.rand(R, 2, generator=g) * 200
    wh[::2] = wh[::2] * 0.04
    boxes = torch.cat([xy, xy + wh], -1)
    emb = torch.randn(LABELS, d, generator=g).to(t)
    w = torch.randn(d, K, generator=g).to(t)
    live = torch.ones(R, dtype=torch.bool)
    bound = _locs_bound(boxes, live, t)
    ref = object_rows(emb.double(), labels, feats.double(), boxes.double())
    narrow = ref[::2, d + FEAT + 4]
    if t == BF16:   # what the bound must exclude on the narrow rows: a width of 0, and the difference of bf16-rounded quotients
        q = (boxes.double() / 800).to(BF16).double()
        assert bool((narrow.abs() > 4 * bound[::2, 4]).all())
        assert float(((q[::2, 2] - q[::2, 0] - narrow).abs() / bound[::2, 4]).max()) > 10.0
    x_out = Guarded(R, Kp, t, cuda, ld=Kp)
    lab_d, feat_d, box_d, emb_d, w_d = (v.to(cuda) for v in (labels, feats, boxes, emb, w))   # held until the results are read
    L.check(lib.imt_obj_rows(O.dt(feats), O.dt(emb), O._p(lab_d), O._p(feat_d), O._p(box_d), O._p(emb_d), O._p(w_d), O._p(x_out.full),
                             None, R, d, Kp, None, O._stream()), "imt_obj_rows")
    x_out.check(tag)
    x = x_out.view.cpu()
    assert _bits_equal(x[:, :d], emb[labels])
    assert float(x[:, K:].float().abs().max()) == 0.0
    _within(x[:, d + FEAT:K], ref[:, d + FEAT:K], bound, tag)


@pytest.mark.parametrize("tf,t", OBJ_TYPES, ids=["f32", "bf16", "f32feat-bf16", "bf16feat-f32"])
@pytest.mark.parametrize("rcase", OBJ_R)
@pytest.mark.parametrize("d", OBJ_D)
def test_obj_rows(cuda, d, rcase, tf, t):
    O, L, lib = _ops()
    K, Kp = d + FEAT + 7, O.obj_padded_k(d)
    assert Kp == {4: 1088, 260: 1344, 1028: 2112}[d] and Kp > K
    R = {"R1": 1, "R5": 5, "R0w": 0, "R0": 0}[rcase]
    want_w = rcase in ("R5", "R0w")
    tag = "obj_rows-d%d-%s-%s/%s" % (d, rcase, _name(tf), _name(t))
    g = torch.Generator().manual_seed(100 + d + R)
    labels = torch.tensor([0, 90, -1, 91, 37][:R] if R == 5 else [13][:R], dtype=torch.int64)
    feats = torch.randn(R, FEAT, generator=g).to(tf)
    xy, wh = torch.rand(R, 2, generator=g) * 600, torch.rand(R, 2, generator=g) * 200
    boxes = torch.cat([xy, xy + wh], -1)
    if R == 5:
        boxes[1] = torch.tensor([100.0, 50.0, 300.0, 200.0])   # multiples of 800 / 256: every loc is exact in both formats
    emb = torch.randn(LABELS, d, generator=g).to(t)
    w = torch.randn(d, K, generator=g).to(t)
    x_out, w_out = Guarded(R, Kp, t, cuda, ld=Kp), Guarded(d, Kp, t, cuda, ld=Kp)
    status = Guarded(1, None, torch.int32, cuda)
    status.view.zero_()
    dev = lambda v: v.to(cuda) if v.numel() else torch.zeros(4, dtype=v.dtype, device=cuda)  # noqa: E731  (an empty tensor has no address)
    lab_d, feat_d, box_d, emb_d, w_d = dev(labels), dev(feats), dev(boxes), dev(emb), dev(w)

    def call(x_buf, status_ptr):
        L.check(lib.imt_obj_rows(O.dt(feats), O.dt(emb), O._p(lab_d), O._p(feat_d), O._p(box_d), O._p(emb_d), O._p(w_d), O._p(x_buf.full),
                                 O._p(w_out.full) if want_w else None, R, d, Kp, status_ptr, O._stream()), "imt_obj_rows")
    call(x_out, O._p(status.view))
    x_out.check(tag + " x")
    w_out.check(tag + " w_pad")
    status.check(tag + " status")
    assert int(status.view.cpu()) == (1 if R == 5 else 0), "the status word flags labels outside [0, 91) and nothing else"
    if want_w:
        wp = w_out.view.cpu()
        assert _bits_equal(wp[:, :K], w), tag + ": weight copy"
        assert float(wp[:, K:].float().abs().max()) == 0.0, tag + ": pad columns of the weight copy"
    else:
        assert bool((w_out.full.float().cpu() == float(torch.tensor(SENT, dtype=t).float())).all()), tag + ": w_out written without being asked"
    if R == 0:
        return
    x = x_out.view.cpu()
    live = (labels > 0) & (labels < LABELS)
    assert float(x[:, K:].float().abs().max()) == 0.0, tag + ": pad columns K..Kp"
    assert float(x[~live].float().abs().max() if bool((~live).any()) else 0.0) == 0.0, tag + ": zeroed rows"
    assert _bits_equal(x[live][:, :d], emb[labels[live]]), tag + ": embedding columns"
    if tf == t or t == F32:    # same format, or bf16 features widened to fp32: a copy
        assert _bits_equal(x[live][:, d:d + FEAT], feats[live].to(t)), tag + ": feature columns"
    else:                      # fp32 features rounded to bf16 once
        f64 = feats[live].double()
        _within(x[live][:, d:d + FEAT], f64, ULP[t] * f64.abs(), tag + " features")
    safe = torch.where(live, labels, torch.zeros_like(labels))
    ref = object_rows(emb.double(), safe, feats.double(), boxes.double())
    _within(x[:, d + FEAT:K], ref[:, d + FEAT:K], _locs_bound(boxes, live, t), tag + " locs")
    if R == 5:   # the row on the 1 / 256 grid: exact
        assert _bits_equal(x[1, d + FEAT:K], torch.tensor([0.125, 0.375, 0.0625, 0.25, 0.25, 0.1875, 0.046875]).to(t)), tag + ": exact locs"
        again = Guarded(R, Kp, t, cuda, ld=Kp)
        call(again, None)      # status = NULL: the same rows, nothing to flag
        again.check(tag + " x (status NULL)")
        assert _bits_equal(again.view.cpu(), x)


# ------------------------------------------------------------------------------------------------ relu_dropout
DROP_SEED = (3 << 32) | 9


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("d", [4, 260, 516])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_relu_dropout_fwd_bwd(cuda, dtype, d, p):
    O, L, lib = _ops()
    rows = 5
    tag = "relu_dropout-%s-5x%d-p%g" % (_name(dtype), d, p)
    g = torch.Generator().manual_seed(200 + d)
    z = torch.randn(rows, d, generator=g).to(dtype)
    flat = z.view(-1)
    flat[0::7], flat[3::11] = 0.0, -0.0          # exact zeros of both signs among positives and negatives
    assert bool((z < 0).any()) and bool((z > 0).any()) and bool((z == 0).any())
    keep = _keep_mask(DROP_SEED, rows * d, p).view(rows, d) if p > 0 else torch.ones(rows, d, dtype=torch.bool)
    pos = z.double() > 0
    y = Guarded(rows, d, dtype, cuda, ld=d)
    y.view.copy_(z)
    L.check(lib.imt_relu_dropout(O.dt(z), O._p(y.view), rows, d, p, DROP_SEED, O._stream()), "imt_relu_dropout")
    y.check(tag + " y")
    got = y.view.cpu()
    assert torch.equal(got != 0, pos & keep), tag + ": the kept set is not keep(seed, r * d + c) on the positive inputs"
    ref = torch.where(pos & keep, z.double(), torch.zeros(rows, d, dtype=torch.float64)) / (1 - p)
    if p == 0:
        assert _bits_equal(got, torch.where(pos, z, torch.zeros_like(z))), tag + ": relu alone must copy (and write +0 elsewhere)"
    _within(got, ref, ULP[dtype] * ref.abs(), tag + " y")
    dy = torch.randn(rows, d, generator=g).to(dtype)
    dz = Guarded(rows, d, dtype, cuda, ld=d)
    dyd = dy.to(cuda)
    L.check(lib.imt_relu_dropout_bwd(O.dt(z), O._p(dyd), O._p(y.view), O._p(dz.view), rows, d, p, DROP_SEED, O._stream()),
            "imt_relu_dropout_bwd")
    dz.check(tag + " dz")
    y.check(tag + " y after the backward")
    assert _bits_equal(y.view.cpu(), got), "the saved output is an input of the backward"
    dref = torch.where(pos & keep, dy.double(), torch.zeros(rows, d, dtype=torch.float64)) / (1 - p)
    gz = dz.view.cpu()
    assert float(gz[~(pos & keep)].float().abs().max()) == 0.0, tag + ": gradient where y <= 0 or the element was dropped"
    _within(gz, dref, ULP[dtype] * dref.abs(), tag + " dz")


# ------------------------------------------------------------------------------------------------ obj_fold_w
@pytest.mark.parametrize("d", [4, 260])
def test_obj_fold_w(cuda, d):
    O, L, lib = _ops()
    K, Kp = d + FEAT + 7, O.obj_padded_k(d)
    g = torch.Generator().manual_seed(300 + d)
    dw = torch.randn(d, Kp, generator=g)
    dw[:, K:] = 1e30                                  # a pad column folded in would show at once
    init = torch.randn(d * K, generator=g)
    grad = Guarded(d * K, None, F32, cuda)
    grad.view.copy_(init)
    dw_d = dw.to(cuda)
    L.check(lib.imt_obj_fold_w(O._p(dw_d), O._p(grad.view), d, Kp, O._stream()), "imt_obj_fold_w")
    grad.check("obj_fold_w d=%d" % d)
    assert _bits_equal(grad.view.cpu(), init + dw[:, :K].reshape(-1)), "grad += dw_pad[:, :K] is one fp32 addition per element"


# ------------------------------------------------------------------------------------------------ obj_embed_grad
EMB_R, EMB_D = [1, 256, 257, 700], [4, 260, 1028, 4096]


@functools.lru_cache(maxsize=None)
def _embed_grad_case(R, d, dtype, one_label):
    """Inputs (CPU, rounded to dtype), fp64 reference, magnitudes and tol of one obj_embed_grad case; shared, never modified."""
    g = torch.Generator().manual_seed(400 + R + d)
    labels = torch.randint(0, LABELS, (R,), generator=g)
    if one_label:
        labels.fill_(37)
    elif R == 1:
        labels[0] = 90
    else:
        labels[0], labels[1], labels[R - 1] = 0, 90, 55   # the last row (row 256 of R = 257, alone in its chunk) is live
    dx = torch.randn(R, d, generator=g).to(dtype)
    init = torch.randn(LABELS, d, generator=g)
    live = labels != 0
    ref = init.double().index_add(0, labels[live], dx.double()[live])
    mag = init.double().abs().index_add(0, labels[live], dx.double().abs()[live])
    g32 = init.clone().index_add_(0, labels[live], dx.float()[live])
    tag = "obj_embed_grad-%s-R%d-d%d%s" % (_name(dtype), R, d, "-one-label" if one_label else "")
    return dict(labels=labels, dx=dx, init=init, ref=ref, mag=mag, tol=_tol([(g32, ref, mag)], tag), tag=tag)


def _run_embed_grad(c, R, d, dev):
    O, L, lib = _ops()
    wide = torch.full((R, d + 8), 1e30, dtype=c["dx"].dtype, device=dev)   # ldx = d + 8: columns past d are never summed
    dxv = wide[:, :d]
    dxv.copy_(c["dx"])
    lab = c["labels"].to(dev)
    outs = []
    for _ in range(2):
        grad = Guarded(LABELS, d, F32, dev, ld=d)
        grad.view.copy_(c["init"])
        L.check(lib.imt_obj_embed_grad(O.dt(dxv), O._p(lab), O._p(dxv), dxv.stride(0), O._p(grad.view), R, d, O._stream()),
                "imt_obj_embed_grad")
        grad.check(c["tag"])
        outs.append(grad.view.cpu())
    assert _bits_equal(outs[0], outs[1]), c["tag"] + ": two calls on the same input differ"
    assert _bits_equal(outs[0][0], c["init"][0]), c["tag"] + ": label 0 takes no gradient"
    _within(outs[0], c["ref"], c["tol"] * c["mag"], c["tag"])


@pytest.mark.parametrize("d", EMB_D)
@pytest.mark.parametrize("R", EMB_R)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_obj_embed_grad(cuda, dtype, R, d):
    c = _embed_grad_case(R, d, dtype, False)
    if R > 1:
        assert bool((c["labels"] == 0).any()) and bool((c["labels"] == 90).any())
    if R == 257:   # row 256 is the second chunk: dropping it must leave an error far above the bound somewhere
        lab = int(c["labels"][256])
        assert lab != 0 and float((c["dx"][256].double().abs() / (c["tol"] * c["mag"][lab])).max()) > 100.0
    _run_embed_grad(c, R, d, cuda)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_obj_embed_grad_one_label(cuda, dtype):
    """All 256 rows carry label 37: four full 64-bit ballots, every set bit walked; the other 89 workgroups add nothing."""
    c = _embed_grad_case(256, 260, dtype, True)
    _run_embed_grad(c, 256, 260, cuda)


# ------------------------------------------------------------------------------------------------ gated_mix_bwd
@functools.lru_cache(maxsize=None)
def _gated_case(rows, d, dtype):
    g = torch.Generator().manual_seed(500 + rows + d)
    dy, a, b = (torch.randn(rows, d, generator=g).to(dtype) for _ in range(3))
    gate = torch.randn(d, generator=g).to(dtype)
    init = torch.randn(d, generator=g)
    tag = "gated_mix_bwd-%s-%dx%d" % (_name(dtype), rows, d)

    def evaluate(cast):
        s = torch.sigmoid(cast(gate) + 1e-7)
        dyc, ac, bc = cast(dy), cast(a), cast(b)
        return s * dyc, (1 - s) * dyc, cast(init) + (dyc * (ac - bc) * s * (1 - s)).sum(0), s
    da, db, dg, s = evaluate(lambda v: v.double())
    da32, db32, dg32, _ = evaluate(lambda v: v.float())
    dyd = dy.double().abs()
    # db = dy - s dy and s (1 - s) = s - s^2 are differences: their terms are what the bound scales with
    m_da, m_db = da.abs(), dyd + (s * dyd)
    m_dg = init.double().abs() + (dyd * (a.double().abs() + b.double().abs()) * (s + s * s)).sum(0)
    tol = _tol([(da32, da, m_da), (db32, db, m_db), (dg32, dg, m_dg)], tag)
    return dict(dy=dy, a=a, b=b, gate=gate, init=init, da=da, db=db, dg=dg, m_da=m_da, m_db=m_db, m_dg=m_dg, tol=tol, tag=tag)


@pytest.mark.parametrize("d", [4, 260, 1028, 2048])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 301])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_gated_mix_bwd(cuda, dtype, rows, d):
    O, L, lib = _ops()
    c = _gated_case(rows, d, dtype)
    tag = c["tag"]
    dyd, ad, bd, gd = (c[k].to(cuda) for k in ("dy", "a", "b", "gate"))
    outs = []
    for _ in range(2):
        da, db = Guarded(rows, d, dtype, cuda, ld=d), Guarded(rows, d, dtype, cuda, ld=d)
        dgate, ws = Guarded(d, None, F32, cuda), Guarded(PARTS * d, None, F32, cuda)
        dgate.view.copy_(c["init"])
        L.check(lib.imt_gated_mix_bwd(O.dt(ad), O._p(dyd), O._p(ad), O._p(bd), O._p(gd), O._p(da.view), O._p(db.view), O._p(dgate.view),
                                      O._p(ws.view), rows, d, O._stream()), "imt_gated_mix_bwd")
        for buf, what in ((da, "da"), (db, "db"), (dgate, "dgate"), (ws, "workspace")):
            buf.check(tag + " " + what)
        outs.append((da.view.cpu(), db.view.cpu(), dgate.view.cpu()))
    assert all(_bits_equal(x, y) for x, y in zip(*outs)), tag + ": two calls on the same input differ"
    _within(outs[0][0], c["da"], _out_bound(c["tol"], c["m_da"], c["da"], dtype), tag + " da")
    _within(outs[0][1], c["db"], _out_bound(c["tol"], c["m_db"], c["db"], dtype), tag + " db")
    _within(outs[0][2], c["dg"], c["tol"] * c["m_dg"], tag + " dgate")


# ------------------------------------------------------------------------------------------------ pool.hip: imt_contrastive
@functools.lru_cache(maxsize=None)
def _contrastive_case(B, N, d):
    g = torch.Generator().manual_seed(600 + N)
    img = torch.nn.functional.normalize(torch.randn(B, d, generator=g), dim=-1)
    txt = torch.nn.functional.normalize(torch.randn(N, d, generator=g) + 0.5 * torch.randn(1, d, generator=g), dim=-1)
    i64, t64 = img.double(), txt.double()
    loss, (g_img, g_txt) = M.contrastive(i64, t64).view(1), M.contrastive_grads(i64, t64)
    loss32, (g_img32, g_txt32) = M.contrastive(img, txt).view(1), M.contrastive_grads(img, txt)
    # magnitudes: C_ij = sum_k |img_ik txt_jk|; dC_ij = (p_ij - [i == j]) / B is a difference on the diagonal
    cross = i64 @ t64.t()
    e = torch.exp(cross)
    den = e.sum(-1, keepdim=True) + 1e-4
    p = e / den
    mag_c = i64.abs() @ t64.abs().t()
    m_dc = p.clone()
    m_dc[:, :B] += torch.eye(B, dtype=torch.float64)
    m_dc = m_dc / B
    m_loss = ((torch.log(den).abs().view(-1) + (p * mag_c).sum(-1) + torch.diagonal(mag_c[:, :B]) + 1e-4).sum() / B).view(1)
    m_img, m_txt = m_dc @ t64.abs(), m_dc.t() @ i64.abs()
    tag = "contrastive-B%d-N%d-d%d" % (B, N, d)
    tol = _tol([(loss32, loss, m_loss), (g_img32, g_img, m_img), (g_txt32, g_txt, m_txt)], tag)
    return dict(img=img, txt=txt, loss=loss, g_img=g_img, g_txt=g_txt, m_loss=m_loss, m_img=m_img, m_txt=m_txt, tol=tol, tag=tag)


@pytest.mark.parametrize("B,N,d", [(1, 1, 4), (3, 300, 12), (4, 263, 1024), (2, 4096, 64)])
def test_contrastive(cuda, B, N, d):
    O, L, lib = _ops()
    c = _contrastive_case(B, N, d)
    tag = c["tag"]
    img, txt = c["img"].to(cuda), c["txt"].to(cuda)
    outs = []
    for _ in range(2):
        loss, ws = Guarded(1, None, F32, cuda), Guarded(B * N + B, None, F32, cuda)
        d_img, d_txt = Guarded(B, d, F32, cuda, ld=d), Guarded(N, d, F32, cuda, ld=d)
        L.check(lib.imt_contrastive(O._p(img), O._p(txt), O._p(loss.view), O._p(d_img.view), O._p(d_txt.view), O._p(ws.view), B, N, d,
                                    O._stream()), "imt_contrastive")
        for buf, what in ((loss, "loss"), (ws, "workspace"), (d_img, "d_img"), (d_txt, "d_txt")):
            buf.check(tag + " " + what)
        outs.append((loss.view.cpu(), d_img.view.cpu(), d_txt.view.cpu()))
    assert all(_bits_equal(x, y) for x, y in zip(*outs)), tag + ": two calls on the same input differ"
    _within(outs[0][0], c["loss"], c["tol"] * c["m_loss"], tag + " loss")
    _within(outs[0][1], c["g_img"], c["tol"] * c["m_img"], tag + " d_img")
    _within(outs[0][2], c["g_txt"], c["tol"] * c["m_txt"], tag + " d_txt")


# ------------------------------------------------------------------------------------------------ pool.hip: imt_l2_dist
# n4 = B * n / 4 groups of four: 1 (one workgroup, one live thread); 65536 = 256 x 256 (wgs == IMT_L2_DIST_PARTS: every part one
# trip); 65537 (wgs = 257 > 256 parts: thread 0 of part 0 takes the first second trip); 2048 * 256 + 1 (the second launch's cap of
# 2048 workgroups binds: its first second trip)
L2_CASES = [(1, 4), (4, 65536), (1, 4 * 65537), (3, 4 * 174763)]


@functools.lru_cache(maxsize=None)
def _l2_case(B, n, dtype):
    g = torch.Generator().manual_seed(700 + B + n % 1000)
    pred = torch.randn(B, n, generator=g).to(dtype)
    target = (torch.randn(B, n, generator=g) * 0.5 + 0.1).to(dtype)
    p64, t64 = pred.double(), target.double()
    loss, grad = C.l2_dist(p64, t64).view(1), C.l2_dist_grad(p64, t64)
    loss32, grad32 = C.l2_dist(pred.float(), target.float()).view(1), C.l2_dist_grad(pred.float(), target.float())
    tag = "l2_dist-%s-n4=%d" % (_name(dtype), B * n // 4)
    # a sum of squares has no cancellation and the difference of two stored values is one rounding: the magnitudes are the values
    tol = _tol([(loss32, loss, loss.abs()), (grad32, grad, grad.abs())], tag)
    return dict(pred=pred, target=target, loss=loss, grad=grad, tol=tol, tag=tag)


@pytest.mark.parametrize("B,n", L2_CASES, ids=["n4=1", "n4=65536", "n4=65537", "n4=524289"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_l2_dist(cuda, dtype, B, n):
    O, L, lib = _ops()
    assert B * n // 4 in (1, 65536, 65537, 2048 * 256 + 1)
    c = _l2_case(B, n, dtype)
    tag = c["tag"]
    pred, target = c["pred"].to(cuda), c["target"].to(cuda)
    outs = []
    for _ in range(2):
        loss, ws = Guarded(1, None, F32, cuda), Guarded(O.L2_DIST_PARTS, None, F32, cuda)
        dpred = Guarded(B * n, None, dtype, cuda)
        L.check(lib.imt_l2_dist(O.dt(pred), O._p(pred), O._p(target), O._p(loss.view), O._p(dpred.view), O._p(ws.view), B, n, O._stream()),
                "imt_l2_dist")
        for buf, what in ((loss, "loss"), (ws, "workspace"), (dpred, "dpred")):
            buf.check(tag + " " + what)
        outs.append((loss.view.cpu(), dpred.view.cpu()))
    assert all(_bits_equal(x, y) for x, y in zip(*outs)), tag + ": two calls on the same input differ"
    _within(outs[0][0], c["loss"], c["tol"] * c["loss"].abs(), tag + " loss")
    grad = c["grad"].view(-1)
    _within(outs[0][1], grad, _out_bound(c["tol"], grad.abs(), grad, dtype), tag + " dpred")
