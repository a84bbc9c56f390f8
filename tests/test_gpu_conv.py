"""imt_conv2d, imt_maxpool2d_3x3s2 and imt_image_nhwc (csrc/conv.hip) on exact data, at the smallest shapes that reach each edge
of the kernels: 128-pixel row tiles (M just below, on and just above one), 64- and 128-channel tiles (Cout below, on and
ragged above one; the 128-wide instance from 256 tiles on), 128-byte K steps (K ending inside a step and on one), odd H and W,
stride-2 windows whose last tap row falls in the padding.

Inputs are integers in [-2, 2], weights in {-1, 0, 1}, scales in {0.5, 1, 2}, shifts and residuals small integers: every fp32
sum is exact (|y| <= 2 K * 2 + 7 < 2^24), so fp32 y must equal the fp64 oracle (F.conv2d on NCHW) BIT FOR BIT and bf16 y the
oracle rounded once to nearest even.  Every operand is carved out of a wider buffer filled with NaN, y out of a sentinel buffer:
results must not change, stay finite, and the sentinel must be intact.  Every case is launched twice: same bits."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SENTINEL = 12352.0  # exact in bf16 and out of reach of any result
EPILOGUES = {
    "none": dict(),
    "affine": dict(scale=True, shift=True),
    "resid": dict(residual=True),
    "relu": dict(relu=True),
    "all": dict(scale=True, shift=True, residual=True, relu=True),
}

# (kernel, stride, pad), Cin, Cout, (B, H, W), epilogue -- not the full product: every value of every axis at least once and
# every kernel form with a ragged M, a ragged N and a K tail (marked *)
CASES = [
    ((3, 1, 1), 8, 8, (1, 7, 7), "none"),          # one partial tile of everything; K = 72
    ((3, 1, 1), 72, 72, (1, 17, 15), "all"),        # * M = 255, N = 72, K = 648 = 10 steps + 8
    ((3, 1, 1), 64, 130, (1, 16, 16), "resid"),     # M = 256 on the tile edge; Cout % 4 != 0: scalar stores
    ((3, 2, 1), 24, 130, (3, 15, 9), "affine"),     # * M = 120, N = 130, K = 216; ho = 7 reads row 15: padding
    ((3, 2, 1), 64, 64, (1, 16, 16), "resid"),      # K = 576 = 9 whole bf16 steps, N on the tile edge
    ((1, 1, 0), 64, 72, (2, 14, 14), "relu"),       # M = 392 = 3 tiles + 8; K = one bf16 step exactly
    ((1, 1, 0), 24, 130, (1, 17, 15), "all"),       # * M = 255, N = 130, K = 24
    ((1, 2, 0), 72, 8, (3, 15, 9), "none"),         # * M = 120, N = 8, K = 72
    ((1, 2, 0), 8, 64, (1, 16, 16), "affine"),      # K = 8: a single chunk
    ((7, 2, 3), 8, 64, (1, 17, 15), "relu"),        # the stem's K = 392
    ((7, 2, 3), 24, 72, (2, 14, 14), "all"),        # * M = 98, N = 72, K = 1176 = 18 steps + 24
    ((3, 1, 1), 8, 130, (1, 127, 129), "all"),      # 128 x 2 = 256 tiles: the 128-channel instance, ragged M and N
]


def _id(c):
    (k, s, p), cin, cout, (b, h, w), epi = c
    return "k%ds%dp%d-c%d-n%d-%dx%dx%d-%s" % (k, s, p, cin, cout, b, h, w, epi)


def _carve(t, fill, dev):
    """A dense copy of t on the device inside a wider buffer of ``fill``, 16-byte aligned; returns (view, buffer, offset)."""
    n = t.numel()
    off = 24  # elements: 48 / 96 bytes in front
    buf = torch.full((off + n + 40,), fill, dtype=t.dtype)
    buf[off:off + n] = t.reshape(-1)
    buf = buf.to(dev)
    return buf[off:off + n].view(t.shape), buf, off


def _surround_intact(buf, off, n, fill):
    outside = torch.cat([buf[:off], buf[off + n:]]).float().cpu()
    want = torch.full_like(outside, fill).to(buf.dtype).float()
    return torch.equal(outside, want) if fill == fill else bool(torch.isnan(outside).all())


def _data(case, seed):
    (k, stride, pad), cin, cout, (B, H, W), epi = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (B, H, W, cin), generator=g).double()
    w = torch.randint(-1, 2, (cout, k, k, cin), generator=g).double()
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    e = EPILOGUES[epi]
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (cout,), generator=g)].double() if e.get("scale") else None
    shift = torch.randint(-3, 4, (cout,), generator=g).double() if e.get("shift") else None
    resid = torch.randint(-4, 5, (B, Ho, Wo, cout), generator=g).double() if e.get("residual") else None
    return x, w, scale, shift, resid, bool(e.get("relu"))


def _oracle(x, w, stride, pad, scale, shift, resid, relu):
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=stride, padding=pad).permute(0, 2, 3, 1)
    if scale is not None:
        y = y * scale
    if shift is not None:
        y = y + shift
    if resid is not None:
        y = y + resid
    pre = y
    if relu:
        y = y.clamp_min(0.0)
    return y.contiguous(), pre


def _run(cuda, dtype, x, w, stride, pad, scale, shift, resid, relu):
    """Launch twice on carved operands; returns y (cpu) after checking surroundings, finiteness and repeatability."""
    from imagetranslate_amd import hip_ops as O
    nan = float("nan")
    xd, xbuf, xo = _carve(x.to(dtype), nan, cuda)
    wd, wbuf, wo = _carve(w.to(dtype), nan, cuda)
    sd = _carve(scale.float(), nan, cuda)[0] if scale is not None else None
    hd = _carve(shift.float(), nan, cuda)[0] if shift is not None else None
    rd = _carve(resid.to(dtype), nan, cuda)[0] if resid is not None else None
    k = w.shape[1]
    B, H, W, _ = x.shape
    shape = (B, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1, w.shape[0])
    outs = []
    for _ in range(2):
        yd, ybuf, yo = _carve(torch.full(shape, SENTINEL, dtype=dtype), SENTINEL, cuda)
        got = O.conv2d_nhwc(xd, wd, stride=stride, pad=pad, scale=sd, shift=hd, residual=rd, relu=relu, out=yd)
        assert got.data_ptr() == yd.data_ptr()
        torch.cuda.synchronize()
        assert _surround_intact(ybuf, yo, yd.numel(), SENTINEL), "bytes outside y were written"
        outs.append(yd.cpu())
    assert _surround_intact(xbuf, xo, xd.numel(), nan) and _surround_intact(wbuf, wo, wd.numel(), nan)
    assert torch.equal(xd.cpu(), x.to(dtype)) and torch.equal(wd.cpu(), w.to(dtype)), "an input was modified"
    assert bool(torch.isfinite(outs[0].float()).all()), "a NaN outside an operand reached y"
    assert torch.equal(outs[0].view(torch.int16 if dtype == BF16 else torch.int32),
                       outs[1].view(torch.int16 if dtype == BF16 else torch.int32)), "two calls differ"
    return outs[0]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_conv2d_exact(cuda, case, dtype):
    (k, stride, pad), cin, cout, bhw, epi = case
    x, w, scale, shift, resid, relu = _data(case, seed=CASES.index(case))
    ref, pre = _oracle(x, w, stride, pad, scale, shift, resid, relu)
    assert float(ref.abs().max()) < 2 ** 24
    if relu:
        assert bool((pre < 0).any()) and bool((pre > 0).any()), "ReLU must be seen to act"
    got = _run(cuda, dtype, x, w, stride, pad, scale, shift, resid, relu)
    want = ref.to(dtype)  # fp32: exact; bf16: rounded once, to nearest even (every ref value is an fp32 number)
    bad = (got.double() != want.double())
    print("CONV %s %s max|y| %g mismatches %d / %d" % (_id(case), "bf16" if dtype == BF16 else "f32", float(ref.abs().max()),
                                                       int(bad.sum()), bad.numel()))
    assert not bool(bad.any()), "first mismatch at %s" % (bad.nonzero()[0].tolist(),)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("form", [(3, 1, 1), (3, 2, 1), (1, 2, 0), (7, 2, 3)], ids=lambda f: "k%ds%dp%d" % f)
def test_conv2d_tap_order(cuda, form, dtype):
    """A different value at every (h, w, c) and one one-hot output channel per tap (kh, kw, c): channel n must show exactly the
    input element its tap addresses, or 0 in the padding -- a transposed or mirrored tap order cannot pass."""
    k, stride, pad = form
    B, H, W, C = 2, 5, 6, 8
    x = (torch.arange(H * W * C, dtype=torch.float64).view(1, H, W, C) + 1.0).repeat(B, 1, 1, 1)  # 1..240: exact in bf16
    x[1] = -x[1]
    n_taps = k * k * C
    w = torch.zeros(n_taps, k, k, C, dtype=torch.float64)
    w.view(n_taps, n_taps)[torch.arange(n_taps), torch.arange(n_taps)] = 1.0
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    want = torch.zeros(B, Ho, Wo, n_taps, dtype=torch.float64)
    for kh in range(k):
        for kw in range(k):
            for ho in range(Ho):
                for wo in range(Wo):
                    h, ww = ho * stride - pad + kh, wo * stride - pad + kw
                    if 0 <= h < H and 0 <= ww < W:
                        want[:, ho, wo, (kh * k + kw) * C:(kh * k + kw + 1) * C] = x[:, h, ww, :]
    got = _run(cuda, dtype, x, w, stride, pad, None, None, None, False)
    assert torch.equal(got.double(), want)


POOL_SHAPES = [(2, 7, 9, 8), (1, 15, 17, 24), (1, 16, 16, 64), (3, 1, 1, 8), (1, 2, 33, 72)]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("negative", [False, True], ids=["mixed", "allneg"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_exact(cuda, shape, negative, dtype):
    from imagetranslate_amd import hip_ops as O
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g)
    if negative:
        x = -x.abs() - 0.25  # padding must count as -inf, not 0
    x = x.to(dtype)
    xd, xbuf, xo = _carve(x, float("nan"), cuda)
    got = O.maxpool2d_nhwc(xd).cpu()
    want = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).to(dtype)
    assert got.shape == want.shape
    assert torch.equal(got.float(), want.float())
    if negative:
        assert bool((got.float() < 0).all())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_image_to_nhwc(cuda, dtype):
    from imagetranslate_amd import hip_ops as O
    from tests import resnet_oracle as RO
    g = torch.Generator().manual_seed(3)
    B, H, W = 2, 16, 17
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    img[0].view(-1)[:768] = torch.arange(256, dtype=torch.uint8).repeat_interleave(3)  # every byte value in every channel
    got = O.image_to_nhwc(img.to(cuda), dtype).cpu()
    assert got.shape == (B, H, W, 8) and got.dtype == dtype
    assert torch.equal(got[..., 3:].float(), torch.zeros(B, H, W, 5)), "channels 3-7 must be exactly 0"
    ref64 = RO.normalise(img)
    ref32 = ref64.float()
    if dtype == F32:
        ulp = (torch.nextafter(ref32.abs(), torch.full_like(ref32, float("inf"))) - ref32.abs()).double()
        err = (got[..., :3].double() - ref64).abs()
        print("IMAGE f32 worst error %.3f ulp" % float((err / ulp).max()))
        assert bool((err <= ulp).all())
    else:
        assert torch.equal(got[..., :3].float(), ref32.to(BF16).float())
