"""CPU side of the frozen ResNet trunk (imagetranslate_amd/resnet.py, extract_features.py): BatchNorm folding, state-dict keys,
weight repacking, checkpoints with and without a trunk, the PIL preprocessing, and the host-side refusals of imt_conv2d (no
launch: safe without a GPU)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import reference_model as R
from tests import resnet_oracle as RO

ERR = -1


def test_folded_batchnorm_equals_batch_norm():
    from imagetranslate_amd.resnet import fold_bn
    g = torch.Generator().manual_seed(0)
    C = 37
    gamma, var = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5
    beta, mean = torch.rand(C, generator=g) * 0.4 - 0.2, torch.rand(C, generator=g) * 0.4 - 0.2
    x = torch.randn(3, C, 5, 4, generator=g, dtype=torch.float64)
    scale, shift = fold_bn(gamma, beta, mean, var)
    assert scale.dtype == torch.float32 and shift.dtype == torch.float32
    want = F.batch_norm(x, mean.double(), var.double(), gamma.double(), beta.double(), training=False, eps=1e-5)
    got = x * scale.double().view(1, C, 1, 1) + shift.double().view(1, C, 1, 1)
    # the fold is fp32: a few roundings of scale (<= 2^-23 relative each) times |x| <= 5, and of shift
    assert float((got - want).abs().max()) < 16 * 2.0 ** -23 * float(x.abs().max()) * float(scale.max())


@pytest.mark.parametrize("depth,count", [(1, 120), (3, 318)])
def test_key_sets_and_counts(depth, count):
    from imagetranslate_amd.resnet import ResNetTrunk, trunk_shapes
    shapes = trunk_shapes(depth)
    sd = RO.make_state(depth)
    assert len(shapes) == count and set(shapes) == set(sd)
    assert all(tuple(sd[k].shape) == s for k, s in shapes.items())
    trunk = ResNetTrunk(depth).load_state_dict(dict(sd, **{"fc.weight": torch.zeros(1000, 512), "fc.bias": torch.zeros(1000)}))
    out = trunk.state_dict()
    assert list(out) == list(shapes) and not any(k.startswith("fc.") for k in out)
    assert all(torch.equal(out[k], sd[k]) and out[k].dtype == sd[k].dtype for k in sd)
    assert trunk.out_channels == (512 if depth == 1 else 2048)
    # num_batches_tracked is optional
    slim = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    assert len(ResNetTrunk(depth).load_state_dict(slim).state_dict()) == count
    assert "layer1.0.downsample.0.weight" not in shapes if depth == 1 else "layer1.0.downsample.0.weight" in shapes
    assert "layer2.0.downsample.1.running_var" in shapes


def test_repack_and_stem_padding_round_trip():
    from imagetranslate_amd.resnet import STEM_CIN, pack_weight, unpack_weight
    g = torch.Generator().manual_seed(1)
    w = torch.randn(6, 16, 3, 3, generator=g)
    p = pack_weight(w)
    assert p.shape == (6, 3, 3, 16) and p.is_contiguous()
    assert float(p[4, 2, 1, 7]) == float(w[4, 7, 2, 1])
    assert torch.equal(unpack_weight(p), w)
    stem = torch.randn(64, 3, 7, 7, generator=g)
    ps = pack_weight(stem, cin_pad=STEM_CIN)
    assert ps.shape == (64, 7, 7, 8) and torch.equal(ps[..., 3:], torch.zeros(64, 7, 7, 5))
    assert torch.equal(unpack_weight(ps, cin=3), stem)
    assert pack_weight(stem, torch.bfloat16, STEM_CIN).dtype == torch.bfloat16


def test_load_state_dict_names_the_key():
    from imagetranslate_amd.resnet import ResNetTrunk
    sd = RO.make_state(1)
    missing = dict(sd)
    del missing["layer3.1.bn2.running_var"]
    with pytest.raises(KeyError, match="layer3.1.bn2.running_var"):
        ResNetTrunk(1).load_state_dict(missing)
    bad = dict(sd)
    bad["layer2.0.downsample.0.weight"] = torch.zeros(128, 64, 3, 3)
    with pytest.raises(ValueError, match="layer2.0.downsample.0.weight"):
        ResNetTrunk(1).load_state_dict(bad)
    with pytest.raises(KeyError, match="image_model.conv1.weight"):
        ResNetTrunk(1).load_state_dict(sd, prefix="image_model.")


def test_depth_6_is_refused():
    from imagetranslate_amd.resnet import ResNetTrunk
    with pytest.raises(NotImplementedError, match="resnext"):
        ResNetTrunk(6)
    with pytest.raises(ValueError):
        ResNetTrunk(0)


def _cap(seed=0):
    from imagetranslate_amd.image_model import ImageCaptioning
    torch.manual_seed(seed)
    return ImageCaptioning(R.SyntheticTextProcessor(300), lang_dec=False, enc_layer=1, dec_layer=1, embed_dim=64, intermediate_dim=128,
                           num_attention_heads=4, resnet_depth=1, use_obj=False)


def test_checkpoint_with_and_without_trunk_round_trips(tmp_path):
    from imagetranslate_amd.image_model import ImageCaptioning
    from imagetranslate_amd.resnet import ResNetTrunk
    from imagetranslate_amd.seq2seq import Seq2Seq
    tp = R.SyntheticTextProcessor(300)
    m = _cap()
    plain = {k: v.clone() for k, v in m.state_dict().items()}
    # without a trunk: the file holds the model's own keys and nothing else, and reloads to the same tensors
    m.save(str(tmp_path / "plain"))
    on_disk = torch.load(str(tmp_path / "plain" / "mt_model.state_dict"), weights_only=True)
    assert list(on_disk) == list(plain) and all(torch.equal(on_disk[k], plain[k]) for k in plain)
    got = Seq2Seq.load(ImageCaptioning, str(tmp_path / "plain"), tok_dir=None, use_obj=False, text_processor=tp)
    assert got.image_model.trunk is None
    assert all(torch.equal(v.cpu(), plain[k]) for k, v in got.state_dict().items())
    # with a trunk: its 120 tensors go in under the reference's names, come back attached, and save again to the same bytes
    tsd = RO.make_state(1, seed=5)
    m.image_model.attach_trunk(ResNetTrunk(1).load_state_dict(tsd))
    assert list(m.state_dict()) == list(plain), "the trunk is not a registered submodule"
    assert not any("conv1" in n or "layer1" in n for n, _ in m.named_parameters())
    m.save(str(tmp_path / "with"))
    first = torch.load(str(tmp_path / "with" / "mt_model.state_dict"), weights_only=True)
    assert set(first) == set(plain) | {"image_model." + k for k in tsd}
    assert all(torch.equal(first["image_model." + k], tsd[k]) and first["image_model." + k].dtype == tsd[k].dtype for k in tsd)
    got = Seq2Seq.load(ImageCaptioning, str(tmp_path / "with"), tok_dir=None, use_obj=False, text_processor=tp)
    assert got.image_model.trunk is not None and got.image_model.trunk.depth == 1
    # extract_features --model DIR reads the trunk (and its depth) from such a checkpoint, and refuses one without a trunk
    from imagetranslate_amd import extract_features as E
    from_ckpt = E.load_trunk(model_dir=str(tmp_path / "with")).state_dict()
    assert all(torch.equal(from_ckpt[k], tsd[k]) for k in tsd)
    with pytest.raises(ValueError, match="no CNN trunk"):
        E.load_trunk(model_dir=str(tmp_path / "plain"))
    with pytest.raises(ValueError, match="exactly one"):
        E.load_trunk()
    got.save(str(tmp_path / "again"))
    second = torch.load(str(tmp_path / "again" / "mt_model.state_dict"), weights_only=True)
    assert list(second) == list(first)
    for k in first:
        assert second[k].dtype == first[k].dtype and torch.equal(second[k].reshape(-1).view(torch.uint8), first[k].reshape(-1).view(torch.uint8)), k


def test_pixels_without_trunk_raise():
    m = _cap()
    with pytest.raises(ValueError, match="attach_trunk"):
        m.image_model(torch.zeros(1, 3, 64, 64))
    from imagetranslate_amd.resnet import ResNetTrunk
    with pytest.raises(ValueError, match="channels"):
        m.image_model.attach_trunk(ResNetTrunk(3))


@pytest.mark.parametrize("size,resized,offset", [((300, 200), (384, 256), (80, 16)), ((200, 300), (256, 384), (16, 80))])
def test_preprocessing_sizes_and_crop(size, resized, offset):
    """A generated image whose pixel (x, y) encodes its own position: after the resize and the crop the output is 224 x 224 and
    its corner shows the stated offsets."""
    from PIL import Image
    from imagetranslate_amd import extract_features as E
    w, h = size
    assert E.resize_size(w, h) == resized == RO.resize_size(w, h)
    assert E.crop_offset(*resized) == offset == RO.crop_box(*resized)
    xs = torch.arange(w).view(1, w).expand(h, w)
    ys = torch.arange(h).view(h, 1).expand(h, w)
    rgb = torch.stack([xs * 255 // (w - 1), ys * 255 // (h - 1), (xs + ys) % 256], dim=-1).to(torch.uint8)
    img = Image.fromarray(rgb.numpy(), "RGB")
    out = E.preprocess(img)
    assert out.shape == (224, 224, 3) and out.dtype == torch.uint8
    assert torch.equal(out, RO.preprocess(img))
    # the same image resized whole, cropped here by the stated offsets
    import numpy as np
    whole = torch.from_numpy(np.asarray(img.resize(resized, Image.BILINEAR)).copy())
    left, top = offset
    assert torch.equal(out, whole[top:top + 224, left:left + 224])
    grey = Image.fromarray(rgb[..., 0].numpy(), "L")
    assert E.preprocess(grey).shape == (224, 224, 3)


def test_unreadable_image_becomes_black(tmp_path, capsys):
    from imagetranslate_amd import extract_features as E
    (tmp_path / "bad.png").write_bytes(b"\x89PNG\r\n\x1a\n" + b"\x00" * 20)
    out = E.load_image(str(tmp_path), "bad.png")
    assert out.shape == (224, 224, 3) and int(out.sum()) == 0
    assert "bad.png" in capsys.readouterr().err
    (tmp_path / "sub").mkdir()
    for name in ("b.jpg", "a.PNG", "sub/c.jpeg", "notes.txt"):
        (tmp_path / name).write_bytes(b"")
    assert E.list_images(str(tmp_path)) == ["a.PNG", "b.jpg", "bad.png", "sub/c.jpeg"]


def _conv_args(**kw):
    from imagetranslate_amd import _lib as L
    a = L.ConvArgs()
    base = dict(dtype=L.IMT_BF16, B=1, H=8, W=8, Cin=8, Cout=8, KH=3, KW=3, stride=1, pad_h=1, pad_w=1, relu=0,
                x=0x1000, w=0x2000, y=0x3000, scale=None, shift=None, residual=None)
    base.update(kw)
    for k, v in base.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,word", [
    (dict(dtype=7), b"dtype"), (dict(x=None), b"x is null"), (dict(w=None), b"w is null"), (dict(y=None), b"y is null"),
    (dict(B=0), b"positive"), (dict(H=-1), b"positive"), (dict(Cout=0), b"positive"), (dict(KW=0), b"positive"),
    (dict(stride=3), b"stride"), (dict(stride=0), b"stride"), (dict(pad_h=-1), b"padding"),
    (dict(Cin=12), b"multiple of 8"), (dict(Cin=3), b"multiple of 8"),
    (dict(H=2, KH=7, pad_h=1), b"Ho or Wo"), (dict(W=1, KW=3, pad_w=0), b"Ho or Wo"),
    (dict(x=0x1008), b"16-byte"), (dict(w=0x2004), b"16-byte"), (dict(y=0x3002), b"16-byte"), (dict(residual=0x4008), b"16-byte"),
    (dict(B=1 << 20, H=1 << 10, W=1 << 10), b"32-bit pixel index"),
    (dict(Cin=1 << 30, KH=1, KW=3, pad_h=0), b"31 bits"),
])
def test_conv2d_host_refusals(kw, word):
    from imagetranslate_amd import _lib as L
    lib = L.load()
    assert lib.imt_conv2d(ctypes.byref(_conv_args(**kw)), None) == ERR
    assert word in lib.imt_last_error(), lib.imt_last_error()


def test_conv2d_supported_and_other_refusals():
    from imagetranslate_amd import _lib as L
    lib = L.load()
    assert lib.imt_conv2d(None, None) == ERR
    assert lib.imt_conv2d_supported(L.IMT_BF16, 64, 3, 3, 1) == 1 and lib.imt_conv2d_supported(L.IMT_F32, 8, 7, 7, 2) == 1
    assert lib.imt_conv2d_supported(L.IMT_BF16, 12, 3, 3, 1) == 0 and lib.imt_conv2d_supported(L.IMT_BF16, 64, 3, 3, 3) == 0
    assert lib.imt_conv2d_supported(5, 64, 3, 3, 1) == 0
    P = 0x1000
    assert lib.imt_maxpool2d_3x3s2(L.IMT_BF16, P, P, 1, 8, 8, 12, None) == ERR and b"multiple of 8" in lib.imt_last_error()
    assert lib.imt_maxpool2d_3x3s2(L.IMT_BF16, None, P, 1, 8, 8, 8, None) == ERR
    assert lib.imt_maxpool2d_3x3s2(9, P, P, 1, 8, 8, 8, None) == ERR
    m = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    s0 = (ctypes.c_float * 3)(0.5, 0.0, 0.5)
    assert lib.imt_image_nhwc(L.IMT_F32, P, P, 1, 8, 8, m, s0, None) == ERR and b"std" in lib.imt_last_error()
    assert lib.imt_image_nhwc(L.IMT_F32, P, P, 0, 8, 8, m, m, None) == ERR
    assert lib.imt_image_nhwc(L.IMT_F32, P, None, 1, 8, 8, m, m, None) == ERR
