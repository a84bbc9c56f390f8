"""The frozen ResNet trunk on the GPU (imagetranslate_amd/resnet.py on csrc/conv.hip) against the fp64 restatement of
tests/resnet_oracle.py, through the image head, checkpoints, ``extract_features`` and ``caption``.

Measure: the project's relative max-norm error max|y - y64| / max|y64| on Gaussian inputs and seeded weights.
  fp32 bar: 1e-4, the project's fp32 bar against fp64.
  bf16 bar: no absolute bar can be derived; the oracle's own "bf16 storage" mode (input, weights and every layer's stored output
  rounded to bf16, arithmetic in fp64) is measured against plain fp64 on the same inputs, and the kernel path must stay
  within 2 x that distance -- the factor covers a different summation order inside each layer and nothing else.
Each case prints ``TRUNK <case> <dtype> err ... (oracle bf16 mode ...)`` before it asserts (pytest -s; DESIGN.md records them)."""
import os

import pytest
import torch

from tests import resnet_oracle as RO

pytestmark = pytest.mark.gpu

F32_BAR = 1e-4
CASES = {"d1-64": (1, 2, 64, 64), "d3-64": (3, 2, 64, 64), "d1-224": (1, 1, 224, 224)}
_REFS = {}


def _ref(case):
    """(state dict, NCHW input, fp64 features, fp64 features of the bf16-storage mode), computed once per case."""
    if case not in _REFS:
        depth, B, H, W = CASES[case]
        sd = RO.make_state(depth, seed=depth)
        x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(11 + H))
        _REFS[case] = (sd, x, RO.trunk_forward(sd, depth, x), RO.trunk_forward(sd, depth, x, bf16_storage=True))
    return _REFS[case]


def _trunk(case, dtype):
    from imagetranslate_amd.resnet import ResNetTrunk
    return ResNetTrunk(CASES[case][0], dtype).load_state_dict(_ref(case)[0]).cuda()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_trunk_against_fp64(cuda, case, dtype):
    depth, B, H, W = CASES[case]
    sd, x, y64, y64_bf16 = _ref(case)
    got = _trunk(case, dtype)(x.cuda())
    C = 512 if depth < 3 else 2048
    assert got.shape == (B, (H // 32) * (W // 32), C) and got.dtype == dtype
    if case == "d1-224":
        assert got.shape[1] == 49
        # region h * 7 + w of the oracle's view(B, C, -1).permute(0, 2, 1) is pixel (h, w) of layer4's map
        assert torch.equal(y64.view(B, 7, 7, C)[:, 3, 5], y64[:, 3 * 7 + 5])
    err, own = RO.rel_err(got, y64), RO.rel_err(y64_bf16, y64)
    print("TRUNK %s %s err %.3e (oracle bf16 mode %.3e)" % (case, "f32" if dtype == torch.float32 else "bf16", err, own))
    if dtype == torch.float32:
        assert err < F32_BAR
    else:
        assert err <= 2.0 * own
    # the NHWC input of image_to_nhwc's layout gives the same bits as the reference's NCHW
    nhwc = torch.zeros(B, H, W, 8)
    nhwc[..., :3] = x.permute(0, 2, 3, 1)
    again = _trunk(case, dtype)(nhwc.to(dtype).cuda())
    assert torch.equal(again.float().cpu(), got.float().cpu())


def _cap(tp=None):
    from imagetranslate_amd.image_model import ImageCaptioning
    from imagetranslate_amd.textprocessor import SyntheticTextProcessor
    torch.manual_seed(0)
    return ImageCaptioning(tp or SyntheticTextProcessor(300), lang_dec=False, enc_layer=1, dec_layer=1, embed_dim=128,
                           intermediate_dim=256, num_attention_heads=4, resnet_depth=1, use_obj=False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_encode_pixels_equals_encode_features(cuda, dtype):
    from imagetranslate_amd.resnet import ResNetTrunk
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(2))
    m = _cap().cuda().eval()
    m.set_compute_dtype(dtype)
    with pytest.raises(ValueError, match="attach_trunk"):
        m.encode(images=x)
    trunk = ResNetTrunk(1, dtype).load_state_dict(_ref("d1-64")[0])
    m.image_model.attach_trunk(trunk)
    with torch.no_grad():
        from_pixels = m.encode(images=x)[0]
        feats = trunk(x.cuda())
        from_feats = m.encode(images=feats)[0]
    assert trunk.device.type == "cuda" and feats.shape == (2, 49, 512) and feats.dtype == dtype
    assert from_pixels.shape == (2, 49, 128)
    assert torch.equal(from_pixels.float().cpu(), from_feats.float().cpu())


def test_checkpoint_with_trunk_gives_the_same_features(cuda, tmp_path):
    from imagetranslate_amd.image_model import ImageCaptioning
    from imagetranslate_amd.seq2seq import Seq2Seq
    from imagetranslate_amd.textprocessor import SyntheticTextProcessor
    sd, x, _, _ = _ref("d1-64")
    m = _cap()
    m.image_model.attach_trunk(_trunk("d1-64", torch.float32))
    want = m.image_model.trunk(x.cuda())
    m.save(str(tmp_path / "ckpt"))
    got = Seq2Seq.load(ImageCaptioning, str(tmp_path / "ckpt"), tok_dir=None, use_obj=False, text_processor=SyntheticTextProcessor(300))
    assert got.image_model.trunk is not None
    feats = got.image_model.region_features(x, torch.float32)
    assert torch.equal(feats.cpu(), want.cpu())


def _images(d):
    """Four generated pictures -- two sizes, one greyscale, one truncated file -- each as a PNG and as a JPEG (the loaders skip
    *.png paths as the reference's do, src/dataset.py:309, so ``caption`` serves the JPEGs)."""
    from PIL import Image
    g = torch.Generator().manual_seed(4)
    specs = [("a_wide", (300, 200), "RGB"), ("b_tall", (200, 300), "RGB"), ("c_grey", (260, 240), "L"), ("d_cut", (280, 230), "RGB")]
    names = []
    for stem, (w, h), mode in specs:
        base = torch.rand(h // 20 + 1, w // 20 + 1, 3 if mode == "RGB" else 1, generator=g)
        big = torch.nn.functional.interpolate(base.permute(2, 0, 1)[None], size=(h, w), mode="bilinear")[0].permute(1, 2, 0)
        arr = (big * 255).to(torch.uint8).numpy()
        img = Image.fromarray(arr if mode == "RGB" else arr[..., 0], mode)
        for ext in (".png", ".jpg"):
            path = os.path.join(d, stem + ext)
            img.save(path)
            if stem == "d_cut":
                blob = open(path, "rb").read()
                with open(path, "wb") as fw:
                    fw.write(blob[:len(blob) // 3] if ext == ".png" else blob[:40])
            names.append(stem + ext)
    return sorted(names)


@pytest.mark.parametrize("fp32", [True, False], ids=["f32", "bf16"])
def test_extract_features_cli_and_caption(cuda, tmp_path, capsys, fp32):
    from PIL import Image
    from imagetranslate_amd import caption, dataset, extract_features
    from imagetranslate_amd.seq_gen import BeamDecoder
    from imagetranslate_amd.textprocessor import SyntheticTextProcessor
    d = str(tmp_path / "images")
    os.makedirs(d)
    names = _images(d)
    sd = RO.make_state(1, seed=1)
    torch.save(sd, str(tmp_path / "resnet18.pt"))
    out = os.path.join(d, "features.pt")
    extract_features.main(["--images", d, "--trunk", str(tmp_path / "resnet18.pt"), "--depth", "1", "--output", out, "--batch", "3"]
                          + (["--fp32"] if fp32 else []))
    assert "d_cut" in capsys.readouterr().err, "the truncated file is reported"
    assert os.listdir(d).count("features.pt") == 1 and not [f for f in os.listdir(d) if ".tmp" in f]
    feats = dataset.RegionFeatures(d)
    assert feats.paths == names and feats.feats.shape == (8, 49, 512) and feats.feats.dtype == torch.float32
    # the oracle on the same preprocessed pixels
    pixels = []
    for n in names:
        try:
            with Image.open(os.path.join(d, n)) as im:
                pixels.append(RO.preprocess(im))
        except Exception:
            pixels.append(torch.zeros(224, 224, 3, dtype=torch.uint8))
    x = RO.normalise(torch.stack(pixels)).permute(0, 3, 1, 2)
    y64 = RO.trunk_forward(sd, 1, x)
    err = RO.rel_err(feats.feats, y64)
    own = RO.rel_err(RO.trunk_forward(sd, 1, x, bf16_storage=True), y64)
    print("TRUNK extract %s err %.3e (oracle bf16 mode %.3e)" % ("f32" if fp32 else "bf16", err, own))
    assert err < F32_BAR if fp32 else err <= 2.0 * own
    # the truncated files' rows are the black image's
    black = extract_features.extract(_loaded(sd), d, ["no_such_file.jpg"], dtype=torch.float32 if fp32 else torch.bfloat16)
    capsys.readouterr()
    for n in ("d_cut.png", "d_cut.jpg"):
        assert torch.equal(feats.get([n])[0], black[0]), n
    assert not torch.equal(feats.get(["a_wide.png"])[0], black[0])

    class TP(SyntheticTextProcessor):
        def decode(self, ids):
            return " ".join(self.id2token(i) for i in ids)

    tp = TP(300)
    model = _cap(tp).cuda().eval()
    model.set_compute_dtype(torch.float32 if fp32 else torch.bfloat16)
    data = dataset.ImageDataset(d, 3, target_lang=0, first_token=tp.token_id("<en>"))
    gen = BeamDecoder(model, beam_width=2)
    lines = []
    for i in range(len(data)):
        caps, paths = caption.caption_batch(data[i], gen, tp, max_len=8)
        lines += [p + "\t" + c for p, c in zip(paths, caps)]
    served = [n for n in names if not n.endswith(".png")]
    assert [ln.split("\t")[0] for ln in lines] == served, "one line per image the loader serves"


def _loaded(sd):
    from imagetranslate_amd.resnet import ResNetTrunk
    return ResNetTrunk(1).load_state_dict(sd)
