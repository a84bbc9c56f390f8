"""fp64 CPU restatement of the frozen ResNet trunk (checker only; shared by test_trunk_host.py and test_gpu_trunk.py).

The reference builds its trunk from torchvision (src/image_model.py:85-97), which is not installed here, so the reference's
trunk cannot be imported: the block structure, the state-dict names and the resize rule below are restated from
torchvision's published definitions (ResNet v1.5: BasicBlock = 3x3 stride s -> 3x3; Bottleneck = 1x1 -> 3x3 stride s -> 1x1,
expansion 4; a 1x1 stride-s downsample where the shape changes; transforms.Resize(256) = shorter side to 256, longer to
int(256 * long / short); CenterCrop(224) at int(round((size - 224) / 2))) and are NOT pinned by a run of the reference.
"""
import torch
import torch.nn.functional as F

LAYERS = {1: ("basic", (2, 2, 2, 2)), 2: ("basic", (3, 4, 6, 3)), 3: ("bottleneck", (3, 4, 6, 3)),
          4: ("bottleneck", (3, 4, 23, 3)), 5: ("bottleneck", (3, 8, 36, 3))}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def structure(depth):
    """[(conv key prefix, bn key prefix, Cin, Cout, k)] in state-dict order."""
    kind, counts = LAYERS[depth]
    out = [("conv1", "bn1", 3, 64, 7)]
    inplanes = 64
    for li, (planes, n) in enumerate(zip((64, 128, 256, 512), counts), 1):
        for i in range(n):
            stride = 2 if li > 1 and i == 0 else 1
            p = "layer%d.%d." % (li, i)
            if kind == "basic":
                width = planes
                out += [(p + "conv1", p + "bn1", inplanes, planes, 3), (p + "conv2", p + "bn2", planes, planes, 3)]
            else:
                width = 4 * planes
                out += [(p + "conv1", p + "bn1", inplanes, planes, 1), (p + "conv2", p + "bn2", planes, planes, 3),
                        (p + "conv3", p + "bn3", planes, width, 1)]
            if stride != 1 or inplanes != width:
                out.append((p + "downsample.0", p + "downsample.1", inplanes, width, 1))
            inplanes = width
    return out


def make_state(depth, seed=0):
    """Seeded torchvision-format state dict (fp32): He-normal convolutions, gamma and running_var in [0.5, 1.5], beta and
    running_mean in [-0.2, 0.2] -- activations stay O(1) through 50 layers."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for conv, bn, cin, cout, k in structure(depth):
        sd[conv + ".weight"] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        sd[bn + ".weight"] = torch.rand(cout, generator=g) + 0.5
        sd[bn + ".bias"] = torch.rand(cout, generator=g) * 0.4 - 0.2
        sd[bn + ".running_mean"] = torch.rand(cout, generator=g) * 0.4 - 0.2
        sd[bn + ".running_var"] = torch.rand(cout, generator=g) + 0.5
        sd[bn + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)
    return sd


def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float64)


def trunk_forward(sd, depth, x, bf16_storage=False):
    """x: NCHW [B, 3, H, W], normalised.  Returns fp64 [B, regions, C] (view(B, C, -1).permute(0, 2, 1)).  ``bf16_storage``:
    the input, the weights and every layer's stored output are rounded to bf16; the arithmetic stays fp64."""
    store = _bf16 if bf16_storage else (lambda t: t)

    def cbr(x, conv, bn, stride, pad, relu, residual=None):
        w = sd[conv + ".weight"].double()
        y = F.conv2d(x, store(w), stride=stride, padding=pad)
        y = F.batch_norm(y, sd[bn + ".running_mean"].double(), sd[bn + ".running_var"].double(), sd[bn + ".weight"].double(),
                         sd[bn + ".bias"].double(), training=False, eps=1e-5)
        if residual is not None:
            y = y + residual
        return store(F.relu(y) if relu else y)

    kind, counts = LAYERS[depth]
    x = store(x.double())
    x = cbr(x, "conv1", "bn1", 2, 3, True)
    x = F.max_pool2d(x, 3, 2, 1)
    inplanes = 64
    for li, (planes, n) in enumerate(zip((64, 128, 256, 512), counts), 1):
        for i in range(n):
            stride = 2 if li > 1 and i == 0 else 1
            p = "layer%d.%d." % (li, i)
            width = planes if kind == "basic" else 4 * planes
            identity = x
            if stride != 1 or inplanes != width:
                identity = cbr(x, p + "downsample.0", p + "downsample.1", stride, 0, False)
            if kind == "basic":
                y = cbr(x, p + "conv1", p + "bn1", stride, 1, True)
                x = cbr(y, p + "conv2", p + "bn2", 1, 1, True, identity)
            else:
                y = cbr(x, p + "conv1", p + "bn1", 1, 0, True)
                y = cbr(y, p + "conv2", p + "bn2", stride, 1, True)
                x = cbr(y, p + "conv3", p + "bn3", 1, 0, True, identity)
            inplanes = width
    B, C = x.shape[:2]
    return x.reshape(B, C, -1).permute(0, 2, 1).contiguous()


def rel_err(y, y64):
    """The project's measure: max|y - y64| / max|y64|."""
    y64 = y64.double()
    return float((y.detach().cpu().double() - y64).abs().max() / y64.abs().max())


# ---------------------------------------------------------------- preprocessing (src/dataset.py:283-289, 366-373)
def resize_size(w, h, size=256):
    """(new width, new height) of transforms.Resize(size) for a PIL image of (w, h)."""
    if w <= h:
        return size, int(size * h / w)
    return int(size * w / h), size


def crop_box(w, h, size=224):
    """(left, top) of transforms.CenterCrop(size)."""
    return int(round((w - size) / 2.0)), int(round((h - size) / 2.0))


def preprocess(img):
    """PIL image -> uint8 [224, 224, 3]: RGB, bilinear resize of the shorter side to 256, centre crop 224."""
    from PIL import Image
    img = img.convert("RGB")
    w, h = img.size
    img = img.resize(resize_size(w, h), Image.BILINEAR)
    left, top = crop_box(*img.size)
    img = img.crop((left, top, left + 224, top + 224))
    import numpy as np
    return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy())


def normalise(u8):
    """uint8 [..., 3] -> fp64 [..., 3]: (v / 255 - mean) / std with the fp32 mean / std the kernel is given."""
    mean = torch.tensor(MEAN, dtype=torch.float32).double()
    std = torch.tensor(STD, dtype=torch.float32).double()
    return (u8.double() / 255.0 - mean) / std
