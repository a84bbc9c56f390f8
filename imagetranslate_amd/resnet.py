"""Frozen ResNet trunk: pixels -> region features, the reference's ``ModifiedResnet`` up to ``x8.view().permute()``
(``src/image_model.py:24-36``; ``init_net`` ``:85-97`` maps ``resnet_depth`` 1-5 to resnet18/34/50/101/152).

Every convolution is one ``imt_conv2d`` launch (implicit GEMM on MFMA, csrc/conv.hip) that carries its BatchNorm -- folded on
the host into an fp32 per-channel scale and shift -- and, where they apply, the residual add and the ReLU in its epilogue;
the stem's max pool is ``imt_maxpool2d_3x3s2``.  Activations are NHWC, so the last layer's ``[B, H/32, W/32, C]`` viewed as
``[B, regions, C]`` is the reference's ``view(B, C, -1).permute(0, 2, 1)`` with region index ``h * (W/32) + w``.

The trunk is always frozen and always in inference mode: running statistics, no gradient (two deviations from the reference,
DESIGN.md section 1).  Parameters and buffers carry torchvision's state-dict names; the block structure is restated from
torchvision's published definition (BasicBlock / Bottleneck with the stride on the 3 x 3, "ResNet v1.5").
"""
from collections import OrderedDict, namedtuple

import torch

from . import hip_ops as O

BN_EPS = 1e-5
STEM_CIN = 8  # the stem's 3 input channels padded to one 16-byte chunk (imt_image_nhwc writes zeros into 3-7)

_SPECS = {1: ("basic", (2, 2, 2, 2)), 2: ("basic", (3, 4, 6, 3)), 3: ("bottleneck", (3, 4, 6, 3)),
          4: ("bottleneck", (3, 4, 23, 3)), 5: ("bottleneck", (3, 8, 36, 3))}
_NAMES = {1: "resnet18", 2: "resnet34", 3: "resnet50", 4: "resnet101", 5: "resnet152", 6: "resnext101_32x8d"}
_BN_FIELDS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")

# one convolution with its BatchNorm: state-dict prefixes, [Cout, Cin, k, k] and the launch geometry
Conv = namedtuple("Conv", "conv bn cin cout k stride pad")
Block = namedtuple("Block", "body down")


def _check_depth(depth):
    if depth == 6:
        raise NotImplementedError("ResNetTrunk: depth 6 (%s) needs grouped convolutions, which imt_conv2d does not take" % _NAMES[6])
    if depth not in _SPECS:
        raise ValueError("ResNetTrunk: depth must be 1..5 (resnet18/34/50/101/152), got %r" % (depth,))


def trunk_plan(depth):
    """(stem Conv, [Block]) of the trunk of ``depth``."""
    _check_depth(depth)
    kind, counts = _SPECS[depth]
    stem = Conv("conv1", "bn1", 3, 64, 7, 2, 3)
    blocks, inplanes = [], 64
    for li, (planes, n) in enumerate(zip((64, 128, 256, 512), counts), 1):
        for i in range(n):
            stride = 2 if (li > 1 and i == 0) else 1
            pre = "layer%d.%d." % (li, i)
            if kind == "basic":
                out = planes
                body = [Conv(pre + "conv1", pre + "bn1", inplanes, planes, 3, stride, 1),
                        Conv(pre + "conv2", pre + "bn2", planes, planes, 3, 1, 1)]
            else:
                out = 4 * planes
                body = [Conv(pre + "conv1", pre + "bn1", inplanes, planes, 1, 1, 0),
                        Conv(pre + "conv2", pre + "bn2", planes, planes, 3, stride, 1),
                        Conv(pre + "conv3", pre + "bn3", planes, out, 1, 1, 0)]
            down = None
            if stride != 1 or inplanes != out:
                down = Conv(pre + "downsample.0", pre + "downsample.1", inplanes, out, 1, stride, 0)
            blocks.append(Block(body, down))
            inplanes = out
    return stem, blocks


def trunk_convs(depth):
    stem, blocks = trunk_plan(depth)
    return [stem] + [c for b in blocks for c in (b.body + ([b.down] if b.down else []))]


def trunk_shapes(depth):
    """Ordered {state-dict key: shape} of the trunk (torchvision's names, without fc.*)."""
    out = OrderedDict()
    for c in trunk_convs(depth):
        out[c.conv + ".weight"] = (c.cout, c.cin, c.k, c.k)
        for f in _BN_FIELDS:
            out[c.bn + "." + f] = () if f == "num_batches_tracked" else (c.cout,)
    return out


def feature_dim(depth):
    _check_depth(depth)
    return 512 if _SPECS[depth][0] == "basic" else 2048


def fold_bn(weight, bias, running_mean, running_var, eps=BN_EPS):
    """BatchNorm in inference mode as y = x * scale + shift, folded in fp32: scale = gamma / sqrt(var + eps),
    shift = beta - mean * scale."""
    scale = weight.float() / torch.sqrt(running_var.float() + eps)
    return scale.contiguous(), (bias.float() - running_mean.float() * scale).contiguous()


def pack_weight(w, dtype=torch.float32, cin_pad=None):
    """[Cout, Cin, KH, KW] -> imt_conv2d's [Cout, KH, KW, Cin] in ``dtype``, Cin zero-padded up to ``cin_pad``."""
    p = w.permute(0, 2, 3, 1)
    if cin_pad is not None and cin_pad > p.shape[3]:
        p = torch.nn.functional.pad(p, (0, cin_pad - p.shape[3]))
    return p.to(dtype).contiguous()


def unpack_weight(p, cin=None):
    """The inverse of pack_weight: [Cout, KH, KW, Cin(+pad)] -> [Cout, Cin, KH, KW]."""
    if cin is not None:
        p = p[..., :cin]
    return p.permute(0, 3, 1, 2).contiguous()


class ResNetTrunk:
    """``ResNetTrunk(depth)(x)``: x is the ``[B, H, W, 8]`` output of ``hip_ops.image_to_nhwc``, decoded ``uint8 [B, H, W, 3]``
    images, or float NCHW ``[B, 3, H, W]`` that is already normalised (the reference's layout; permuted and padded on the
    device).  Returns region features ``[B, regions, C]`` in the compute dtype.  Not an nn.Module: it owns no trainable
    parameter, so it stays outside a model's flat parameter store."""

    def __init__(self, depth: int = 1, dtype=torch.float32):
        self.depth = depth
        self.stem, self.blocks = trunk_plan(depth)
        self.out_channels = feature_dim(depth)
        self.dtype = dtype
        self.device = torch.device("cpu")
        self._state = None   # the loaded tensors: NCHW, fp32, on the host
        self._packed = {}    # conv prefix -> (w [Cout, KH, KW, Cin], scale, shift) on self.device

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, state, prefix=""):
        """Takes torchvision's keys (below ``prefix``); names the first missing or mis-shaped one.  ``fc.*`` is ignored and
        ``num_batches_tracked`` is optional."""
        own = OrderedDict()
        for key, shape in trunk_shapes(self.depth).items():
            t = state.get(prefix + key)
            if t is None:
                if key.endswith("num_batches_tracked"):
                    own[key] = torch.zeros((), dtype=torch.int64)
                    continue
                raise KeyError("ResNetTrunk(depth=%d): state dict has no %r" % (self.depth, prefix + key))
            if key.endswith("num_batches_tracked"):
                own[key] = t.detach().cpu().to(torch.int64).reshape(())
                continue
            if tuple(t.shape) != shape:
                raise ValueError("ResNetTrunk(depth=%d): %r is %s, expected %s" % (self.depth, prefix + key, tuple(t.shape), shape))
            own[key] = t.detach().cpu().float().contiguous()
        self._state = own
        self._pack()
        return self

    def state_dict(self, prefix=""):
        """The loaded tensors under torchvision's names: NCHW, fp32 (what the reference's trunk loads)."""
        self._require_weights()
        return OrderedDict((prefix + k, v) for k, v in self._state.items())

    def _require_weights(self):
        if self._state is None:
            raise RuntimeError("ResNetTrunk: no weights loaded (load_state_dict)")

    def _pack(self):
        self._packed = {}
        if self._state is None:
            return
        s = self._state
        for c in trunk_convs(self.depth):
            w = pack_weight(s[c.conv + ".weight"], self.dtype, max(c.cin, STEM_CIN))  # pads the stem's 3 channels only
            scale, shift = fold_bn(*(s[c.bn + "." + f] for f in _BN_FIELDS[:4]))
            self._packed[c.conv] = tuple(t.to(self.device) for t in (w, scale, shift))

    def to(self, device):
        self.device = torch.device(device)
        self._pack()
        return self

    def cuda(self):
        return self.to("cuda")

    def set_compute_dtype(self, dtype):
        if dtype != self.dtype:
            self.dtype = dtype
            self._pack()
        return self

    # ------------------------------------------------------------------ forward
    def _conv(self, x, c, relu, residual=None):
        w, scale, shift = self._packed[c.conv]
        return O.conv2d_nhwc(x, w, stride=c.stride, pad=c.pad, scale=scale, shift=shift, residual=residual, relu=relu)

    def _input(self, x):
        if x.dim() != 4:
            raise ValueError("ResNetTrunk: 4-D pixels expected, got %s" % (tuple(x.shape),))
        x = x.to(self.device)
        if x.dtype == torch.uint8 and x.shape[3] == 3:
            return O.image_to_nhwc(x, self.dtype)
        if not x.dtype.is_floating_point:
            raise ValueError("ResNetTrunk: uint8 [B, H, W, 3] or float pixels expected, got %s %s" % (tuple(x.shape), x.dtype))
        if x.shape[3] == STEM_CIN and x.shape[1] != 3:
            return x.to(self.dtype).contiguous()
        if x.shape[1] == 3:  # the reference's NCHW, already normalised
            out = torch.zeros((x.shape[0], x.shape[2], x.shape[3], STEM_CIN), device=self.device, dtype=self.dtype)
            out[..., :3] = x.permute(0, 2, 3, 1)
            return out
        raise ValueError("ResNetTrunk: [B, H, W, 8] (image_to_nhwc) or NCHW [B, 3, H, W] expected, got %s" % (tuple(x.shape),))

    @torch.no_grad()
    def forward(self, x):
        self._require_weights()
        if self.device.type != "cuda":
            raise O.L.ImtError("ResNetTrunk runs on the GPU (no CPU fallback): call .to('cuda') first")
        x = self._input(x)
        x = O.maxpool2d_nhwc(self._conv(x, self.stem, relu=True))
        for b in self.blocks:
            identity = self._conv(x, b.down, relu=False) if b.down is not None else x
            for c in b.body[:-1]:
                x = self._conv(x, c, relu=True)
            x = self._conv(x, b.body[-1], relu=True, residual=identity)
        B, Ho, Wo, C = x.shape
        return x.view(B, Ho * Wo, C)

    __call__ = forward
