"""The frozen ResNet trunk at B = 32, 224 x 224, depth 1 (resnet18) and depth 3 (resnet50), bf16 and fp32:
  * every distinct convolution shape of the trunk: imt_conv2d with its whole epilogue (device-event median, FLOP/s from
    2 M N K), next to imt_gemm NT on the same (M, N, K) and torch.nn.functional.conv2d (channels-last) on the same shape;
  * the whole trunk against the same chain of torch operators (conv2d, batch_norm, relu, max_pool2d, add; channels-last);
  * images per second of extract_features on generated JPEGs (decode and preprocessing on the host included).
Nothing is gated on these numbers.  torch runs with cudnn.benchmark off, i.e. MIOpen's immediate mode.
Usage: python tools/trunk_bench.py OUT.json [timed calls] [images]"""
import json
import os
import statistics
import sys
import tempfile
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagetranslate_amd import extract_features as E  # noqa: E402
from imagetranslate_amd import hip_ops as O  # noqa: E402
from imagetranslate_amd.resnet import ResNetTrunk, trunk_plan, trunk_shapes  # noqa: E402
from tools.caption2image_bench import _stats, _timed  # noqa: E402

B, SIDE = 32, 224
DTYPES = ((torch.bfloat16, "bf16"), (torch.float32, "fp32"))


def random_state(depth, seed=0):
    """He-normal convolutions, BatchNorm statistics near identity (the generator of tests/resnet_oracle.py)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in trunk_shapes(depth).items():
        if key.endswith("num_batches_tracked"):
            sd[key] = torch.tensor(0)
        elif len(shape) == 4:
            sd[key] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        elif key.endswith(("running_var", ".weight")):
            sd[key] = torch.rand(shape, generator=g) + 0.5
        else:
            sd[key] = torch.rand(shape, generator=g) * 0.4 - 0.2
    return sd


def conv_shapes(depth):
    """Distinct (H, W, Cin, Cout, k, stride, pad, residual) of the trunk's launches at SIDE x SIDE, in order, with their counts."""
    stem, blocks = trunk_plan(depth)
    seen, side = {}, SIDE

    def add(c, side, residual):
        key = (side, side, max(c.cin, 8), c.cout, c.k, c.stride, c.pad, residual)
        seen[key] = seen.get(key, 0) + 1
        return (side + 2 * c.pad - c.k) // c.stride + 1
    side = add(stem, side, False)
    side = (side - 1) // 2 + 1
    for b in blocks:
        if b.down is not None:
            add(b.down, side, False)
        for c in b.body[:-1]:
            side = add(c, side, False)
        side = add(b.body[-1], side, True)
    return seen


def torch_trunk(sd, depth, x):
    """The same chain as torch operators on a channels-last NCHW tensor."""
    stem, blocks = trunk_plan(depth)

    def cbr(x, c, relu, residual=None):
        y = F.conv2d(x, sd[c.conv + ".weight"], stride=c.stride, padding=c.pad)
        y = F.batch_norm(y, sd[c.bn + ".running_mean"], sd[c.bn + ".running_var"], sd[c.bn + ".weight"], sd[c.bn + ".bias"], False, 0.0, 1e-5)
        if residual is not None:
            y = y + residual
        return F.relu(y) if relu else y
    x = F.max_pool2d(cbr(x, stem, True), 3, 2, 1)
    for b in blocks:
        identity = cbr(x, b.down, False) if b.down is not None else x
        for c in b.body[:-1]:
            x = cbr(x, c, True)
        x = cbr(x, b.body[-1], True, identity)
    return x.flatten(2).permute(0, 2, 1)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "trunk.json"
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    n_images = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    layers, trunks = [], []
    for depth in (1, 3):
        sd = random_state(depth)
        for dtype, name in DTYPES:
            for (H, W, cin, cout, k, stride, pad, residual), count in conv_shapes(depth).items():
                x = torch.randn(B, H, W, cin, device=dev).to(dtype)
                w = (torch.randn(cout, k, k, cin, generator=g) * (2.0 / (cin * k * k)) ** 0.5).to(dev, dtype)
                scale, shift = torch.rand(cout, generator=g).to(dev) + 0.5, torch.rand(cout, generator=g).to(dev)
                Ho, Wo = O.conv_out_size(H, k, stride, pad), O.conv_out_size(W, k, stride, pad)
                M, N, K = B * Ho * Wo, cout, k * k * cin
                res = torch.randn(B, Ho, Wo, cout, device=dev).to(dtype) if residual else None
                y = torch.empty(B, Ho, Wo, cout, device=dev, dtype=dtype)
                a, bm = torch.randn(M, K, device=dev).to(dtype), w.view(cout, K)
                c = torch.empty(M, N, device=dev, dtype=dtype)
                xt = x.permute(0, 3, 1, 2)  # NCHW view of NHWC memory = channels-last
                wt = w.permute(0, 3, 1, 2)
                ours = lambda: O.conv2d_nhwc(x, w, stride=stride, pad=pad, scale=scale, shift=shift, residual=res, relu=True, out=y)
                gemm = lambda: O.gemm(a, bm, O.IMT_NT, out=c)
                tconv = lambda: F.conv2d(xt, wt, stride=stride, padding=pad)
                t_ours, t_gemm, t_torch = _timed([ours, gemm, tconv], calls, warmup=3)
                flops = 2.0 * M * N * K
                tf = lambda ms: round(flops / statistics.median(ms) / 1e9, 2)
                layers.append({"depth": depth, "dtype": name, "launches_per_forward": count,
                               "shape": {"H": H, "W": W, "Cin": cin, "Cout": cout, "k": k, "stride": stride, "pad": pad, "residual": residual},
                               "M": M, "N": N, "K": K,
                               "imt_conv2d": dict(_stats(t_ours), tflops=tf(t_ours)),
                               "imt_gemm_same_mnk": dict(_stats(t_gemm), tflops=tf(t_gemm)),
                               "torch_conv2d_channels_last": dict(_stats(t_torch), tflops=tf(t_torch)),
                               "conv_rate_over_gemm_rate": round(statistics.median(t_gemm) / statistics.median(t_ours), 3)})
            trunk = ResNetTrunk(depth, dtype).load_state_dict(sd).cuda()
            px = torch.randn(B, SIDE, SIDE, 8, device=dev)
            px[..., 3:] = 0
            px = px.to(dev, dtype)
            tsd = {k: v.to(dev, dtype).contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v.to(dev, torch.float32)
                   for k, v in sd.items()}
            pt = px[..., :3].permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
            with torch.no_grad():
                t_ours, t_torch = _timed([lambda: trunk(px), lambda: torch_trunk(tsd, depth, pt)], calls, warmup=3)
            total = sum(2.0 * r["M"] * r["N"] * r["K"] * r["launches_per_forward"] for r in layers if r["depth"] == depth and r["dtype"] == name)
            trunks.append({"depth": depth, "dtype": name, "B": B, "flop": total,
                           "resnet_trunk": dict(_stats(t_ours), tflops=round(total / statistics.median(t_ours) / 1e9, 2),
                                                images_per_s=round(B / statistics.median(t_ours) * 1e3, 1)),
                           "torch_ops": dict(_stats(t_torch), tflops=round(total / statistics.median(t_torch) / 1e9, 2)),
                           "speedup_median_vs_torch_ops": round(statistics.median(t_torch) / statistics.median(t_ours), 3)})
    # extract_features end to end on generated JPEGs
    from PIL import Image
    extract = []
    with tempfile.TemporaryDirectory() as d:
        for i in range(n_images):
            arr = torch.randint(0, 256, (12, 16, 3), generator=g, dtype=torch.uint8).numpy()
            Image.fromarray(arr, "RGB").resize((320, 240), Image.BILINEAR).save(os.path.join(d, "img%04d.jpg" % i))
        paths = E.list_images(d)
        for depth in (1, 3):
            trunk = ResNetTrunk(depth).load_state_dict(random_state(depth))
            for dtype, name in DTYPES:
                E.extract(trunk, d, paths[:64], batch=64, dtype=dtype)  # warm-up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                feats = E.extract(trunk, d, paths, batch=64, dtype=dtype)
                dt = time.perf_counter() - t0
                extract.append({"depth": depth, "dtype": name, "images": len(paths), "batch": 64, "seconds": round(dt, 3),
                                "images_per_s": round(len(paths) / dt, 1), "feats": list(feats.shape)})
    res = {"bench": "trunk", "device": torch.cuda.get_device_name(0), "layers": layers, "trunk": trunks, "extract_features": extract,
           "method": "device events, medians, the paths alternating in one process after warm-up rounds; extract_features by wall clock",
           "workload": "frozen ResNet trunk, B = 32, 224 x 224; imt_conv2d timed with its scale / shift / residual / ReLU epilogue"}
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fw:
        fw.write(text + "\n")


if __name__ == "__main__":
    main()
