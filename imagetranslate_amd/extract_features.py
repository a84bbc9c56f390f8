"""Region features from pixels: ``python -m imagetranslate_amd.extract_features --images DIR (--trunk FILE | --model DIR)
--output DIR/features.pt`` writes the ``features.pt`` that ``dataset.RegionFeatures`` reads, i.e. what the reference computes
per batch with its frozen ``ModifiedResnet`` (``src/image_model.py:24-36``) from the images its datasets load
(``src/dataset.py:283-289,366-373``).  A frozen trunk's output is a constant of the image, so extracting once loses nothing.

Host (PIL, a small thread pool that decodes the next batch while the GPU runs this one): convert to RGB, bilinear resize so
that the shorter side is 256 and the longer ``int(256 * long / short)``, centre crop 224 at ``int(round((size - 224) / 2))``;
an unreadable image becomes a black one with a warning.  Device: ``imt_image_nhwc`` (ToTensor + Normalize), then
``resnet.ResNetTrunk`` on the MFMA convolution kernels, bf16 unless ``--fp32``.  ``feats`` is stored fp32 ``[n, 49, C]``
beside ``paths`` (relative to DIR, as ``RegionFeatures`` looks them up); the file is written to a temporary name and renamed.
"""
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from optparse import OptionParser

import torch

from . import hip_ops as O
from .resnet import ResNetTrunk

RESIZE, CROP = 256, 224
EXTENSIONS = (".jpg", ".jpeg", ".png")
MAX_WORKERS = 8


def resize_size(w, h, size=RESIZE):
    """(width, height) after transforms.Resize(size) of a (w, h) image: shorter side to size, longer to int(size * long / short)."""
    if w <= h:
        return size, int(size * h / w)
    return int(size * w / h), size


def crop_offset(w, h, size=CROP):
    """(left, top) of transforms.CenterCrop(size) in a (w, h) image."""
    return int(round((w - size) / 2.0)), int(round((h - size) / 2.0))


def preprocess(img):
    """PIL image -> uint8 [224, 224, 3] (RGB, resized, centre-cropped)."""
    import numpy as np
    from PIL import Image
    img = img.convert("RGB")  # no RGBA or greyscale past this point (src/dataset.py:367-368)
    img = img.resize(resize_size(*img.size), Image.BILINEAR)
    left, top = crop_offset(*img.size)
    img = img.crop((left, top, left + CROP, top + CROP))
    return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy())


def load_image(root, path):
    from PIL import Image
    try:
        with Image.open(os.path.join(root, path)) as im:
            return preprocess(im)
    except Exception as e:  # the reference's bare except (src/dataset.py:371-373)
        print("Corrupted image %s (%s): a black image takes its place" % (path, type(e).__name__), file=sys.stderr)
        return torch.zeros((CROP, CROP, 3), dtype=torch.uint8)


def list_images(root, list_file=None):
    """Paths relative to ``root``: the lines of ``list_file``, or every *.jpg / *.jpeg / *.png below root, sorted."""
    if list_file is not None:
        with open(list_file, "r") as fp:
            return [ln.strip() for ln in fp if ln.strip()]
    found = []
    for d, _, files in os.walk(root):
        found += [os.path.relpath(os.path.join(d, f), root) for f in files if f.lower().endswith(EXTENSIONS)]
    return sorted(found)


def load_trunk(trunk_file=None, model_dir=None, depth=1):
    """The trunk from a torchvision-format state dict (``depth`` says which ResNet), or from a checkpoint directory whose
    state dict carries it under ``image_model.*`` (its mt_config says the depth)."""
    if (trunk_file is None) == (model_dir is None):
        raise ValueError("extract_features: give exactly one of --trunk FILE and --model DIR")
    if trunk_file is not None:
        return ResNetTrunk(depth).load_state_dict(torch.load(trunk_file, map_location="cpu", weights_only=True))
    from .safe_pickle import load_mt_config
    depth = load_mt_config(os.path.join(model_dir, "mt_config"))[7]
    sd = torch.load(os.path.join(model_dir, "mt_model.state_dict"), map_location="cpu", weights_only=True)
    pre = "image_model."
    if pre + "conv1.weight" not in sd:
        raise ValueError("extract_features: the checkpoint in %s carries no CNN trunk (no %sconv1.weight)" % (model_dir, pre))
    return ResNetTrunk(depth).load_state_dict(sd, prefix=pre)


@torch.no_grad()
def extract(trunk, root, paths, batch=64, dtype=torch.bfloat16, device="cuda"):
    """fp32 [len(paths), regions, C] on the host."""
    trunk.to(device).set_compute_dtype(dtype)
    out = []
    chunks = [paths[i:i + batch] for i in range(0, len(paths), batch)]
    with ThreadPoolExecutor(max_workers=max(1, min(MAX_WORKERS, batch))) as pool:
        decode = lambda chunk: [pool.submit(load_image, root, p) for p in chunk]  # noqa: E731
        pending = decode(chunks[0]) if chunks else []
        for i in range(len(chunks)):
            pixels = torch.stack([f.result() for f in pending])
            pending = decode(chunks[i + 1]) if i + 1 < len(chunks) else []  # decoded while the GPU runs this batch
            out.append(trunk(O.image_to_nhwc(pixels.to(device), dtype)).float().cpu())
    if not out:
        return torch.zeros((0, (CROP // 32) ** 2, trunk.out_channels), dtype=torch.float32)
    return torch.cat(out)


def write_features(path, paths, feats):
    tmp = path + ".tmp.%d" % os.getpid()
    try:
        torch.save({"paths": list(paths), "feats": feats}, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def get_option_parser():
    parser = OptionParser()
    for flag, dest, kind, default in (("--images", "images", "string", None), ("--list", "list", "string", None),
                                      ("--trunk", "trunk", "string", None), ("--model", "model", "string", None),
                                      ("--depth", "depth", "int", 1), ("--output", "output", "string", None),
                                      ("--batch", "batch", "int", 64)):
        parser.add_option(flag, dest=dest, type=kind, default=default)
    parser.add_option("--fp32", action="store_true", dest="fp32", default=False)
    return parser


def main(argv=None):
    options, _ = get_option_parser().parse_args(argv)
    if options.images is None or options.output is None:
        raise SystemExit("extract_features: --images DIR and --output FILE are required")
    trunk = load_trunk(options.trunk, options.model, options.depth)
    paths = list_images(options.images, options.list)
    feats = extract(trunk, options.images, paths, batch=options.batch, dtype=torch.float32 if options.fp32 else torch.bfloat16)
    write_features(options.output, paths, feats)
    print("Extracted %s region features of %d images into %s" % (tuple(feats.shape[1:]), len(paths), options.output))


if __name__ == "__main__":
    main()
