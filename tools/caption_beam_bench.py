#!/usr/bin/env python3
"""Captioning beam search with the object stream on the C3 shape (6L decoder + 6L obj_decoder, d=512, bf16, V=30000):
region features [B,49,2048] + detector features [B,N,1024], one-launch decoder steps (IMT_DECODE_FUSED=1, two launches per
step: one per stack) against the launch-per-operator chain (IMT_DECODE_FUSED=0), and the same search without objects.
Usage: python tools/caption_beam_bench.py [B] [N] [beam] [max_len].  Prints one JSON line per run."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagetranslate_amd.image_model import ImageCaptioning  # noqa: E402
from imagetranslate_amd.seq_gen import BeamDecoder  # noqa: E402
from imagetranslate_amd.textprocessor import SyntheticTextProcessor  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    beam = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    max_len = int(sys.argv[4]) if len(sys.argv) > 4 else 24
    torch.manual_seed(1234)
    m = ImageCaptioning(SyntheticTextProcessor(30000), lang_dec=False, enc_layer=6, dec_layer=6, embed_dim=512, intermediate_dim=2048,
                        use_obj=True, num_attention_heads=8, image_feat_dim=2048)
    m.set_compute_dtype(torch.bfloat16)
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(1234)
    labels = torch.randint(1, 91, (B, N), generator=g)
    xy = torch.rand(B, N, 2, generator=g) * 600
    objects = {"feats": torch.randn(B, N, 1024, generator=g), "boxes": torch.cat([xy, xy + 100], -1), "labels": labels}
    args = dict(images=torch.randn(B, 49, 2048, generator=g), first_tokens=torch.full((B,), 5, dtype=torch.long),
                tgt_langs=torch.ones(B, dtype=torch.long), pad_idx=0)
    for fused, objs in (("1", objects), ("0", objects), ("1", None), ("0", None)):
        os.environ["IMT_DECODE_FUSED"] = fused
        dec = BeamDecoder(m, beam_width=beam, kv_cache=True, sync_every=10 ** 6)  # every step runs: equal work per mode
        dec(max_len=4, objects=objs, **args)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec(max_len=max_len, objects=objs, **args)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"objects": objs is not None, "one_launch": fused == "1", "B": B, "N": N, "beam": beam,
                          "steps": max_len - 1, "ms_per_search": round(1e3 * dt, 2), "ms_per_step": round(1e3 * dt / (max_len - 1), 3)}),
              flush=True)


if __name__ == "__main__":
    main()
