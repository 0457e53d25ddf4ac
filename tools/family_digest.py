#!/usr/bin/env python
"""sha256 of the embeddings of every encoder-family library at its smallest shapes, one line per case: run it in two trees on one
machine and compare the outputs line for line to show that a change of the host code left every embedding bit-identical.

  python tools/family_digest.py [--out FILE]

Only effocr_amd's public Python API is used (make_encoder, init_state_dict), so the same file runs in any tree that has the families.
Per case: 3 seeded crops, each precision, the default sub-batch and set_chunk(2) (a sub-batch loop with a remainder), with and
without normalize."""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from effocr_amd.encoders import make_encoder           # noqa: E402
from effocr_amd.weights import init_state_dict         # noqa: E402

# the smallest shapes that still take every branch: 64^2 leaves the residual nets a 2x2 last stage (downsample and plain blocks both run)
CASES = [("beit_tiny_test", 32), ("vit8_tiny_test", 16), ("resnet34", 64), ("resnet50", 64), ("resnetv2_50x1_bitm", 64),
         ("mobilenetv3_small_075", 64), ("efficientnet_b0", 64), ("swin_tiny_patch4_window7_224", 224)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for arch, img in CASES:
        sd = init_state_dict(arch, seed=1, img_size=img)
        x = torch.randn(3, 3, img, img, generator=torch.Generator().manual_seed(2)).to(dev)
        for prec in ("bf16", "fp16", "fp32"):
            enc = make_encoder(arch, sd, img_size=img, precision=prec, device=dev)
            for chunk in (0, 2):
                enc.set_chunk(chunk)
                for normalize in (False, True):
                    emb = enc.forward(x, normalize=normalize)
                    enc.check_status()
                    digest = hashlib.sha256(emb.cpu().numpy().tobytes()).hexdigest()
                    lines.append(f"{arch} img={img} {prec} chunk={chunk} normalize={int(normalize)} {digest}")
                    print(lines[-1], flush=True)
            del enc
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
