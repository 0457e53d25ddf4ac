#!/usr/bin/env python
"""beit_base_patch16_224 encoder + exact k-NN throughput on one GPU, with vit_base_patch16_224 in the same run.

  python tools/beit_time.py [--sizes 16,1024] [--precisions fp16,bf16,fp32] [--iters 10]

crops/s of Recognizer.neighbors (encoder -> fused L2 normalise -> IP top-10 over a 10 000 x 768 index), seeded random weights
(init_state_dict(scale="unit")), 224^2 fp32 crops already on the device; CUDA-event time of `iters` back-to-back calls after 3 warm-up
calls.  Both networks cost 17.6 GMAC per crop; ViT-B runs the fused kernels of libeffocr_hip.so, BEiT one kernel per operator, and the
last column is the ratio of their rates.  The BEiT library has no in-library profiler: the kernel breakdown comes from
`rocprofv3 --kernel-trace --stats` over `--profile-only` (one warm-up and one timed 1024-crop forward per precision, nothing else)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from effocr_amd import weights as W                    # noqa: E402
from effocr_amd.encoders import make_encoder           # noqa: E402
from effocr_amd.knn import FaissKNN, IndexFlatIP       # noqa: E402
from effocr_amd.pipeline import Recognizer             # noqa: E402

BEIT, VIT, IMG = "beit_base_patch16_224", "vit_base_patch16_224", 224


def rate(rec, enc, x, iters, dev):
    for _ in range(3):
        rec.neighbors(x)
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        rec.neighbors(x)
    e1.record()
    torch.cuda.synchronize(dev)
    enc.check_status()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,1024")
    ap.add_argument("--precisions", default="fp16,bf16,fp32")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--profile-only", action="store_true", help="two 1024-crop BEiT forwards per precision, for rocprofv3")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sizes = [int(s) for s in a.sizes.split(",")]
    precs = a.precisions.split(",")
    g = torch.Generator().manual_seed(0)
    x_all = torch.randn(max(sizes), 3, IMG, IMG, generator=g).to(dev)
    if a.profile_only:
        sd = W.init_state_dict(BEIT, seed=0)
        for prec in precs:
            enc = make_encoder(BEIT, sd, precision=prec, device=dev)
            for _ in range(2):
                enc.forward(x_all)
            torch.cuda.synchronize(dev)
            enc.check_status()
        return
    index = torch.nn.functional.normalize(torch.randn(10000, 768, generator=g), dim=1)
    chars = [chr(0x4E00 + i) for i in range(10000)]
    print(f"{IMG}^2 crops, encoder + k-NN (10 000 x 768 index, k = 10), {a.iters} calls after 3 warm-up calls (crops/s; ms per call)")
    print(f"{'precision':>9} {'crops':>6} {BEIT:>28} {VIT:>28} {'BEiT / ViT-B':>13}")
    for prec in precs:
        ms = {}
        for arch in (BEIT, VIT):
            enc = make_encoder(arch, W.init_state_dict(arch, seed=0), precision=prec, device=dev)
            knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
            knn.train(index)
            rec = Recognizer(enc, knn, chars, knn=10)
            for n in sizes:
                ms[arch, n] = rate(rec, enc, x_all[:n], a.iters, dev)
            del rec, enc
        for n in sizes:
            cells = [f"{n / ms[arch, n] * 1e3:>9.0f} {ms[arch, n]:>9.2f} ms".rjust(28) for arch in (BEIT, VIT)]
            print(f"{prec:>9} {n:>6} " + " ".join(cells) + f" {ms[VIT, n] / ms[BEIT, n]:>13.3f}", flush=True)


if __name__ == "__main__":
    main()
