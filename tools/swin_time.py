#!/usr/bin/env python
"""swin_tiny_patch4_window7_224 encoder + exact k-NN throughput on one GPU.

  python tools/swin_time.py [--sizes 16,1024] [--precisions fp16,bf16] [--iters 10]

crops/s of Recognizer.neighbors (encoder -> fused L2 normalise -> IP top-10 over a 10 000 x 768 index), seeded random weights
(init_state_dict(scale="unit")), 224^2 fp32 crops already on the device; CUDA-event time of `iters` back-to-back calls after 3 warm-up
calls.  The Swin library has no in-library profiler: the kernel breakdown comes from `rocprofv3 --kernel-trace --stats` over
`--profile-only` (one warm-up and one timed 1024-crop forward per precision, nothing else)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from effocr_amd import weights as W                    # noqa: E402
from effocr_amd.encoders import SwinEncoder            # noqa: E402
from effocr_amd.knn import FaissKNN, IndexFlatIP       # noqa: E402
from effocr_amd.pipeline import Recognizer             # noqa: E402

ARCH, IMG = "swin_tiny_patch4_window7_224", 224


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,1024")
    ap.add_argument("--precisions", default="fp16,bf16")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=0, help="effocr_swin_set_chunk (0 = the library's default)")
    ap.add_argument("--profile-only", action="store_true", help="two 1024-crop forwards per precision, for rocprofv3")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sizes = [int(s) for s in a.sizes.split(",")]
    precs = a.precisions.split(",")
    sd = W.init_state_dict(ARCH, seed=0)
    g = torch.Generator().manual_seed(0)
    x_all = torch.randn(max(sizes), 3, IMG, IMG, generator=g).to(dev)
    if a.profile_only:
        for prec in precs:
            enc = SwinEncoder(ARCH, sd, precision=prec, device=dev)
            enc.set_chunk(a.chunk)
            for _ in range(2):
                enc.forward(x_all)
            torch.cuda.synchronize(dev)
            enc.check_status()
        return
    index = torch.nn.functional.normalize(torch.randn(10000, 768, generator=g), dim=1)
    chars = [chr(0x4E00 + i) for i in range(10000)]
    print(f"chunk setting {a.chunk}")
    print(f"{ARCH} {IMG}^2, encoder + k-NN (10 000 x 768 index, k = 10), {a.iters} calls after 3 warm-up calls")
    print(f"{'precision':>9} " + " ".join(f"{n:>16}" for n in sizes) + "   (crops/s; ms per call)")
    for prec in precs:
        enc = SwinEncoder(ARCH, sd, precision=prec, device=dev)
        enc.set_chunk(a.chunk)
        knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
        knn.train(index)
        rec = Recognizer(enc, knn, chars, knn=10)
        cells = []
        for n in sizes:
            x = x_all[:n]
            for _ in range(3):
                rec.neighbors(x)
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                rec.neighbors(x)
            e1.record()
            torch.cuda.synchronize(dev)
            enc.check_status()
            ms = e0.elapsed_time(e1) / a.iters
            cells.append(f"{n / ms * 1e3:>7.0f} {ms:>7.2f}ms".rjust(16))
        print(f"{prec:>9} " + " ".join(cells), flush=True)


if __name__ == "__main__":
    main()
