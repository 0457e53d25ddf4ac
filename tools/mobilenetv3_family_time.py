#!/usr/bin/env python
"""MobileNetV3 family encoder and encoder + exact k-NN throughput on one GPU, with mobilenetv3_small_050 on the merged path
(libeffocr_hip.so) as the yardstick of the same run.

  python tools/mobilenetv3_family_time.py [--archs ...] [--sizes 1,16,64,256,1024] [--precisions fp16,bf16,fp32] [--iters 20]
                                          [--chunk 0] [--one ARCH,PREC,N]

crops/s of the engine's forward alone and of Recognizer.neighbors (encoder -> fused L2 normalise -> IP top-10 over a 10 000 x D index),
seeded random weights (init_state_dict(scale="unit")), 224^2 fp32 crops already on the device.  Every call is timed on its own with a
CUDA-event pair after 3 warm-up calls; the median and the fastest of `iters` calls are reported.  The MAC rate is crops/s x the
multiply-accumulates per crop counted from the builder's block table (weights.mobilenetv3_blocks).

--one ARCH,PREC,N runs a single N-crop forward after one warm-up call and exits: the process to put behind
`rocprofv3 --kernel-trace --stats --` for the per-kernel breakdown (the family's library has no profiler of its own)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from effocr_amd import weights as W                    # noqa: E402
from effocr_amd.encoders import make_encoder           # noqa: E402
from effocr_amd.knn import FaissKNN, IndexFlatIP       # noqa: E402
from effocr_amd.pipeline import Recognizer             # noqa: E402

IMG = 224
YARDSTICK = "mobilenetv3_small_050"
ARCHS = [YARDSTICK, "mobilenetv3_small_075", "mobilenetv3_small_100", "mobilenetv3_large_100"]


def macs_per_crop(arch, img=IMG):
    """Multiply-accumulates of one crop: stem, every block (expand, depthwise, squeeze-excite, project), ConvBnAct, conv_head."""
    stem, blocks, nf = W.mobilenetv3_blocks(arch)
    H = img // 2
    macs = H * H * 27 * stem
    for b in blocks:
        Ho = (H - 1) // b["stride"] + 1
        if b["type"] == "ir":
            macs += H * H * b["cin"] * b["mid"]
        if b["type"] != "cn":
            macs += Ho * Ho * b["mid"] * b["k"] ** 2 + 2 * b["mid"] * b["se"]
        macs += Ho * Ho * (b["cin"] if b["type"] == "cn" else b["mid"]) * b["cout"]
        H = Ho
    return macs + blocks[-1]["cout"] * nf


def time_calls(fn, dev, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--archs", default=",".join(ARCHS))
    ap.add_argument("--sizes", default="1,16,64,256,1024")
    ap.add_argument("--precisions", default="fp16,bf16,fp32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=0, help="set_chunk of the engines (0 = each library's default)")
    ap.add_argument("--one", default="", help="ARCH,PREC,N: one N-crop forward after a warm-up call, then exit (for rocprofv3)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    if a.one:
        arch, prec, n = a.one.split(",")
        enc = make_encoder(arch, W.init_state_dict(arch, seed=0, img_size=IMG), img_size=IMG, precision=prec, device=dev)
        enc.set_chunk(a.chunk)
        x = torch.randn(int(n), 3, IMG, IMG, generator=g).to(dev)
        enc.forward(x)
        torch.cuda.synchronize(dev)
        enc.forward(x)
        enc.check_status()
        print(f"one {n}-crop {prec} forward of {arch} done")
        return
    sizes = [int(s) for s in a.sizes.split(",")]
    x_all = torch.randn(max(sizes), 3, IMG, IMG, generator=g).to(dev)
    chars = [chr(0x4E00 + i) for i in range(10000)]
    print(f"{IMG}^2 crops on the device, chunk setting {a.chunk}, {a.iters} timed calls after 3 warm-up calls, each with its own event pair;")
    print("cells: crops/s from the MEDIAN call (crops/s from the fastest call); k-NN: 10 000 x D index, k = 10")
    rate = {}
    for arch in a.archs.split(","):
        D, macs = W.embed_dim(arch), macs_per_crop(arch)
        sd = W.init_state_dict(arch, seed=0, img_size=IMG)
        index = torch.nn.functional.normalize(torch.randn(10000, D, generator=g), dim=1)
        print(f"\n{arch}: {macs / 1e6:.1f} M MACs per crop, D = {D}")
        print(f"{'':>14} " + " ".join(f"{n:>18}" for n in sizes))
        for prec in a.precisions.split(","):
            enc = make_encoder(arch, sd, img_size=IMG, precision=prec, device=dev)
            enc.set_chunk(a.chunk)
            knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
            knn.train(index)
            rec = Recognizer(enc, knn, chars, knn=10)
            rows = {"encoder": [], "enc+knn": []}
            for n in sizes:
                x = x_all[:n]
                for name, fn in (("encoder", lambda: enc.forward(x)), ("enc+knn", lambda: rec.neighbors(x))):
                    med, best = time_calls(fn, dev, a.iters)
                    rows[name].append(f"{n / med * 1e3:>9.0f} ({n / best * 1e3:>7.0f})")
                    if name == "encoder":
                        rate[(arch, prec, n)] = n / med * 1e3 * macs
                enc.check_status()
            for name, cells in rows.items():
                print(f"{prec:>5} {name:>8} " + " ".join(cells))
            del enc, rec, knn
    nmax = max(sizes)
    print(f"\nMAC rate of the encoder at {nmax} crops (median call), TMAC/s, and its ratio to {YARDSTICK} on the merged path in this run")
    for (arch, prec, n), r in rate.items():
        if n == nmax:
            base = rate.get((YARDSTICK, prec, n))
            print(f"{arch:>24} {prec:>5} {r / 1e12:>8.3f}" + (f"   x{r / base:.2f}" if base else ""))


if __name__ == "__main__":
    main()
