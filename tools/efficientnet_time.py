#!/usr/bin/env python
"""EfficientNet-B0 encoder and encoder + exact k-NN throughput on one GPU, with mobilenetv3_large_100 (libeffocr_mnv3.so, the path this
network's kernels were built to beat) as the yardstick of the same run.

  python tools/efficientnet_time.py [--archs ...] [--sizes 1,16,64,256,1024] [--precisions fp16,bf16,fp32] [--iters 20]
                                    [--chunk 0] [--one ARCH,PREC,N]

crops/s of the engine's forward alone and of Recognizer.neighbors (encoder -> fused L2 normalise -> IP top-10 over a 10 000 x 1280 index),
seeded random weights (init_state_dict(scale="unit")), 224^2 fp32 crops already on the device.  Every call is timed on its own with a
CUDA-event pair after 3 warm-up calls; the median and the fastest of `iters` calls are reported.  The MAC rate is crops/s x the
multiply-accumulates per crop counted from the builder's block table (weights.efficientnet_blocks).  The smaller call sizes are timed in
every precision too, but the yardstick (timed at the largest size only, every precision) is what the MAC rates are compared with.

--one ARCH,PREC,N runs two N-crop forwards after one warm-up call and exits: the process to put behind
`rocprofv3 --kernel-trace --stats --` for the per-kernel breakdown (the library has no profiler of its own)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from effocr_amd import weights as W                    # noqa: E402

IMG = 224
YARDSTICK = "mobilenetv3_large_100"
ARCHS = ["efficientnet_b0", "tf_efficientnet_b0"]


def macs_per_crop(arch, img=IMG):
    """Multiply-accumulates of one crop: stem, every block (expand, depthwise, squeeze-excite, project), conv_head (the ConvBnAct and
    conv_head of a MobileNetV3 when ``arch`` is the yardstick)."""
    if W.is_mobilenetv3(arch):
        stem, blocks, nf = W.mobilenetv3_blocks(arch)
    else:
        stem, blocks, nf = W.efficientnet_blocks(arch)
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
    if W.is_mobilenetv3(arch):
        return macs + blocks[-1]["cout"] * nf              # conv_head after the pool
    return macs + H * H * blocks[-1]["cout"] * nf          # conv_head on every pixel of the last map, before the pool


def compulsory_bytes_per_crop(arch, img=IMG):
    """HBM bytes one crop cannot avoid with fp32 activations kept in HBM between launches: every launch's input read once and its output
    written once (the residual input a second time), weights not counted (they stay in cache across crops)."""
    stem, blocks, nf = W.efficientnet_blocks(arch)
    H = img // 2
    n = 3 * img * img + H * H * stem
    for b in blocks:
        Ho = (H - 1) // b["stride"] + 1
        if b["type"] == "ir":
            n += H * H * (b["cin"] + b["mid"])             # expand: read the block input, write the expansion
        n += H * H * b["mid"] + Ho * Ho * b["mid"]         # depthwise: read, write
        n += Ho * Ho * (b["mid"] + b["cout"] + (b["cout"] if b["res"] else 0))    # project: read (x gate), write, residual
        H = Ho
    n += H * H * (blocks[-1]["cout"] + nf) + H * H * nf + nf                      # conv_head, pool
    return 4 * n


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
    from effocr_amd.encoders import make_encoder
    from effocr_amd.knn import FaissKNN, IndexFlatIP
    from effocr_amd.pipeline import Recognizer
    ap = argparse.ArgumentParser()
    ap.add_argument("--archs", default=",".join(ARCHS))
    ap.add_argument("--sizes", default="1,16,64,256,1024")
    ap.add_argument("--precisions", default="fp16,bf16,fp32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=0, help="set_chunk of the engines (0 = each library's default)")
    ap.add_argument("--one", default="", help="ARCH,PREC,N: two N-crop forwards after a warm-up call, then exit (for rocprofv3)")
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
        enc.forward(x)
        enc.check_status()
        print(f"two {n}-crop {prec} forwards of {arch} done (after one warm-up forward)")
        return
    sizes = [int(s) for s in a.sizes.split(",")]
    nmax = max(sizes)
    x_all = torch.randn(nmax, 3, IMG, IMG, generator=g).to(dev)
    chars = [chr(0x4E00 + i) for i in range(10000)]
    print(f"{IMG}^2 crops on the device, chunk setting {a.chunk}, {a.iters} timed calls after 3 warm-up calls, each with its own event pair;")
    print("cells: crops/s from the MEDIAN call (crops/s from the fastest call); k-NN: 10 000 x D index, k = 10; one run on one box")
    rate = {}
    for arch in [YARDSTICK] + a.archs.split(","):
        D, macs = W.embed_dim(arch), macs_per_crop(arch)
        sd = W.init_state_dict(arch, seed=0, img_size=IMG)
        index = torch.nn.functional.normalize(torch.randn(10000, D, generator=g), dim=1)
        yard = arch == YARDSTICK
        print(f"\n{arch}{' (yardstick, existing path)' if yard else ''}: {macs / 1e6:.1f} M MACs per crop, D = {D}"
              + ("" if yard else f", {compulsory_bytes_per_crop(arch) / 1e6:.1f} MB of compulsory activation traffic per crop"))
        these = [nmax] if yard else sizes
        print(f"{'':>14} " + " ".join(f"{n:>18}" for n in these))
        for prec in a.precisions.split(","):
            enc = make_encoder(arch, sd, img_size=IMG, precision=prec, device=dev)
            enc.set_chunk(a.chunk)
            knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
            knn.train(index)
            rec = Recognizer(enc, knn, chars, knn=10)
            rows = {"encoder": [], "enc+knn": []}
            for n in these:
                x = x_all[:n]
                for name, fn in (("encoder", lambda: enc.forward(x)), ("enc+knn", lambda: rec.neighbors(x))):
                    med, best = time_calls(fn, dev, a.iters)
                    rows[name].append(f"{n / med * 1e3:>9.0f} ({n / best * 1e3:>7.0f})")
                    if name == "encoder":
                        rate[(arch, prec, n)] = n / med * 1e3
                enc.check_status()
            for name, cells in rows.items():
                print(f"{prec:>5} {name:>8} " + " ".join(cells))
            del enc, rec, knn
    print(f"\nencoder at {nmax} crops (median call): crops/s, TMAC/s, ratio to {YARDSTICK}'s TMAC/s in this run, compulsory TB/s and its "
          "fraction of 8 TB/s")
    for (arch, prec, n), r in rate.items():
        if n != nmax:
            continue
        t = r * macs_per_crop(arch)
        base = rate.get((YARDSTICK, prec, n))
        line = f"{arch:>24} {prec:>5} {r:>9.0f} {t / 1e12:>8.3f}"
        if arch != YARDSTICK:
            bw = r * compulsory_bytes_per_crop(arch)
            line += (f"   x{t / (base * macs_per_crop(YARDSTICK)):.2f}" if base else "") + f"   {bw / 1e12:.3f} TB/s ({bw / 8e12:.1%})"
        print(line)


if __name__ == "__main__":
    main()
