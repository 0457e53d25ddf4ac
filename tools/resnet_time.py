#!/usr/bin/env python
"""resnet34 / resnet50 encoder + exact k-NN throughput on one GPU, and the FLOP / byte floors of a crop.

  python tools/resnet_time.py [--archs resnet34,resnet50] [--sizes 1,16,1024] [--precisions fp16,bf16,fp32] [--iters 10]

crops/s of Recognizer.neighbors (encoder -> fused L2 normalise -> IP top-10 over a 10 000 x D index), seeded random weights
(init_state_dict(scale="unit")), 224^2 fp32 crops already on the device; CUDA-event time of `iters` back-to-back calls after 3 warm-up
calls.  `frac` = crops/s x convolution FLOPs per crop / the dense 16-bit MFMA peak (2.5 PFLOP/s; fp32 rows against the same peak, whose
own fp32 MFMA peak is 1/16 of it).  The library has no in-library profiler: the per-kernel times come from
`rocprofv3 --kernel-trace --stats -- python tools/resnet_time.py --profile-only` (two 1024-crop forwards per arch and precision)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from effocr_amd import weights as W                    # noqa: E402
from effocr_amd.encoders import ResNetEncoder          # noqa: E402
from effocr_amd.knn import FaissKNN, IndexFlatIP       # noqa: E402
from effocr_amd.pipeline import Recognizer             # noqa: E402

IMG = 224
PEAK16 = 2.5e15


def floors(arch, img=IMG, es=2):
    """(convolution FLOPs, activation bytes the layer-by-layer forward must move) per crop: every conv reads its input and writes its
    output once in the operand type (es bytes), the last conv of a block also reads the residual; the stem reads the fp32 crop, writes
    and reads its 192-column im2col rows; the max pool reads the stem's output and writes a quarter of it."""
    depths, widths, block = W.RESNET_CFG[arch]
    exp = W.resnet_expansion(arch)
    S = img // 2
    flops = 2.0 * 64 * 147 * S * S
    byt = 3 * img * img * 4 + S * S * 192 * es * 2 + S * S * 64 * es       # crop, im2col rows (write + read), stem output
    byt += S * S * 64 * es + (S // 2) ** 2 * 64 * es                        # max pool
    H, cin = S // 2, 64
    for li, (nb, w) in enumerate(zip(depths, widths)):
        for bi in range(nb):
            s = 2 if (bi == 0 and li > 0) else 1
            Ho, cout = H // s, w * exp
            if block == "bottleneck":                                       # (H_in, cin, cout, k, H_out)
                convs = [(H, cin, w, 1, H), (H, w, w, 3, Ho), (Ho, w, cout, 1, Ho)]
            else:
                convs = [(H, cin, w, 3, Ho), (Ho, w, w, 3, Ho)]
            if bi == 0 and (s != 1 or cin != cout):
                convs.append((H, cin, cout, 1, Ho))
            for hi, ci, co, k, ho in convs:
                flops += 2.0 * ci * co * k * k * ho * ho
                byt += (hi * hi * ci + ho * ho * co) * es
            byt += Ho * Ho * cout * es                                      # residual read
            H, cin = Ho, cout
    return flops, byt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--archs", default="resnet34,resnet50")
    ap.add_argument("--sizes", default="1,16,1024")
    ap.add_argument("--precisions", default="fp16,bf16,fp32")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=0, help="effocr_resnet_set_chunk (0 = the library's default)")
    ap.add_argument("--profile-only", action="store_true", help="two 1024-crop forwards per arch and precision, for rocprofv3")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sizes = [int(s) for s in a.sizes.split(",")]
    precs = a.precisions.split(",")
    g = torch.Generator().manual_seed(0)
    x_all = torch.randn(max(sizes + [1024 if a.profile_only else 1]), 3, IMG, IMG, generator=g).to(dev)
    for arch in a.archs.split(","):
        sd = W.init_state_dict(arch, seed=0)
        D = W.embed_dim(arch)
        fl, by = floors(arch)
        if a.profile_only:
            for prec in precs:
                enc = ResNetEncoder(arch, sd, precision=prec, device=dev)
                enc.set_chunk(a.chunk)
                for _ in range(2):
                    enc.forward(x_all[:1024])
                torch.cuda.synchronize(dev)
                enc.check_status()
            continue
        index = torch.nn.functional.normalize(torch.randn(10000, D, generator=g), dim=1)
        chars = [chr(0x4E00 + i) for i in range(10000)]
        print(f"{arch} {IMG}^2: {fl / 1e9:.2f} GFLOP of convolutions per crop; 16-bit activation floor {by / 1e6:.1f} MB per crop; "
              f"encoder + k-NN (10 000 x {D} index, k = 10), {a.iters} calls after 3 warm-up calls, chunk setting {a.chunk}")
        print(f"{'precision':>9} " + " ".join(f"{n:>24}" for n in sizes) + "   (crops/s, ms per call, frac of 2.5 PF)")
        for prec in precs:
            enc = ResNetEncoder(arch, sd, precision=prec, device=dev)
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
                cps = n / ms * 1e3
                cells.append(f"{cps:>8.0f} {ms:>7.2f}ms {cps * fl / PEAK16:>5.3f}".rjust(24))
            print(f"{prec:>9} " + " ".join(cells), flush=True)


if __name__ == "__main__":
    main()
