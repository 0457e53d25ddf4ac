#!/usr/bin/env python
"""convnext_tiny encoder + exact k-NN throughput on one GPU, and the per-kernel roofline of the encoder.

  python tools/convnext_time.py [--sizes 1,16,64,256,1024] [--precisions fp16,bf16,fp32] [--iters 10]

Part 1: crops/s of Recognizer.neighbors (encoder -> fused L2 normalise -> IP top-10 over a 10 000 x 768 index), seeded random weights
(init_state_dict(scale="unit")), 224^2 fp32 crops already on the device; CUDA-event time of `iters` back-to-back calls after 3 warm-up calls.
Part 2: the library's own per-launch event profiler (HipEncoder.profile_begin / profile_collect) over one 1024-crop forward per precision:
per kernel class the time, the executed FLOPs / time against 2.5 PFLOP/s (16-bit dense MFMA peak; fp32 MFMA: 157 TFLOP/s) and the
compulsory bytes (each operand read once, each result written once) / time against 8 TB/s."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from effocr_amd import weights as W                    # noqa: E402
from effocr_amd.encoders import HipEncoder             # noqa: E402
from effocr_amd.knn import FaissKNN, IndexFlatIP       # noqa: E402
from effocr_amd.pipeline import Recognizer             # noqa: E402

ARCH, IMG = "convnext_tiny", 224
PEAK = {"fp16": 2.5e15, "bf16": 2.5e15, "fp32": 157e12}
HBM = 8e12


def class_bytes(B, prec):
    """Compulsory bytes per kernel class of one B-crop forward (the layout of api.hip convnext_forward)."""
    es = 4 if prec == "fp32" else 2
    depths, widths = W.CONVNEXT_CFG[ARCH]
    cps = [(c + 127) // 128 * 128 for c in widths]
    out = {}

    def add(k, v):
        out[k] = out.get(k, 0.0) + v
    H = IMG // 4
    add("cnx_stem", B * 3 * IMG * IMG * 4 + B * H * H * cps[0] * 4)
    for i, (d, c) in enumerate(zip(depths, widths)):
        cp = cps[i]
        if i > 0:
            M0 = B * H * H
            add("cnx_ln_s2d", M0 * cps[i - 1] * 4 + M0 * widths[i - 1] * es)
            H //= 2
            add("cnx_downsample", M0 * widths[i - 1] * es + cp * 4 * widths[i - 1] * es + B * H * H * cp * 4)
        M = B * H * H
        add("cnx_dwconv_ln", d * (M * cp * 4 + M * cp * es))
        add("cnx_fc1_gelu", d * (M * cp * es + 4 * c * cp * es + M * 4 * c * es))
        add("cnx_fc2_scale_resid", d * (M * 4 * c * es + cp * 4 * c * es + 2 * M * cp * 4))
    add("cnx_head", B * H * H * cps[3] * 4 + B * widths[3] * 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,64,256,1024")
    ap.add_argument("--precisions", default="fp16,bf16,fp32")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=0, help="effocr_encoder_set_chunk (0 = the library's default)")
    ap.add_argument("--no-profile", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sizes = [int(s) for s in a.sizes.split(",")]
    precs = a.precisions.split(",")
    sd = W.init_state_dict(ARCH, seed=0, img_size=IMG)
    g = torch.Generator().manual_seed(0)
    index = torch.nn.functional.normalize(torch.randn(10000, 768, generator=g), dim=1)
    x_all = torch.randn(max(sizes), 3, IMG, IMG, generator=g).to(dev)
    chars = [chr(0x4E00 + i) for i in range(10000)]
    print(f"chunk setting {a.chunk}")
    print(f"{ARCH} {IMG}^2, encoder + k-NN (10 000 x 768 index, k = 10), {a.iters} calls after 3 warm-up calls")
    print(f"{'precision':>9} " + " ".join(f"{n:>12}" for n in sizes) + "   (crops/s; ms per call)")
    engines = {}
    for prec in precs:
        enc = HipEncoder(ARCH, sd, img_size=IMG, precision=prec, device=dev)
        enc.set_chunk(a.chunk)
        engines[prec] = enc
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
            cells.append(f"{n / ms * 1e3:>7.0f} {ms:>6.2f}ms".rjust(12) if n >= 256 else f"{n / ms * 1e3:>6.0f} {ms:>5.2f}ms".rjust(12))
        print(f"{prec:>9} " + " ".join(cells))
    B = 1024 if 1024 in sizes else max(sizes)
    for prec, enc in ([] if a.no_profile else engines.items()):
        x = x_all[:B]
        enc.forward(x)
        torch.cuda.synchronize(dev)
        enc.profile_begin()
        enc.forward(x)
        prof = enc.profile_collect()
        nb = class_bytes(B, prec)
        tot = sum(v["ms"] for v in prof.values())
        print(f"\nper kernel class, {prec}, one {B}-crop forward (library event profiler: {tot:.2f} ms, {B / tot * 1e3:.0f} crops/s encoder only)")
        print(f"{'class':>22} {'launches':>8} {'ms':>8} {'share':>6} {'TFLOP/s':>8} {'of peak':>7} {'GB':>7} {'TB/s':>6} {'of 8TB/s':>8}")
        for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]):
            tf = v["flops"] / (v["ms"] * 1e-3) / 1e12 if v["ms"] > 0 else 0.0
            gb = nb.get(k, 0.0) / 1e9
            tbs = gb / (v["ms"] * 1e-3) / 1e3 if v["ms"] > 0 else 0.0
            print(f"{k:>22} {v['launches']:>8} {v['ms']:>8.3f} {v['ms'] / tot:>6.1%} {tf:>8.1f} {tf * 1e12 / PEAK[prec]:>7.1%} {gb:>7.2f} {tbs:>6.2f} {tbs * 1e12 / HBM:>8.1%}")


if __name__ == "__main__":
    main()
