#!/usr/bin/env python
"""mobilenetv3_small_050 encoder and encoder + exact k-NN throughput on one GPU, and the per-kernel roofline of the encoder.

  python tools/mobilenetv3_time.py [--sizes 1,16,64,256,1024] [--precisions fp16,bf16,fp32] [--iters 10]

Part 1: crops/s of HipEncoder.forward alone and of Recognizer.neighbors (encoder -> fused L2 normalise -> IP top-10 over a
10 000 x 1024 index), and the k-NN search alone on the encoder's output, seeded random weights
(init_state_dict(scale="unit")), 224^2 fp32 crops already on the device; CUDA-event time of `iters` back-to-back calls after 3 warm-up calls.
Part 2: the library's own per-launch event profiler (HipEncoder.profile_begin / profile_collect) over one 1024-crop forward per precision:
per kernel class the time, the algorithmic FLOPs / time against 2.5 PFLOP/s (16-bit dense MFMA peak; fp32: 157 TFLOP/s) and the
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

ARCH, IMG = "mobilenetv3_small_050", 224
PEAK = {"fp16": 2.5e15, "bf16": 2.5e15, "fp32": 157e12}
HBM = 8e12


def class_bytes(B, prec):
    """Compulsory bytes per kernel class of one B-crop forward (the workspace layout of api.hip mnv3_forward, fp32 throughout)."""
    S4, S8, t1 = IMG // 4, IMG // 8, (IMG // 4 + 7) // 8
    return {"mnv3_stem_ds": B * (3 * IMG * IMG + S4 * S4 * 16 + t1 * t1 * 16) * 4,
            "mnv3_stage1": B * (S4 * S4 * 16 + S8 * S8 * 16) * 4,
            "mnv3_tail": B * (S8 * S8 * 16 + 288) * 4,
            "mnv3_head": B * (288 + 1024) * 4 + 288 * 1024 * (4 if prec == "fp32" else 2)}


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
    index = torch.nn.functional.normalize(torch.randn(10000, 1024, generator=g), dim=1)
    x_all = torch.randn(max(sizes), 3, IMG, IMG, generator=g).to(dev)
    chars = [chr(0x4E00 + i) for i in range(10000)]
    print(f"chunk setting {a.chunk}")
    print(f"{ARCH} {IMG}^2, {a.iters} calls after 3 warm-up calls; rows: encoder alone, encoder + k-NN (10 000 x 1024 index, k = 10),")
    print("k-NN alone on the encoder's output")
    print(f"{'':>14} " + " ".join(f"{n:>16}" for n in sizes) + "   (crops/s; ms per call)")
    engines = {}
    for prec in precs:
        enc = HipEncoder(ARCH, sd, img_size=IMG, precision=prec, device=dev)
        enc.set_chunk(a.chunk)
        engines[prec] = enc
        knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
        knn.train(index)
        rec = Recognizer(enc, knn, chars, knn=10)
        rows = {"encoder": [], "enc+knn": [], "knn": []}
        for n in sizes:
            x = x_all[:n]
            emb = enc.forward(x, normalize=True)
            for name, fn in (("encoder", lambda: enc.forward(x)), ("enc+knn", lambda: rec.neighbors(x)),
                             ("knn", lambda: knn.index.search_device(emb, 10))):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize(dev)
                ms = e0.elapsed_time(e1) / a.iters
                rows[name].append(f"{n / ms * 1e3:>7.0f} {ms:>6.3f}ms".rjust(16))
            enc.check_status()
        for name, cells in rows.items():
            print(f"{prec:>5} {name:>8} " + " ".join(cells))
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
