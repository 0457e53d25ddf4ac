#!/usr/bin/env python
"""Per YOLO11 scale (n / s / m / l / x): the localizer network at batch 16 on 640 x 640 (device-resident input) in both operand modes,
ms per image, beside the YOLOv8 and YOLOv5 scale of the same letter measured in the same run (same process, same device, one after the
other: the pool's machines differ by about 3 %), ultralytics' published GFLOPs per image and the share of the fp32 MFMA peak that
follows from them.  Then the two kernels of yolo11.hip alone at batch 16 through the op entry points: time against the time their
input and output bytes take at the project's measured 6.3 TB/s copy rate and, for the attention, the time its FLOPs take at the fp32
MFMA peak.  No target is set for these numbers: the text file is what came out.
   python tools/yolo11_time.py [--scales nsmlx] [--out profiles/yolo11_time.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from effocr_amd import _lib  # noqa: E402
from effocr_amd.localizer_engine import (HipLocalizer, HipLocalizerV8, HipLocalizerV11, init_yolo11_state_dict, init_yolov5_state_dict,  # noqa: E402
                                         init_yolov8_state_dict, yolo11_param_shapes, yolov5_param_shapes, yolov8_param_shapes)

GFLOPS = {"n": 6.5, "s": 21.5, "m": 68.0, "l": 86.9, "x": 194.9}    # ultralytics' published figures for YOLO11 at 640 x 640 (per image)
PEAK_FP32_MFMA = 157.3e12                                           # FLOP/s, MI355X
COPY_RATE = 6.3e12                                                  # B/s, the project's measured device copy rate


def gpu_ms(fn, rounds=5, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    return float(np.median(ts)), float(min(ts))


def measure(engine, sd, x, dev):
    eng = engine(sd, device=dev)
    t32 = gpu_ms(lambda: eng.forward(x))
    eng.set_option("bf16_operands", 1)
    t16 = gpu_ms(lambda: eng.forward(x))
    del eng
    torch.cuda.empty_cache()
    return t32, t16


def kernels_alone(dev, B, lines):
    L = _lib.yolo11_lib()
    stream = _lib.current_stream(dev)
    lines += ["#", f"# the two kernels of yolo11.hip alone, batch {B}, through the op entry points (median of 5 rounds of 50 launches back to back, so a",
              "# launch's share of the queue is inside the figure); bytes = input + output once; attention FLOPs = 2 N^2 (32 + 64) per head",
              f"# {'kernel':<44} {'us':>9} {'us of its bytes at 6.3 TB/s':>28} {'us of its FLOPs at 157.3 TF':>28}"]
    for heads, tag in ((2, "n"), (4, "s / m / l"), (6, "x")):
        N = 400
        qkv = torch.randn(B, N, heads * 128, device=dev)
        out = torch.empty(B, N, heads * 64, device=dev)
        t, _ = gpu_ms(lambda: _lib.yolo11_check(L.effocr_yolo11_op_attention(_lib.ptr(qkv), B, 20, 20, heads, _lib.ptr(out), stream), "op_attention"), reps=50)
        byts, flops = (qkv.numel() + out.numel()) * 4, B * heads * 2 * N * N * 96
        lines.append(f"  {'attention 20x20 heads ' + str(heads) + ' (' + tag + ')':<44} {t * 1e3:>9.1f} {byts / COPY_RATE * 1e6:>28.2f} {flops / PEAK_FP32_MFMA * 1e6:>28.2f}")
        print(lines[-1], flush=True)
    for hw, C, tag in ((20, 128, "attn.pe, n"), (20, 384, "attn.pe, x"), (80, 64, "Detect cv3.0.0.0, n"), (80, 384, "Detect cv3.0.0.0, x"), (20, 768, "Detect cv3.2.0.0, x")):
        x = torch.randn(B, hw, hw, C, device=dev)
        w, b = torch.randn(C, 9, device=dev), torch.randn(C, device=dev)
        out = torch.empty_like(x)
        t, _ = gpu_ms(lambda: _lib.yolo11_check(L.effocr_yolo11_op_dwconv3x3(_lib.ptr(x), B, hw, hw, C, C, _lib.ptr(w), _lib.ptr(b), 1, _lib.ptr(out), C, stream),
                                                "op_dwconv3x3"), reps=50)
        lines.append(f"  {'dwconv3x3 ' + str(hw) + 'x' + str(hw) + ' C=' + str(C) + ' (' + tag + ')':<44} {t * 1e3:>9.1f} {2 * x.numel() * 4 / COPY_RATE * 1e6:>28.2f} {'-':>28}")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", default="nsmlx")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = 16
    x = torch.rand(B, 3, 640, 640, generator=torch.Generator().manual_seed(1)).to(dev)
    mparams = lambda shapes: sum(torch.Size(v).numel() for k, v in shapes.items() if "running_" not in k) / 1e6   # noqa: E731
    lines = [f"# {torch.cuda.get_device_name(0)}; network only, batch {B} on 640 x 640, device-resident input, nc = 2, seeded random weights",
             "# ms per image = (median of 5 rounds of 10 forwards) / 16, (fastest round) in brackets; fp32 = exact fp32 MFMA operands,",
             "# bf16 = bf16-rounded operands (stem, the heads' last 1x1, attention and depthwise kernels fp32); YOLOv8 and YOLOv5 of the same letter",
             "# measured in the same run.  GFLOPs: ultralytics' published figure per image (YOLO11 rows); fp32 share = GFLOPs / fp32 ms / 157.3 TFLOP/s",
             f"# {'scale':<8} {'Mparams':>8} {'fp32 ms/img':>20} {'bf16 ms/img':>20} {'GFLOPs':>8} {'fp32 MFMA share':>16}"]
    for s in a.scales:
        for fam, engine, init, shapes in (("yolo11", HipLocalizerV11, init_yolo11_state_dict, yolo11_param_shapes),
                                          ("yolov8", HipLocalizerV8, init_yolov8_state_dict, yolov8_param_shapes),
                                          ("yolov5", HipLocalizer, init_yolov5_state_dict, yolov5_param_shapes)):
            (t32, t32min), (t16, t16min) = measure(engine, init(2, s, seed=0), x, dev)
            extra = f" {GFLOPS[s]:>8.1f} {GFLOPS[s] * 1e9 / (t32 / B * 1e-3) / PEAK_FP32_MFMA:>16.3f}" if fam == "yolo11" else ""
            lines.append(f"  {fam + s:<8} {mparams(shapes(2, s)):>8.2f} {t32 / B:>11.4f} ({t32min / B:.4f}) {t16 / B:>11.4f} ({t16min / B:.4f}){extra}")
            print(lines[-1], flush=True)
    kernels_alone(dev, B, lines)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
