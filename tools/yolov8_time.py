#!/usr/bin/env python
"""Per YOLOv8 scale (n / s / m / l / x): the localizer network at batch 16 on 640 x 640 (device-resident input) in both operand modes,
ms per image, beside the YOLOv5 scale of the same letter measured in the same run (same process, same device, one after the other).
No target is set for these numbers: the text file is what came out.
   python tools/yolov8_time.py [--scales nsmlx] [--out profiles/yolov8_time.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from effocr_amd.localizer_engine import (HipLocalizer, HipLocalizerV8, init_yolov5_state_dict, init_yolov8_state_dict,  # noqa: E402
                                         yolov5_param_shapes, yolov8_param_shapes)


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
             "# bf16 = bf16-rounded operands (stem and the heads' last 1x1 fp32); YOLOv5 of the same letter measured in the same run",
             f"# {'scale':<8} {'Mparams':>8} {'fp32 ms/img':>20} {'bf16 ms/img':>20}"]
    for s in a.scales:
        for fam, engine, init, shapes in (("yolov8", HipLocalizerV8, init_yolov8_state_dict, yolov8_param_shapes),
                                          ("yolov5", HipLocalizer, init_yolov5_state_dict, yolov5_param_shapes)):
            (t32, t32min), (t16, t16min) = measure(engine, init(2, s, seed=0), x, dev)
            lines.append(f"  {fam + s:<8} {mparams(shapes(2, s)):>8.2f} {t32 / B:>11.4f} ({t32min / B:.4f}) {t16 / B:>11.4f} ({t16min / B:.4f})")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
