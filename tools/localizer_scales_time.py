#!/usr/bin/env python
"""Per YOLOv5 scale (n / s / m / l / x): the localizer network at batch 16 on 640 x 640 (device-resident input) in both operand
modes, its conv GFLOP per image and the fraction of the fp32 MFMA peak (157.3 TF, as bench.py counts it), the FLOPs the channel
padding to 32 adds (n / m / x), and run_effocr lines/s at BASELINE configs[4]'s shape (64 x 4096x256 lines per call, ViT-S/16 bf16
recognizer, 10 000-row index; bench.py's c5 workload with the localizer swapped).
   python tools/localizer_scales_time.py [--scales nsmlx] [--lines-scales nsm] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from effocr_amd.localizer_engine import YOLOV5_SCALES, EffLocalizer, HipLocalizer, init_yolov5_state_dict  # noqa: E402
from oracle.yolo_modules import YoloV5, conv_flops  # noqa: E402

FP32_PEAK = 157.3e12


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


def padding_flops(scale, h=640, w=640):
    """2 x the multiply-accumulates the stored channel padding to 32 adds (model.1's input, model.2's inner C3 tensors; the stem's zero
    groups are not computed)."""
    depth, width = YOLOV5_SCALES[scale]
    c0 = int(np.ceil(64 * width / 8) * 8)
    c_ = c0                                                   # model.2 = C3(c128 -> c128): c_ = c128 / 2 = c64
    p = (c0 + 31) // 32 * 32
    if p == c0:
        return 0.0
    n = max(round(3 * depth), 1)
    px = (h // 4) * (w // 4)                                  # model.1 and model.2 run at stride 4
    c128 = 2 * c0
    extra = 9 * (p - c0) * c128                               # model.1: 3x3, Cin c0 -> p
    extra += 2 * (p - c_) * c128                              # model.2 cv1 | cv2: Cout 2 c_ -> 2 p
    extra += n * (p * p - c_ * c_) * (1 + 9)                  # bottlenecks: 1x1 and 3x3, c_ -> p in and out
    extra += 2 * (p - c_) * c128                              # cv3: Cin 2 c_ -> 2 p
    return 2.0 * extra * px


def lines_per_s(scale, dev):
    from effocr_amd.knn import FaissKNN, IndexFlatIP
    from effocr_amd.pipeline import run_effocr
    from effocr_amd.recognizer_engine import EffRecognizer
    from effocr_amd.transforms import PairedTransform
    from effocr_amd.weights import init_state_dict
    nc = 2
    sd = init_yolov5_state_dict(nc, scale, seed=0)
    for l in range(3):
        b = sd[f"model.24.m.{l}.bias"].view(3, nc + 5)
        b[:, 4] += 5.5
        b[:, 5] += 2.5
    loc = EffLocalizer(sd, iou_thresh=0.05, conf_thresh=0.5, device=dev)
    arch = "vit_small_patch16_224"
    rec = EffRecognizer(init_state_dict(arch, seed=0, img_size=224), arch=arch, precision="bf16", device=dev)
    knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False, device=dev)
    knn.train(torch.nn.functional.normalize(torch.randn(10000, rec._eng_net.embed_dim, generator=torch.Generator().manual_seed(0)), dim=1))
    chars = [chr(0x4E00 + i) for i in range(10000)]
    tf = PairedTransform(size=224, device=dev)
    rng = np.random.default_rng(0)
    lines = [(rng.integers(0, 256, (256, 4096, 3)) // 32 * 32).astype(np.uint8) for _ in range(64)]

    def call():
        t0 = time.perf_counter()
        res, _ = run_effocr(lines, loc, rec, tf, "jp", knn_func=knn, candidate_chars=chars)
        return time.perf_counter() - t0, res

    _, res = call()
    t = sorted(call()[0] for _ in range(5))[2]
    return {"lines_per_s": round(64 / t, 2), "ms_per_64_line_call_median_of_5": round(1e3 * t, 3),
            "chars_per_line": round(sum(len(v) for v in res.values()) / 64, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", default="nsmlx")
    ap.add_argument("--lines-scales", default="nsm", help="scales to run the configs[4] pipeline with ('' = none)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    x = torch.rand(16, 3, 640, 640, generator=torch.Generator().manual_seed(1)).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "batch": 16, "input": [640, 640], "fp32_mfma_peak_tflops": FP32_PEAK / 1e12, "scales": {}}
    for s in a.scales:
        depth, width = YOLOV5_SCALES[s]
        fl = conv_flops(YoloV5(2, depth, width), 640, 640)
        eng = HipLocalizer(init_yolov5_state_dict(2, s, seed=0), device=dev)
        t32, t32min = gpu_ms(lambda: eng.forward(x))
        eng.set_option("bf16_operands", 1)
        t16, t16min = gpu_ms(lambda: eng.forward(x))
        eng.set_option("bf16_operands", 0)
        pad = padding_flops(s)
        r = {"GFLOP_per_image": round(fl / 1e9, 2), "padding_GFLOP_per_image": round(pad / 1e9, 3),
             "padding_fraction": round(pad / fl, 4),
             "fp32_ms_per_image": round(t32 / 16, 4), "fp32_ms_per_image_min": round(t32min / 16, 4),
             "fp32_mfma_frac": round(16 * fl / (t32 * 1e-3) / FP32_PEAK, 4),
             "bf16_operands_ms_per_image": round(t16 / 16, 4), "bf16_operands_ms_per_image_min": round(t16min / 16, 4)}
        del eng
        torch.cuda.empty_cache()
        if s in a.lines_scales:
            r["run_effocr_configs4"] = lines_per_s(s, dev)
        out["scales"][s] = r
        print(f"yolov5{s}: {json.dumps(r)}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
