#!/usr/bin/env python
"""Cost of the call-size-invariant mode: the same engines in default and in invariant mode, alternated round by round inside one process
(DESIGN.md "Call-size-invariant mode"; the committed output is profiles/call_size_invariant_cost.txt).

  encoders    crops/s of HipEncoder.forward(normalize=True) + k-NN (k = 10, 10 000 rows) and ms per call, device-resident crops
  localizer   images/s and ms per call of the yolov5s network at 640 x 640
  run_effocr  lines/s over 64 synthetic 4096 x 256 lines at lines_per_chunk 1 and 16, both engines switched together

    python tools/call_size_invariant_cost.py [rounds]        (default 5 rounds per mode, the median is reported)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from effocr_amd.encoders import HipEncoder                      # noqa: E402
from effocr_amd.knn import FaissKNN, IndexFlatIP                # noqa: E402
from effocr_amd.localizer_engine import EffLocalizer, HipLocalizer, init_yolov5s_state_dict   # noqa: E402
from effocr_amd.pipeline import run_effocr                      # noqa: E402
from effocr_amd.recognizer_engine import EffRecognizer          # noqa: E402
from effocr_amd.transforms import PairedTransform               # noqa: E402
from effocr_amd.weights import init_state_dict                  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
dev = torch.device("cuda:0")


def alternate(step, set_mode, items, min_calls=20, budget=4096):
    """Median over ROUNDS of the time per call of ``step`` in each mode, the modes alternating: -> {mode: seconds per call}."""
    n = max(min_calls, budget // items)
    t = {0: [], 1: []}
    for mode in (0, 1):                                          # warm up both modes' kernels and workspaces
        set_mode(mode)
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for mode in (0, 1):
            set_mode(mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                step()
            torch.cuda.synchronize()
            t[mode].append((time.perf_counter() - t0) / n)
    set_mode(0)
    return {m: float(np.median(v)) for m, v in t.items()}


def row(label, items, unit, t):
    print(f"{label:34s} default {items / t[0]:9.0f} {unit}/s {t[0] * 1e3:8.3f} ms/call   invariant {items / t[1]:9.0f} {unit}/s "
          f"{t[1] * 1e3:8.3f} ms/call   invariant / default time {t[1] / t[0]:5.2f}", flush=True)


print(f"# call-size-invariant mode against the default mode, alternated in one process, median of {ROUNDS} rounds per mode")
print("# encoders: forward(normalize=True) + k-NN (k = 10 over 10 000 rows), crops resident on the device")
for arch, img, precs, sizes in (("vit_small_patch16_224", 224, ("fp16", "bf16"), (1, 16, 64, 128, 256, 1024)),
                                ("vit_base_patch16_224", 224, ("fp16",), (64, 1024)),
                                ("resnet18", 32, ("fp32",), (64,))):
    sd = init_state_dict(arch, seed=0, img_size=img)
    for prec in precs:
        enc = HipEncoder(arch, sd, img_size=img, precision=prec, device=dev)
        idx = IndexFlatIP(enc.embed_dim, device=dev)
        idx.add(torch.nn.functional.normalize(torch.randn(10000, enc.embed_dim, generator=torch.Generator().manual_seed(0)), dim=1))
        for B in sizes:
            x = torch.randn(B, 3, img, img, device=dev)
            t = alternate(lambda: idx.search_device(enc.forward(x, normalize=True), 10),
                          lambda m: enc.set_option("call_size_invariant", m), B)
            row(f"{arch} {prec} {img}^2 B={B}", B, "crops", t)
        enc.check_status()
        del enc, idx

print("# localizer: yolov5s network, 640 x 640, fp32 operands")
loc = HipLocalizer(init_yolov5s_state_dict(2, seed=0), input_shape=(640, 640), device=dev)
for B in (1, 16):
    im = torch.rand(B, 3, 640, 640, device=dev)
    t = alternate(lambda: loc.forward(im), lambda m: loc.set_option("call_size_invariant", m), B, min_calls=20, budget=320)
    row(f"yolov5s 640^2 B={B}", B, "images", t)
del loc

print("# run_effocr: 64 lines of 4096 x 256, yolov5s + vit_small_patch16_224 fp16, both engines switched together")
loc_sd = init_yolov5s_state_dict(2, seed=0)
for l in range(3):                                               # a Detect head that fires: ~50 character boxes per line
    b = loc_sd[f"model.24.m.{l}.bias"].view(3, 7)
    b[:, 4] += 5.5
    b[:, 5] += 2.5
    b[:, 6] += 2.4
eloc = EffLocalizer(loc_sd, iou_thresh=0.05, conf_thresh=0.5, device=dev)
arch = "vit_small_patch16_224"
rec = EffRecognizer(init_state_dict(arch, seed=1, img_size=224), arch=arch, precision="fp16", device=dev)
tf = PairedTransform(size=224, device=dev)
chars = [chr(0x4E00 + i) for i in range(2000)]
knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False, device=dev)
knn.train(torch.nn.functional.normalize(torch.randn(len(chars), 384, generator=torch.Generator().manual_seed(1)), dim=1))
rng = np.random.default_rng(11)
lines = [(rng.integers(0, 256, (256, 4096, 3)) // 32 * 32).astype(np.uint8) for _ in range(64)]


def both(m):
    eloc._eng_net.set_option("call_size_invariant", m)
    rec._eng_net.set_option("call_size_invariant", m)


for lpc in (1, 16):
    t = alternate(lambda: run_effocr(lines, eloc, rec, tf, "jp", knn_func=knn, candidate_chars=chars, lines_per_chunk=lpc), both,
                  len(lines), min_calls=2, budget=128)
    row(f"run_effocr lines_per_chunk={lpc}", len(lines), "lines", t)
