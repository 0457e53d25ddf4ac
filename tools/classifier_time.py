"""Throughput of the FFNN classifier head (libeffocr_head.so) and of the classifier recognizer against the kNN recognizer.

  python tools/classifier_time.py --out DIR     full sweep, writes DIR/classifier_time.txt and DIR/classifier_time.json
  python tools/classifier_time.py --quick       a short pass (for a kernel-trace run), prints only

Timing: device events around `reps` back-to-back calls on one stream after `warmup` calls; the median of 5 such rounds per point.
Sweep 1 — the head alone, ids + logits, B in {1, 16, 64, 1024} x N in {182, 30 813} x d in {384, 768, 1024}, with its roofline
(FLOP at the 157.3 TF fp32 MFMA peak, bytes of W + emb + logits at 8 TB/s).  Sweep 2 — ViT-S/16 fp16 at 224: encoder + head + fused
argmax (N = 30 813) against encoder + fused L2 normalise + IndexFlatIP top-10 over 10 000 rows, at 16, 64 and 1024 crops."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from effocr_amd import weights as W                    # noqa: E402
from effocr_amd.classifiers import AutoClassifierFactory, HipClassifierHead   # noqa: E402
from effocr_amd.encoders import AutoEncoderFactory      # noqa: E402
from effocr_amd.knn import FaissKNN, IndexFlatIP        # noqa: E402

PEAK_TF, HBM_TBS = 157.3, 8.0


def timed(fn, warmup, reps, rounds=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out)


def head_sweep(dev, Bs, Ns, ds, warmup, reps, lines, rows):
    for d in ds:
        for N in Ns:
            g = torch.Generator().manual_seed(N + d)
            head = HipClassifierHead(torch.randn(N, d, generator=g) / d ** 0.5, torch.randn(N, generator=g) * 0.1, device=dev)
            for B in Bs:
                emb = torch.randn(B, d, device=dev)
                ms_both = timed(lambda: head._run(emb, True, True), warmup, reps)
                ms_ids = timed(lambda: head.predict(emb), warmup, reps)
                flop = 2.0 * B * N * d
                byts = 4.0 * (N * d + B * d + B * N)
                roof_us = max(flop / (PEAK_TF * 1e12), byts / (HBM_TBS * 1e12)) * 1e6
                r = dict(B=B, N=N, d=d, us_logits_ids=ms_both * 1e3, us_ids=ms_ids * 1e3, tflops=flop / (ms_ids * 1e-3) / 1e12,
                         tbs=4.0 * N * d / (ms_ids * 1e-3) / 1e12, roofline_us=roof_us)
                rows.append(r)
                lines.append(f"head B={B:5d} N={N:6d} d={d:5d}: logits+ids {r['us_logits_ids']:9.2f} us  ids only {r['us_ids']:9.2f} us  "
                             f"({r['tflops']:6.1f} TF/s, W at {r['tbs']:5.2f} TB/s; roofline {roof_us:8.2f} us)")
                print(lines[-1], flush=True)


def e2e(dev, crops_list, warmup, reps, lines, rows):
    arch, N = "vit_small_patch16_224", 30813
    sd = W.init_state_dict(arch, seed=1, num_classes=N)
    clf = AutoClassifierFactory("timm", arch, N, precision="fp16")()
    clf.load_state_dict(sd)
    clf.to(dev).eval()
    enc = AutoEncoderFactory("timm", arch, precision="fp16")()
    enc.load_state_dict({k: v for k, v in sd.items() if not k.startswith("head.")})
    enc.to(dev).eval()
    knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
    knn.train(torch.nn.functional.normalize(torch.randn(10000, 384, generator=torch.Generator().manual_seed(2)), dim=1))
    for B in crops_list:
        x = torch.randn(B, 3, 224, 224, device=dev)
        ms_c = timed(lambda: clf.predict(x), warmup, reps)
        ms_k = timed(lambda: knn(enc.engine.forward(x, normalize=True), k=10), warmup, reps)
        ms_e = timed(lambda: enc.engine.forward(x, normalize=False), warmup, reps)
        clf.check_status()
        enc.check_status()
        r = dict(crops=B, ms_encoder=ms_e, ms_classifier=ms_c, ms_knn=ms_k, crops_per_s_classifier=B / ms_c * 1e3,
                 crops_per_s_knn=B / ms_k * 1e3, ratio=ms_k / ms_c)
        rows.append(r)
        lines.append(f"vit_small fp16 {B:5d} crops: encoder {ms_e:8.3f} ms | encoder+head+argmax (N={N}) {ms_c:8.3f} ms "
                     f"({r['crops_per_s_classifier']:9.0f} crops/s) | encoder+normalise+kNN top-10 (10 000 rows) {ms_k:8.3f} ms "
                     f"({r['crops_per_s_knn']:9.0f} crops/s) | classifier rate / kNN rate {r['ratio']:.3f}")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="directory for classifier_time.txt / .json")
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines, head_rows, e2e_rows = [], [], []
    if a.quick:
        head_sweep(dev, [16, 1024], [182, 30813], [384], 3, 5, lines, head_rows)
        e2e(dev, [64], 2, 3, lines, e2e_rows)
    else:
        head_sweep(dev, [1, 16, 64, 1024], [182, 30813], [384, 768, 1024], 20, 50, lines, head_rows)
        e2e(dev, [16, 64, 1024], 5, 10, lines, e2e_rows)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "classifier_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(os.path.join(a.out, "classifier_time.json"), "w") as f:
            json.dump({"head": head_rows, "e2e": e2e_rows, "device": torch.cuda.get_device_name(dev)}, f, indent=1)


if __name__ == "__main__":
    main()
