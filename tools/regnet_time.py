#!/usr/bin/env python
"""regnetx_002 .. regnety_016 encoder + exact k-NN throughput on one GPU, with mobilenetv3_large_100 and resnet34 for scale, and the grouped
3x3 convolution alone.

  python tools/regnet_time.py [--crops 1024] [--precisions fp16,bf16] [--iters 3] [--out profiles/regnet_time.txt]

The driver touches no GPU: every measurement is a child process of its own (`--step ...`) under its own `timeout`, and the driver stops
at the first step that fails or runs out of time.  Steps:
  encoder ARCH        for each precision: crops/s of Recognizer.neighbors (encoder -> fused L2 normalise -> IP top-10 over a 10 000 x D
                      index), seeded random weights (init_state_dict(scale="unit")), 224^2 fp32 crops already on the device; the median of
                      three CUDA-event windows of about half a second of back-to-back calls each (at least `iters` calls), after 2 warm-up
                      calls.
  gconv               effocr_regnet_op_gconv alone at 64 crops on RANDOM N(0, 1) activations and weights, in the shapes of the first
                      block of s1, the first block of s2 and the other blocks of s2 of regnety_008 (group width 16, with the tile sums) and
                      regnetx_006 (group width 24, without), every precision.  Beside each time: what the kernel's input and output bytes
                      (fp32 activations; the weights are a few KB) would take at the 6.3 TB/s copy rate this project measured,
                      and the ratio.  No ratio was set in advance.
Per 224^2 crop the ten models cost 0.2 / 0.4 / 0.6 / 0.8 / 1.6 GMAC (X and Y alike), mobilenetv3_large_100 0.22, resnet34 3.7."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REGNETS = ("regnetx_002", "regnetx_004", "regnetx_006", "regnetx_008", "regnetx_016",
           "regnety_002", "regnety_004", "regnety_006", "regnety_008", "regnety_016")
SCALE = ("mobilenetv3_large_100", "resnet34")
IMG = 224
STEP_TIMEOUT = {"encoder": 150, "gconv": 120}          # seconds, per child process
COPY_RATE = 6.3e12                                        # bytes/s, DESIGN.md
# (what, in_size, channels, stride, group width, tile sums)
GCONV_SHAPES = (("regnety_008 s1.b1", 112, 64, 2, 16, True), ("regnety_008 s2.b1", 56, 128, 2, 16, True), ("regnety_008 s2.b2", 28, 128, 1, 16, True),
                ("regnetx_006 s1.b1", 112, 48, 2, 24, False), ("regnetx_006 s2.b1", 56, 96, 2, 24, False), ("regnetx_006 s2.b2", 28, 96, 1, 24, False))


def windows(call, warmup, min_calls, dev, target_ms=500.0, repeats=3):
    """(min, median, max) ms per call over `repeats` CUDA-event windows of n back-to-back calls each, and n: after `warmup` calls one call
    is timed to size n so that a window lasts about `target_ms` (at least `min_calls` calls)."""
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize(dev)

    def timed(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / n
    n = max(min_calls, int(target_ms / max(timed(min_calls), 1e-3)))
    got = sorted(timed(n) for _ in range(repeats))
    return got[0], got[len(got) // 2], got[-1], n


def step_encoder(arch, precs, crops, iters):
    import torch
    from effocr_amd import weights as W
    from effocr_amd.encoders import make_encoder
    from effocr_amd.knn import FaissKNN, IndexFlatIP
    from effocr_amd.pipeline import Recognizer
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(crops, 3, IMG, IMG, generator=g).to(dev)
    D = W.embed_dim(arch)
    index = torch.nn.functional.normalize(torch.randn(10000, D, generator=g), dim=1)
    sd = W.init_state_dict(arch, seed=0)
    for prec in precs:
        enc = make_encoder(arch, sd, precision=prec, device=dev)
        knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
        knn.train(index)
        rec = Recognizer(enc, knn, [chr(0x4E00 + i) for i in range(10000)], knn=10)
        lo, ms, hi, n = windows(lambda: rec.neighbors(x), 2, iters, dev)
        enc.check_status()
        print(f"RESULT {prec:>9} {crops:>6} {arch:>24} {crops / ms * 1e3:>10.0f} crops/s {ms:>9.2f} ms per call (windows of {n} calls: {lo:.2f} .. {hi:.2f} ms)")
        del rec, knn, enc


def step_gconv(precs):
    import torch
    from effocr_amd import _lib
    dev = torch.device("cuda:0")
    B = 64
    L = _lib.regnet_lib()
    g = torch.Generator().manual_seed(0)
    for what, H, C, stride, gw, sums in GCONV_SHAPES:
        Ho = (H - 1) // stride + 1
        x = torch.randn(B, H, H, C, generator=g).to(dev)
        w = torch.randn(C, gw, 3, 3, generator=g) / (3 * gw ** 0.5)
        b = (torch.randn(C, generator=g) * 0.1).to(dev)
        out = torch.empty(B, Ho, Ho, C, device=dev)
        part = torch.empty(B, int(L.effocr_regnet_op_tiles(Ho)), C, device=dev) if sums else None
        nbytes = 4.0 * B * C * (H * H + Ho * Ho)
        floor_us = nbytes / COPY_RATE * 1e6
        for prec in precs:
            host = torch.empty(int(L.effocr_regnet_op_gconv_weight_bytes(_lib.PREC[prec], C, gw)), dtype=torch.uint8)
            _lib.regnet_check(L.effocr_regnet_op_pack_gconv(_lib.PREC[prec], C, gw, _lib.ptr(w), _lib.ptr(host)), "effocr_regnet_op_pack_gconv")
            wd = host.to(dev)

            def launch():
                _lib.regnet_check(L.effocr_regnet_op_gconv(_lib.PREC[prec], _lib.ptr(x), B, H, C, stride, gw, _lib.ptr(wd), _lib.ptr(b), _lib.ptr(out),
                                                           _lib.ptr(part), _lib.current_stream(dev)), "effocr_regnet_op_gconv")
            lo, ms, hi, n = windows(launch, 3, 20, dev, target_ms=300.0)
            assert torch.isfinite(out).all()
            mac = 9.0 * gw * C * B * Ho * Ho
            print(f"RESULT {prec:>9} gconv alone, {what}: B={B} {H}^2 -> {Ho}^2, C={C}, gw={gw}, stride {stride}{', tile sums' if sums else ''}, random data: "
                  f"{ms * 1e3:.1f} us per launch ({lo * 1e3:.1f} .. {hi * 1e3:.1f}, windows of {n}); {nbytes / 1e6:.1f} MB in + out = {floor_us:.1f} us at "
                  f"6.3 TB/s: {ms * 1e3 / floor_us:.2f} x the copy time; {2 * mac / ms / 1e9:.2f} TFLOP/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=1024)
    ap.add_argument("--precisions", default="fp16,bf16")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regnet_time.txt"))
    ap.add_argument("--step", nargs="+", help="(internal) run one measurement in this process")
    a = ap.parse_args()
    precs = a.precisions.split(",")
    if a.step:
        if a.step[0] == "encoder":
            step_encoder(a.step[1], precs, a.crops, a.iters)
        else:
            step_gconv(precs + ["fp32"])
        return 0
    steps = [("encoder", arch) for arch in REGNETS + SCALE] + [("gconv",)]
    lines = [f"python tools/regnet_time.py --crops {a.crops} --precisions {a.precisions} --iters {a.iters}   (1x MI355X; seeded weights; measured, nothing assumed)",
             f"{IMG}^2 crops, encoder + k-NN (10 000 x D index, k = 10); median of three ~0.5 s windows of back-to-back calls after 2 warm-up calls (min .. max)"]
    rc = 0
    for st in steps:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT[st[0]]), sys.executable, os.path.abspath(__file__), "--crops", str(a.crops), "--iters", str(a.iters),
               "--precisions", a.precisions, "--step", *st]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        got = [ln[len("RESULT "):] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            lines.append(f"step {' '.join(st)}: FAILED (exit {r.returncode}); nothing after it was run")
            sys.stderr.write(r.stdout[-4000:])
            rc = 1
            break                                          # a failed GPU step ends the run: nothing more is started on the device
        lines += got
        print("\n".join(got), flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
