#!/usr/bin/env python
"""vit_small_patch8_224 / vit_base_patch8_224 encoder + exact k-NN throughput on one GPU, with vit_small_patch16_224 for scale, and the
streaming attention kernel alone.

  python tools/vit8_time.py [--crops 1024] [--precisions fp16,bf16] [--iters 5] [--out profiles/vit8_time.txt]

The driver touches no GPU: every measurement is a child process of its own (`--step ...`) under its own `timeout`, and the driver stops
at the first step that fails or runs out of time.  Steps:
  encoder ARCH PREC   crops/s of Recognizer.neighbors (encoder -> fused L2 normalise -> IP top-10 over a 10 000 x D index), seeded random
                      weights (init_state_dict(scale="unit")), 224^2 fp32 crops already on the device; the median of three CUDA-event
                      windows of about one second of back-to-back calls each (at least `iters` calls), after 2 warm-up calls.
  attention PREC      effocr_vit8_op_attn alone at B = 64, T = 785, 6 heads (one ViT-S/8 layer of 64 crops) on RANDOM N(0, 1) q, k, v —
                      zero-filled q / k collapse the softmax work and flatter the number — 4 B heads T^2 64 FLOP per launch; the median of three windows
                      of about one second of launches each, after 3 warm-up launches.
Per crop ViT-S/8 costs 44.8 GFLOP (33.3 in the linears, 11.4 in attention, 0.1 in the patch embedding), ViT-B/8 156.3, ViT-S/16 9.2."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S8, B8, S16, IMG = "vit_small_patch8_224", "vit_base_patch8_224", "vit_small_patch16_224", 224
STEP_TIMEOUT = {S8: 150, B8: 240, S16: 120, "attention": 90}          # seconds, per child process


def windows(call, warmup, min_calls, dev, target_ms=1000.0, repeats=3):
    """(min, median, max) ms per call over `repeats` CUDA-event windows of n back-to-back calls each, and n: after `warmup` calls one call
    is timed to size n so that a window lasts about `target_ms` (at least `min_calls` calls) — a window of a few milliseconds measures
    the clock ramp and the scheduler as much as the kernels."""
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


def step_encoder(arch, prec, crops, iters):
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
    enc = make_encoder(arch, W.init_state_dict(arch, seed=0), precision=prec, device=dev)
    knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
    knn.train(index)
    rec = Recognizer(enc, knn, [chr(0x4E00 + i) for i in range(10000)], knn=10)
    lo, ms, hi, n = windows(lambda: rec.neighbors(x), 2, iters, dev)
    enc.check_status()
    print(f"RESULT {prec:>9} {crops:>6} {arch:>24} {crops / ms * 1e3:>10.0f} crops/s {ms:>9.2f} ms per call (windows of {n} calls: {lo:.2f} .. {hi:.2f} ms)")


def step_attention(prec):
    import torch
    from effocr_amd import _lib
    dev = torch.device("cuda:0")
    B, T, heads = 64, 785, 6
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[prec]
    qkv = torch.randn(B * T, 3 * heads * 64, generator=torch.Generator().manual_seed(0)).to(dt).to(dev)
    out = torch.empty(B * T, heads * 64, dtype=dt, device=dev)
    L = _lib.vit8_lib()

    def launch():
        _lib.vit8_check(L.effocr_vit8_op_attn(_lib.ptr(qkv), B, T, heads, _lib.PREC[prec], _lib.ptr(out), _lib.current_stream(dev)), "effocr_vit8_op_attn")
    lo, ms, hi, n = windows(launch, 3, 20, dev)
    flop = 4.0 * B * heads * T * T * 64
    assert torch.isfinite(out.float()).all()
    print(f"RESULT {prec:>9} attention alone B={B} T={T} heads={heads}, random data: {ms:.4f} ms per launch, {flop / ms / 1e9:.1f} TFLOP/s "
          f"(windows of {n} launches: {flop / hi / 1e9:.1f} .. {flop / lo / 1e9:.1f} TFLOP/s)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=1024)
    ap.add_argument("--precisions", default="fp16,bf16")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vit8_time.txt"))
    ap.add_argument("--step", nargs="+", help="(internal) run one measurement in this process")
    a = ap.parse_args()
    if a.step:
        if a.step[0] == "encoder":
            step_encoder(a.step[1], a.step[2], a.crops, a.iters)
        else:
            step_attention(a.step[1])
        return 0
    precs = a.precisions.split(",")
    steps = [("encoder", arch, prec) for prec in precs for arch in (S8, B8, S16)] + [("attention", prec) for prec in precs]
    lines = [f"python tools/vit8_time.py --crops {a.crops} --precisions {a.precisions} --iters {a.iters}   (1x MI355X; seeded weights; measured, nothing assumed)",
             f"{IMG}^2 crops, encoder + k-NN (10 000 x D index, k = 10); median of three ~1 s windows of back-to-back calls after 2 warm-up calls (min .. max)"]
    rc = 0
    for st in steps:
        limit = STEP_TIMEOUT[st[1] if st[0] == "encoder" else "attention"]
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--crops", str(a.crops), "--iters", str(a.iters), "--step", *st]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        got = [ln[len("RESULT "):] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            lines.append(f"step {' '.join(st)}: FAILED (exit {r.returncode}); nothing after it was run")
            sys.stderr.write(r.stdout[-4000:])
            rc = 1
            break                                          # a failed GPU step ends the run: nothing more is started on the device
        lines += got
        print(got[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
