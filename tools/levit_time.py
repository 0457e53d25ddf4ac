#!/usr/bin/env python
"""levit_128s .. levit_384 encoder + exact k-NN throughput on one GPU, with vit_small_patch16_224 and mobilenetv3_small_050 for scale, and
the LeViT attention kernel alone.

  python tools/levit_time.py [--crops 1024] [--precisions fp16,bf16] [--iters 5] [--out profiles/levit_time.txt]

The driver touches no GPU: every measurement is a child process of its own (`--step ...`) under its own `timeout`, and the driver stops
at the first step that fails or runs out of time.  Steps:
  encoder ARCH PREC   crops/s of Recognizer.neighbors (encoder -> fused L2 normalise -> IP top-10 over a 10 000 x D index), seeded random
                      weights (init_state_dict(scale="unit")), 224^2 fp32 crops already on the device; the median of three CUDA-event
                      windows of about one second of back-to-back calls each (at least `iters` calls), after 2 warm-up calls.
  attention PREC      effocr_levit_op_attention alone at 64 crops on RANDOM N(0, 1) q, k, v and biases — zero-filled q / k collapse the
                      softmax work and flatter the number — in the three shapes of levit_128s' first stages: 14 x 14 keys, 4 heads, kd 16,
                      values 32 (stage 0); the 14 -> 7 down-sampling, 8 heads, values 64; 7 x 7 keys, 6 heads, values 32 (stage 1).
                      2 B heads Tq Tk (kd + vd) FLOP per launch; the median of three windows of about a second, after 3 warm-up launches.
Per 224^2 crop the five models cost about 0.3 / 0.4 / 0.65 / 1.1 / 2.3 GMAC (timm's figures), ViT-S/16 4.6 GMAC."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVITS = ("levit_128s", "levit_128", "levit_192", "levit_256", "levit_384")
SCALE = ("vit_small_patch16_224", "mobilenetv3_small_050")
IMG = 224
STEP_TIMEOUT = {"encoder": 150, "attention": 90}          # seconds, per child process
ATTN_SHAPES = (("stage 0", 14, 1, 4, 16, 32), ("14 -> 7", 14, 2, 8, 16, 64), ("stage 1", 7, 1, 6, 16, 32))


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
    if enc.crop_dtype != torch.float32:
        x = x.to(enc.crop_dtype)
    knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
    knn.train(index)
    rec = Recognizer(enc, knn, [chr(0x4E00 + i) for i in range(10000)], knn=10)
    lo, ms, hi, n = windows(lambda: rec.neighbors(x), 2, iters, dev)
    enc.check_status()
    print(f"RESULT {prec:>9} {crops:>6} {arch:>24} {crops / ms * 1e3:>10.0f} crops/s {ms:>9.2f} ms per call (windows of {n} calls: {lo:.2f} .. {hi:.2f} ms)")


def step_attention(prec):
    import torch
    from effocr_amd import _lib
    from effocr_amd.weights import levit_sub
    dev = torch.device("cuda:0")
    B = 64
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[prec]
    L = _lib.levit_lib()
    g = torch.Generator().manual_seed(0)
    for what, R, stride, heads, kd, vd in ATTN_SHAPES:
        Tk, Tq = R * R, (levit_sub(R) if stride == 2 else R) ** 2
        hs = (2 * kd if stride == 1 else kd) + vd
        kv = torch.randn(B * Tk, heads * hs, generator=g).to(dt).to(dev)
        q = kv if stride == 1 else torch.randn(B * Tq, heads * kd, generator=g).to(dt).to(dev)
        tb = torch.randn(heads, Tk, generator=g).to(dev)
        out = torch.empty(B * Tq, heads * vd, dtype=dt, device=dev)
        ldq, qhs, koff, voff = (heads * hs, hs, kd, 2 * kd) if stride == 1 else (heads * kd, kd, 0, kd)

        def launch():
            _lib.levit_check(L.effocr_levit_op_attention(_lib.ptr(q), ldq, qhs, 0, _lib.ptr(kv), heads * hs, hs, koff, voff, _lib.ptr(tb), B, R, stride,
                                                         heads, kd, vd, 1, _lib.PREC[prec], _lib.ptr(out), _lib.current_stream(dev)), "effocr_levit_op_attention")
        lo, ms, hi, n = windows(launch, 3, 20, dev)
        flop = 2.0 * B * heads * Tq * Tk * (kd + vd)
        assert torch.isfinite(out.float()).all()
        print(f"RESULT {prec:>9} attention alone, {what}: B={B} keys={Tk} queries={Tq} heads={heads} kd={kd} vd={vd}, random data: {ms * 1e3:.1f} us per "
              f"launch, {flop / ms / 1e9:.2f} TFLOP/s (windows of {n} launches: {lo * 1e3:.1f} .. {hi * 1e3:.1f} us)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=1024)
    ap.add_argument("--precisions", default="fp16,bf16")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levit_time.txt"))
    ap.add_argument("--step", nargs="+", help="(internal) run one measurement in this process")
    a = ap.parse_args()
    if a.step:
        if a.step[0] == "encoder":
            step_encoder(a.step[1], a.step[2], a.crops, a.iters)
        else:
            step_attention(a.step[1])
        return 0
    precs = a.precisions.split(",")
    steps = [("encoder", arch, prec) for prec in precs for arch in LEVITS + SCALE] + [("attention", prec) for prec in precs]
    lines = [f"python tools/levit_time.py --crops {a.crops} --precisions {a.precisions} --iters {a.iters}   (1x MI355X; seeded weights; measured, nothing assumed)",
             f"{IMG}^2 crops, encoder + k-NN (10 000 x D index, k = 10); median of three ~1 s windows of back-to-back calls after 2 warm-up calls (min .. max)"]
    rc = 0
    for st in steps:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT[st[0]]), sys.executable, os.path.abspath(__file__), "--crops", str(a.crops), "--iters", str(a.iters),
               "--step", *st]
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
