#!/usr/bin/env python
"""pvt_v2_b0 .. pvt_v2_b5 encoder + exact k-NN throughput on one GPU, with vit_small_patch16_224, levit_128 and mobilenetv3_small_050 for
scale, and the PVTv2 attention and depthwise 3x3 + GELU kernels alone.

  python tools/pvt_time.py [--crops 1024] [--precisions fp16,bf16] [--iters 5] [--out profiles/pvt_time.txt]

The driver touches no GPU: every measurement is a child process of its own (`--step ...`) under its own `timeout`, and the driver stops
at the first step that fails or runs out of time.  Steps:
  encoder ARCH PREC   crops/s of Recognizer.neighbors (encoder -> fused L2 normalise -> IP top-10 over a 10 000 x D index), seeded random
                      weights (init_state_dict), 224^2 fp32 crops already on the device; the median of three CUDA-event windows of about
                      one second of back-to-back calls each (at least `iters` calls), after 2 warm-up calls.
  kernels PREC        effocr_pvt_op_attention and effocr_pvt_op_dwconv_gelu alone at 64 crops on RANDOM N(0, 1) data, in the four stage
                      shapes of pvt_v2_b1 at 224^2 (3136 / 784 / 196 / 49 queries on 49 keys; hidden widths 512 / 1024 / 1280 / 2048), each
                      beside the time its input and output bytes take at the project's measured 6.3 TB/s copy rate; the median of three
                      windows of about a second, after 3 warm-up launches."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PVTS = ("pvt_v2_b0", "pvt_v2_b1", "pvt_v2_b2", "pvt_v2_b3", "pvt_v2_b4", "pvt_v2_b5")
SCALE = ("vit_small_patch16_224", "levit_128", "mobilenetv3_small_050")
IMG = 224
STEP_TIMEOUT = {"encoder": 240, "kernels": 120}           # seconds, per child process
COPY_TBS = 6.3                                             # the project's measured device copy rate, TB/s
# pvt_v2_b1 at 224^2: (stage, queries, heads, width, hidden width); 49 keys, head width 64
STAGES = ((0, 3136, 1, 64, 512), (1, 784, 2, 128, 1024), (2, 196, 5, 320, 1280), (3, 49, 8, 512, 2048))


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


def step_kernels(prec):
    import torch
    from effocr_amd import _lib
    dev = torch.device("cuda:0")
    B, M, hd = 64, 49, 64
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[prec]
    es = torch.empty(0, dtype=dt).element_size()
    L = _lib.pvt_lib()
    g = torch.Generator().manual_seed(0)
    for stage, N, heads, C, hid in STAGES:
        q = torch.randn(B * N, C, generator=g).to(dt).to(dev)
        kv = torch.randn(B * M, 2 * C, generator=g).to(dt).to(dev)
        out = torch.empty(B * N, C, dtype=dt, device=dev)

        def attn():
            _lib.pvt_check(L.effocr_pvt_op_attention(_lib.ptr(q), _lib.ptr(kv), B, N, M, heads, hd, _lib.PREC[prec], _lib.ptr(out),
                                                     _lib.current_stream(dev)), "effocr_pvt_op_attention")
        lo, ms, hi, n = windows(attn, 3, 20, dev)
        assert torch.isfinite(out.float()).all()
        flop = 4.0 * B * N * M * C
        floor = (2 * B * N * C + B * M * 2 * C) * es / (COPY_TBS * 1e12) * 1e6
        print(f"RESULT {prec:>9} attention alone, stage {stage}: B={B} queries={N} keys={M} heads={heads} hd={hd}, random data: {ms * 1e3:.1f} us per launch "
              f"({flop / ms / 1e9:.2f} TFLOP/s; its bytes at {COPY_TBS} TB/s: {floor:.1f} us; windows of {n} launches: {lo * 1e3:.1f} .. {hi * 1e3:.1f} us)")
        side = int(round(N ** 0.5))
        h = torch.randn(B * N, hid, generator=g).to(dt).to(dev)
        w = (torch.randn(9, hid, generator=g) / 3).to(dev)
        b = (torch.randn(hid, generator=g) * 0.1).to(dev)
        ho = torch.empty_like(h)

        def dw():
            _lib.pvt_check(L.effocr_pvt_op_dwconv_gelu(_lib.ptr(h), B, side, side, hid, _lib.ptr(w), _lib.ptr(b), _lib.PREC[prec], _lib.ptr(ho),
                                                       _lib.current_stream(dev)), "effocr_pvt_op_dwconv_gelu")
        lo, ms, hi, n = windows(dw, 3, 20, dev)
        assert torch.isfinite(ho.float()).all()
        floor = 2.0 * B * N * hid * es / (COPY_TBS * 1e12) * 1e6
        print(f"RESULT {prec:>9} depthwise 3x3 + GELU alone, stage {stage}: B={B} grid={side}x{side} C={hid}, random data: {ms * 1e3:.1f} us per launch "
              f"(its bytes at {COPY_TBS} TB/s: {floor:.1f} us; windows of {n} launches: {lo * 1e3:.1f} .. {hi * 1e3:.1f} us)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=1024)
    ap.add_argument("--precisions", default="fp16,bf16")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pvt_time.txt"))
    ap.add_argument("--step", nargs="+", help="(internal) run one measurement in this process")
    a = ap.parse_args()
    if a.step:
        if a.step[0] == "encoder":
            step_encoder(a.step[1], a.step[2], a.crops, a.iters)
        else:
            step_kernels(a.step[1])
        return 0
    precs = a.precisions.split(",")
    steps = [("encoder", arch, prec) for prec in precs for arch in PVTS + SCALE] + [("kernels", prec) for prec in precs]
    lines = [f"python tools/pvt_time.py --crops {a.crops} --precisions {a.precisions} --iters {a.iters}   (1x MI355X; seeded weights; measured, nothing assumed)",
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
