#!/usr/bin/env python
"""BiT ResNetV2 encoder and encoder + exact k-NN throughput on one GPU, with resnet50 (libeffocr_resnet.so: the same convolution kernels,
BatchNorm folded into the weights, no normalisation pass) as the yardstick of the same run, and the share of every kernel.

  python tools/bit_time.py [--archs ...] [--sizes 1024] [--precisions fp16] [--iters 10] [--chunk 0] [--out profiles/bit_time.txt]
                           [--no-profile] [--one ARCH,PREC,N]

crops/s of the engine's forward alone and of Recognizer.neighbors (encoder -> fused L2 normalise -> IP top-10 over a 10 000 x 2048 index),
seeded random weights, 224^2 fp32 crops already on the device.  Every call is timed on its own with a CUDA-event pair after 3 warm-up
calls; the median and the fastest of `iters` calls are reported.  The kernel shares come from a child process under
`rocprofv3 --kernel-trace --stats` per architecture (the library has no profiler of its own): `--one ARCH,PREC,N` is that child, two
N-crop forwards after one warm-up call.  The report goes to --out and to the standard output."""
import argparse
import glob
import os
import sqlite3
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from effocr_amd import weights as W                    # noqa: E402

IMG = 224
YARDSTICK = "resnet50"
ARCHS = ["resnetv2_50x1_bitm", "resnetv2_101x1_bitm"]
# substrings of the kernel symbols -> the names DESIGN.md uses
CLASSES = [("bit_gn_stats", "groupnorm statistics"), ("bit_gn_merge", "groupnorm merge"),("bit_gn_apply", "groupnorm apply + relu"), ("bit_stem_pool", "stem pad + pool"),
           ("bit_head", "head"), ("rn_conv16", "convolution (rn_conv16)"), ("rn_im2col16", "stem im2col"), ("rn_maxpool16", "max pool"),
           ("rn_avgpool", "average pool")]


def kernel_class(name):
    for sub, c in CLASSES:
        if sub in name:
            return c
    return name[:48]


def time_calls(fn, dev, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def kernel_shares(arch, prec, n):
    """[(class, launches, total ms, share)] of a fresh child process under rocprofv3 --kernel-trace --stats, by total time."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "stats", "--", sys.executable, os.path.abspath(__file__), "--one",
               f"{arch},{prec},{n}"]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
        dbs = glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)
        if res.returncode != 0 or not dbs:
            raise RuntimeError(f"rocprofv3 failed ({res.returncode}):\n{res.stdout[-2000:]}")
        rows = sqlite3.connect(dbs[0]).execute("select name, count(*), sum(duration) from kernels group by name").fetchall()
    by = {}
    for name, cnt, dur in rows:
        c = by.setdefault(kernel_class(name), [0, 0.0])
        c[0] += cnt
        c[1] += dur / 1e6
    tot = sum(v[1] for v in by.values())
    return sorted(((k, v[0], v[1], v[1] / tot) for k, v in by.items()), key=lambda r: -r[2])


def main():
    from effocr_amd.encoders import make_encoder
    from effocr_amd.knn import FaissKNN, IndexFlatIP
    from effocr_amd.pipeline import Recognizer
    ap = argparse.ArgumentParser()
    ap.add_argument("--archs", default=",".join(ARCHS))
    ap.add_argument("--sizes", default="1024")
    ap.add_argument("--precisions", default="fp16")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=0, help="set_chunk of the engines (0 = each library's default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bit_time.txt"))
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 child processes")
    ap.add_argument("--one", default="", help="ARCH,PREC,N: two N-crop forwards after a warm-up call, then exit (for rocprofv3)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    if a.one:
        arch, prec, n = a.one.split(",")
        enc = make_encoder(arch, W.init_state_dict(arch, seed=0, img_size=IMG), img_size=IMG, precision=prec, device=dev)
        x = torch.randn(int(n), 3, IMG, IMG, generator=g).to(dev)
        enc.forward(x)
        torch.cuda.synchronize(dev)
        enc.forward(x)
        enc.forward(x)
        enc.check_status()
        print(f"two {n}-crop {prec} forwards of {arch} done (after one warm-up forward)")
        return
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    sizes = [int(s) for s in a.sizes.split(",")]
    nmax = max(sizes)
    # the profiled children first, while this process has not opened the GPU: each is a fresh process of its own
    shares = {} if a.no_profile else {arch: kernel_shares(arch, a.precisions.split(",")[0], nmax) for arch in a.archs.split(",")}
    x_all = torch.randn(nmax, 3, IMG, IMG, generator=g).to(dev)
    chars = [chr(0x4E00 + i) for i in range(10000)]
    index = torch.nn.functional.normalize(torch.randn(10000, 2048, generator=g), dim=1)
    say(f"# python tools/bit_time.py --sizes {a.sizes} --precisions {a.precisions} --iters {a.iters} --chunk {a.chunk}   (1x MI355X)")
    say(f"{IMG}^2 crops on the device, {a.iters} timed calls after 3 warm-up calls, each with its own event pair;")
    say("cells: crops/s from the MEDIAN call (crops/s from the fastest call); k-NN: 10 000 x 2048 index, k = 10; one run on one box")
    for arch in [YARDSTICK] + a.archs.split(","):
        sd = W.init_state_dict(arch, seed=0, img_size=IMG)
        say(f"\n{arch}{' (yardstick: folded BatchNorm, no normalisation pass)' if arch == YARDSTICK else ''}")
        say(f"{'':>14} " + " ".join(f"{n:>18}" for n in sizes))
        for prec in a.precisions.split(","):
            enc = make_encoder(arch, sd, img_size=IMG, precision=prec, device=dev)
            enc.set_chunk(a.chunk)
            knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
            knn.train(index)
            rec = Recognizer(enc, knn, chars, knn=10)
            rows = {"encoder": [], "enc+knn": []}
            for n in sizes:
                x = x_all[:n]
                for name, fn in (("encoder", lambda: enc.forward(x)), ("enc+knn", lambda: rec.neighbors(x))):
                    med, best = time_calls(fn, dev, a.iters)
                    rows[name].append(f"{n / med * 1e3:>9.0f} ({n / best * 1e3:>7.0f})")
                enc.check_status()
            for name, cells in rows.items():
                say(f"{prec:>5} {name:>8} " + " ".join(cells))
            del enc, rec, knn
    for arch, rows in shares.items():
        say(f"\n# rocprofv3 --kernel-trace --stats -- python tools/bit_time.py --one {arch},{a.precisions.split(',')[0]},{nmax}   (three forwards)")
        say(f"{'kernel':28s} {'launches':>8s} {'total ms':>10s} {'share':>7s}")
        for k, cnt, ms, share in rows:
            say(f"{k:28s} {cnt:8d} {ms:10.3f} {share:7.1%}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
