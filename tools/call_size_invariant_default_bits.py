#!/usr/bin/env python
"""Default mode untouched: torch.equal of the default-mode outputs of two builds of libeffocr_hip.so (the parent commit's against this
tree's) on seeded weights and inputs.  Each build runs in a fresh process of its own (EFFOCR_HIP_LIB selects it) and dumps its outputs;
the caller compares the dumps.  The committed output is profiles/call_size_invariant_default_bits.txt.

    python tools/call_size_invariant_default_bits.py PARENT_LIBRARY.so [scratch directory]"""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("vit_small_patch16_224", 224, "bf16", (6, 64, 300)), ("vit_small_patch16_224", 224, "fp16", (6, 64, 300)),
         ("vit_base_patch16_224", 224, "fp16", (64,)), ("resnet18", 32, "fp32", (64,))]
LOC_BATCHES = (1, 3)


def dump(path):
    from effocr_amd.encoders import HipEncoder
    from effocr_amd.localizer_engine import HipLocalizer, init_yolov5s_state_dict
    from effocr_amd.weights import init_state_dict
    dev = torch.device("cuda:0")
    out = {}
    for arch, img, prec, sizes in CASES:
        enc = HipEncoder(arch, init_state_dict(arch, seed=3, img_size=img), img_size=img, precision=prec, device=dev)
        x = torch.randn(max(sizes), 3, img, img, generator=torch.Generator(device=dev).manual_seed(21), device=dev)
        for B in sizes:
            for l2 in (False, True):
                out[f"{arch} {prec} {img}^2 B={B} {'l2' if l2 else 'raw'}"] = enc.forward(x[:B].contiguous(), normalize=l2).cpu()
        enc.check_status()
    loc = HipLocalizer(init_yolov5s_state_dict(2, seed=0), input_shape=(640, 640), device=dev)
    im = torch.rand(max(LOC_BATCHES), 3, 640, 640, generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    for B in LOC_BATCHES:
        out[f"yolov5s fp32 640^2 B={B} predictions"] = loc.forward(im[:B].contiguous()).cpu()
    torch.save(out, path)


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == "--dump":
        return dump(sys.argv[2])
    parent = os.path.abspath(sys.argv[1])
    scratch = sys.argv[2] if len(sys.argv) > 2 else "."
    os.makedirs(scratch, exist_ok=True)
    dumps = []
    for tag, lib in (("parent", parent), ("this", None)):
        env = dict(os.environ)
        env.pop("EFFOCR_HIP_LIB", None)
        if lib:
            env["EFFOCR_HIP_LIB"] = lib
        dumps.append(os.path.join(scratch, f"default_bits_{tag}.pt"))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", dumps[-1]], env=env, check=True, timeout=600)
    a, b = (torch.load(p, weights_only=True) for p in dumps)
    print("# torch.equal of the DEFAULT-mode outputs, parent commit's libeffocr_hip.so vs this tree's: seeded init_state_dict weights, seeded inputs")
    print("# case shape finite equal bits_equal")
    same = 0
    for k in a:
        eq = torch.equal(a[k], b[k])
        bits = torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))
        same += eq and bits
        print(f"{k} {tuple(a[k].shape)} finite={bool(torch.isfinite(a[k]).all())} equal={eq} bits_equal={bits}")
    print(f"# {same} of {len(a)} cases identical")
    return 0 if same == len(a) and list(a) == list(b) else 1


if __name__ == "__main__":
    sys.exit(main())
