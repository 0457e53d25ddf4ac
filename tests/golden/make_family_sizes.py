#!/usr/bin/env python
"""Records tests/golden/family_sizes.json: what every encoder-family library reports, through its C ABI alone, about the size of each
architecture it accepts — embed_dim, num_params, weights_bytes and workspace_bytes(b) with the default sub-batch and after
set_chunk(3).  No GPU: create and the size queries touch host memory only.

  python tests/golden/make_family_sizes.py [--libdir effocr_amd] [--out tests/golden/family_sizes.json]

The committed fixture was recorded from a build of the commit before the families' host code moved onto shared cores (enc_core.hpp's
enc_default_chunk, token_core.hpp, resnet_core.hpp); tests/test_family_sizes_host.py holds every later build to it.  Re-record it only
for a change that is meant to move a blob, a workspace or a default sub-batch, from a build of that change."""
import argparse
import ctypes
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
PRECISIONS = {"bf16": 0, "fp16": 1, "fp32": 2}
BATCHES = (1, 2, 7, 255, 256, 257, 1000, 4096)
# family -> (every architecture its create accepts, image sizes: the smallest accepted, 64 where accepted, 224)
FAMILIES = {
    "swin": (["swin_tiny_patch4_window7_224"], [224]),
    "resnet": (["resnet34", "resnet50"], [32, 64, 224]),
    "mnv3": (["mobilenetv3_small_050", "mobilenetv3_small_075", "mobilenetv3_small_100", "mobilenetv3_large_100"], [32, 64, 224]),
    "effnet": (["efficientnet_b0", "tf_efficientnet_b0"], [32, 64, 224]),
    "beit": (["beit_base_patch16_224", "beitv2_base_patch16_224", "beit_tiny_test"], [16, 64, 224]),
    "bit": (["resnetv2_50x1_bitm", "resnetv2_50x1_bit", "resnetv2_101x1_bitm", "resnetv2_101x1_bit"], [32, 64, 224]),
    "vit8": (["vit_small_patch8_224", "vit_base_patch8_224", "vit8_tiny_test"], [8, 64, 224]),
}


def _bind(libdir, fam):
    L = ctypes.CDLL(os.path.join(libdir, f"libeffocr_{fam}.so"))
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    sig = {"create": (i32, [ctypes.c_char_p, i32, i32, ctypes.POINTER(vp)]), "destroy": (None, [vp]), "embed_dim": (i32, [vp]),
           "num_params": (i32, [vp]), "weights_bytes": (sz, [vp]), "workspace_bytes": (sz, [vp, i32]), "set_chunk": (i32, [vp, i32]),
           "last_error": (ctypes.c_char_p, [])}
    fns = {}
    for name, (res, args) in sig.items():
        fn = getattr(L, f"effocr_{fam}_{name}")
        fn.restype, fn.argtypes = res, args
        fns[name] = fn
    return fns


def record(libdir):
    """{"<family>/<arch>/<img>/<precision>": [embed_dim, num_params, weights_bytes, [workspace_bytes(b), default sub-batch],
    [workspace_bytes(b) after set_chunk(3)]]} with b over BATCHES."""
    out = {}
    for fam, (archs, imgs) in FAMILIES.items():
        f = _bind(libdir, fam)
        for arch in archs:
            for img in imgs:
                for pname, prec in PRECISIONS.items():
                    h = ctypes.c_void_p()
                    rc = f["create"](arch.encode(), img, prec, ctypes.byref(h))
                    if rc != 0:
                        raise RuntimeError(f"{fam} create({arch}, {img}, {pname}) = {rc}: {f['last_error']().decode()}")
                    try:
                        row = [f["embed_dim"](h), f["num_params"](h), f["weights_bytes"](h)]
                        for chunk in (0, 3):
                            if f["set_chunk"](h, chunk) != 0:
                                raise RuntimeError(f"{fam} set_chunk({chunk}): {f['last_error']().decode()}")
                            row.append([f["workspace_bytes"](h, b) for b in BATCHES])
                    finally:
                        f["destroy"](h)
                    out[f"{fam}/{arch}/{img}/{pname}"] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libdir", default=os.path.join(HERE, "..", "..", "effocr_amd"))
    ap.add_argument("--out", default=os.path.join(HERE, "family_sizes.json"))
    a = ap.parse_args()
    rows = record(a.libdir)
    with open(a.out, "w") as fp:       # one case per line: a change of one case is a one-line diff
        fp.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in rows.items()) + "\n}\n")
    print(f"{len(rows)} cases -> {a.out}")


if __name__ == "__main__":
    main()
