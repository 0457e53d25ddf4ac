"""-m gpu: the call-size-invariant mode (DESIGN.md "Call-size-invariant mode").  With ``call_size_invariant=True`` the output row of a
crop / image is a function of its pixels, the weights, the precision and the image size only: the SAME bits in every call size, at every
position of the call, beside any other items, under ``chunk`` and under the engines' own sub-batching.  Every comparison is
``torch.equal``, on raw and on L2-normalised embeddings; the guards pin that the default mode really does differ on these shapes."""
import functools

import numpy as np
import pytest
import torch

from effocr_amd.weights import init_state_dict

pytestmark = pytest.mark.gpu

REL = {"fp32": 1e-5, "fp16": 1e-3, "bf16": 8e-3}       # tests/test_gpu_encoder.py: the 16-bit modes against the fp32 arithmetic


@functools.lru_cache(maxsize=None)
def _sd(arch, img):
    return init_state_dict(arch, seed=3, img_size=img)


def _probes(dev, img, n=6, seed=21):
    return torch.randn(n, 3, img, img, generator=torch.Generator(device=dev).manual_seed(seed), device=dev)


def _call(probes, B, places, dev):
    """A call of B crops: fillers from a seed of its own, the probes copied in at every offset of ``places`` (as many as fit)."""
    img = probes.shape[-1]
    x = torch.randn(B, 3, img, img, generator=torch.Generator(device=dev).manual_seed(1000 + B), device=dev)
    for p in places:
        k = min(probes.shape[0], B - p)
        x[p:p + k] = probes[:k]
    return x


def _assert_rows(enc, probes, ref, B, places, dev, what):
    """The probes' rows of a B-crop call equal the rows ``ref`` = (raw, normalised) of the probes' own call, bit for bit."""
    x = _call(probes, B, places, dev)
    for normalize, want in zip((False, True), ref):
        out = enc.forward(x, normalize=normalize)
        for p in places:
            k = min(probes.shape[0], B - p)
            assert torch.equal(out[p:p + k], want[:k]), f"{what}: {B} crops, probes at {p}, normalize={normalize}: " \
                                                        f"max diff {(out[p:p + k] - want[:k]).abs().max().item():.3e}"


def _reference(enc, probes):
    return enc.forward(probes, normalize=False).clone(), enc.forward(probes, normalize=True).clone()


# both sides of every boundary of launch_mlp (13 | 14, 27 | 28, 36 | 37, 83 | 84) and of HipEncoder._split_plan (88, 131 | 132), a full
# round of 128-token panels plus a tail (200 crops = 308 panels on 256 CUs), more images than CUs (300: the per-image kernel's tail launch)
VIT_S_SIZES = (1, 13, 14, 27, 28, 36, 37, 83, 84, 88, 131, 132, 200, 300)


def _places(B):
    if B < 200:
        return (0,)
    # the front, the last six, and six that straddle the seam of the side-stream sub-batches (two of 100 / three of 100 crops)
    return (0, 97, B - 6)


@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_vit_small(dev, prec):
    from effocr_amd.encoders import HipEncoder
    arch = "vit_small_patch16_224"
    enc = HipEncoder(arch, _sd(arch, 224), precision=prec, device=dev, call_size_invariant=True)
    assert enc.call_size_invariant is True
    probes = _probes(dev, 224)
    ref = _reference(enc, probes)
    for B in VIT_S_SIZES:
        _assert_rows(enc, probes, ref, B, _places(B), dev, f"{arch} {prec}")
    # one call, no side streams: 300 crops = 462 panels, the probes across the end of the first full round (crop 166 spans panels 255 | 256)
    enc.split_streams = False
    _assert_rows(enc, probes, ref, 300, (0, 164, 294), dev, f"{arch} {prec}, one stream")
    enc.split_streams = True
    enc.check_status()
    enc.set_option("chunk", 5)
    for B in VIT_S_SIZES:
        _assert_rows(enc, probes, ref, B, _places(B), dev, f"{arch} {prec}, chunk 5")
    enc.set_chunk(0)
    enc.check_status()


def test_vit_small_default_mode_depends_on_the_call_size(dev):
    """The guard of the test above: with the mode off, the raw fp16 embeddings of the probes differ between the 6- and the 64-crop call
    (pair parts against whole pair panels).  If this ever stops holding, these shapes prove nothing: pick others."""
    from effocr_amd.encoders import HipEncoder
    arch = "vit_small_patch16_224"
    enc = HipEncoder(arch, _sd(arch, 224), precision="fp16", device=dev)
    assert enc.call_size_invariant is False
    probes = _probes(dev, 224)
    six = enc.forward(probes).clone()
    mid = enc.forward(_call(probes, 64, (0,), dev))[:6]
    assert not torch.equal(six, mid)


@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_vit_base(dev, prec):
    """fp16 / bf16: 40 and 70 crops cross one round of gemm3 tiles (fc1: 31 x 12 against 54 x 12 tiles on 256 CUs), so its tail launch
    and tile heights change; the probes at both ends.  fp32: 1 and 6 crops."""
    from effocr_amd.encoders import HipEncoder
    arch = "vit_base_patch16_224"
    enc = HipEncoder(arch, _sd(arch, 224), precision=prec, device=dev, call_size_invariant=True)
    probes = _probes(dev, 224, seed=22)
    ref = _reference(enc, probes)
    _assert_rows(enc, probes, ref, 1, (0,), dev, f"{arch} {prec}")
    if prec != "fp32":
        for B in (40, 70):
            _assert_rows(enc, probes, ref, B, (0, B - 6), dev, f"{arch} {prec}")
    enc.check_status()


RESNET_SIZES = {224: (1, 6, 40), 32: (1, 64, 300)}


@pytest.mark.parametrize("img", [224, 32])
def test_resnet18(dev, img):
    from effocr_amd.encoders import HipEncoder
    sd = _sd("resnet18", img)
    enc = HipEncoder("resnet18", sd, img_size=img, precision="fp32", device=dev, call_size_invariant=True)
    probes = _probes(dev, img, seed=23)
    ref = _reference(enc, probes)
    for B in RESNET_SIZES[img]:
        _assert_rows(enc, probes, ref, B, (0, B - 6) if B > 12 else (0,), dev, f"resnet18 {img}")


def test_resnet18_default_mode_depends_on_the_call_size(dev):
    """Guard: in default mode at least one pair of the call sizes above gives the first crop different bits (split-K counts that follow
    the launch's tile count)."""
    from effocr_amd.encoders import HipEncoder
    differs = []
    for img, sizes in RESNET_SIZES.items():
        enc = HipEncoder("resnet18", _sd("resnet18", img), img_size=img, precision="fp32", device=dev)
        probes = _probes(dev, img, seed=23)
        rows = [enc.forward(_call(probes, B, (0,), dev))[:1].clone() for B in sizes]
        differs += [not torch.equal(rows[0], r) for r in rows[1:]]
    print("resnet18, default mode, first crop differs from its 1-crop call:", differs)
    assert any(differs)


# Where the default mode's split-K counts differ, from conv2d_nhwc's rule (a launch of g tiles with nks K stages — K / 32 with fp32
# operands, ceil(K / 64) with bf16 — is cut min(CUs / g, nks / 2, 32)-way while 2 g <= CUs and nks >= 8; 256 CUs).  The layer that decides
# is model.7, the 3 x 3 stride-2 convolution into P5 (s: 256 -> 512 channels, K = 2304; n: 128 -> 256, K = 1152):
#   320^2, 100 P5 pixels per image   s fp32: 4 tiles at B = 1 (32-way) against 12 at B = 3 (21-way); n fp32: the 3 x 3 convolutions of
#                                    model.2 (6400 pixels: 50 tiles, 4-way) against B = 3 (150 tiles: no split)
#                                    s bf16: 36 stages cap B = 1 and B = 3 at 18-way alike, B = 8 is 28 tiles: 9-way
#                                    n bf16: 18 stages cap every call of up to 18 images at 9-way, model.2 has too few stages to split:
#                                    NO pair of calls at this size differs, so this size alone would prove nothing for n bf16
#   640^2, 400 P5 pixels per image   B = 1 against B = 8: s 16 against 100 tiles (16-way / 2-way), n 8 against 50 tiles (fp32 18-way /
#                                    5-way, bf16 9-way / 5-way): all four differ
# (scale, precision) -> the batch sizes whose default-mode bits must differ from the 1-image call at 320^2; at 640^2 it is B = 8 for all
GUARD_320 = {("s", "fp32"): (3, 8), ("n", "fp32"): (3,), ("s", "bf16"): (8,), ("n", "bf16"): ()}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("scale", ["s", "n"])
def test_localizer(dev, scale, precision):
    """The same image alone, first of 3 and last of 8 at 320 x 320, and alone against last of 8 at 640 x 640: raw predictions bit-equal
    in the mode.  Guard, asserted in every parametrisation: with the mode off the same calls give the image other bits — B = 1 against
    B = 3 with fp32 operands (yolov5s and yolov5n), against B = 8 for yolov5s with bf16 operands, and B = 1 against B = 8 at 640 x 640 for
    all four (the only size at which yolov5n with bf16 operands crosses a split boundary: table above).  After on -> off the handle
    gives the bits of a localizer that never had the mode on."""
    from effocr_amd.localizer_engine import HipLocalizer, init_yolov5_state_dict
    sd = init_yolov5_state_dict(2, scale, seed=1)
    for size in (320, 640):
        g = torch.Generator(device=dev).manual_seed(5)
        im = torch.rand(1, 3, size, size, generator=g, device=dev)
        calls = {}                                                          # batch size -> (the call, the image's position in it)
        if size == 320:
            calls[3] = (torch.rand(3, 3, size, size, generator=g, device=dev), 0)
        calls[8] = (torch.rand(8, 3, size, size, generator=g, device=dev), 7)
        for x, pos in calls.values():
            x[pos] = im[0]
        loc = HipLocalizer(sd, input_shape=(size, size), device=dev, precision=precision, call_size_invariant=True)
        assert loc.call_size_invariant is True
        one = loc.forward(im).clone()
        assert torch.isfinite(one).all()
        for B, (x, pos) in calls.items():
            assert torch.equal(loc.forward(x)[pos], one[0]), (size, B)
        loc.set_option("call_size_invariant", 0)
        d1 = loc.forward(im).clone()
        dB = {B: loc.forward(x)[pos].clone() for B, (x, pos) in calls.items()}
        for B, d in dB.items():
            print(f"yolov5{scale} {precision} {size}^2, default mode: B = 1 and B = {B} {'differ' if not torch.equal(d1[0], d) else 'agree'}, "
                  f"max diff {(d1[0] - d).abs().max().item():.3e}")
        for B in (GUARD_320[(scale, precision)] if size == 320 else (8,)):
            assert not torch.equal(d1[0], dB[B]), (size, B)
        fresh = HipLocalizer(sd, input_shape=(size, size), device=dev, precision=precision)
        assert torch.equal(fresh.forward(im), d1)
        for B, (x, pos) in calls.items():
            assert torch.equal(fresh.forward(x)[pos], dB[B]), (size, B)


def test_run_effocr_does_not_depend_on_lines_per_chunk(dev):
    """12 synthetic lines through run_effocr with both engines in the mode: the strings of lines_per_chunk 1 and 16 are identical.
    run_effocr returns no boxes, so the character boxes are compared by PROXY: the localizer's kept rows (boxes, scores, classes — what
    the box stage of run_effocr is computed from, per line) of every line alone, as lines_per_chunk = 1 sends it, and inside the 12-line
    call, as lines_per_chunk = 16 sends it."""
    from effocr_amd.knn import FaissKNN, IndexFlatIP
    from effocr_amd.localizer_engine import EffLocalizer, init_yolov5s_state_dict
    from effocr_amd.pipeline import run_effocr
    from effocr_amd.recognizer_engine import EffRecognizer
    from effocr_amd.transforms import PairedTransform
    chars = [chr(0x4E00 + i) for i in range(226)]
    loc_sd = init_yolov5s_state_dict(2, seed=2)
    for l in range(3):                                                      # a Detect head that fires: tens of character boxes per line
        b = loc_sd[f"model.24.m.{l}.bias"].view(3, 7)
        b[:, 4] += 5.5
        b[:, 5] += 2.5
        b[:, 6] += 2.4
    loc = EffLocalizer(loc_sd, iou_thresh=0.05, conf_thresh=0.5, device=dev, call_size_invariant=True)
    arch = "vit_small_patch16_224"
    rec = EffRecognizer(_sd(arch, 224), arch=arch, precision="fp16", device=dev, call_size_invariant=True)
    assert loc.call_size_invariant and rec.call_size_invariant
    tf = PairedTransform(size=224, device=dev)
    rng = np.random.default_rng(31)
    lines = [(rng.integers(0, 256, (256, 2048, 3)) // 32 * 32).astype(np.uint8) for _ in range(12)]
    index = torch.nn.functional.normalize(torch.randn(len(chars), 384, generator=torch.Generator().manual_seed(1)), dim=1)
    knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False, device=dev)
    knn.train(index)
    a, _ = run_effocr(lines, loc, rec, tf, "jp", knn_func=knn, candidate_chars=chars, lines_per_chunk=1)
    b, _ = run_effocr(lines, loc, rec, tf, "jp", knn_func=knn, candidate_chars=chars, lines_per_chunk=16)
    assert a == b
    assert sum(len(s) for s in a.values()) >= 60, a                         # the lines really carry text
    together = loc.run(lines)
    for i, line in enumerate(lines):
        alone = loc.run([line])[0]
        assert torch.equal(alone, together[i]), i


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_switching_the_mode_off_restores_the_default_bits(dev, prec):
    """The mode overrides the A/B switches without overwriting them: after on -> off the handle gives the bits of an engine that never
    had it on, with the caller's own mlp_pair = -1 back in force (64 crops: the hidden-split parts instead of the pair panels)."""
    from effocr_amd.encoders import HipEncoder
    arch = "vit_small_patch16_224"
    x = _call(_probes(dev, 224), 64, (0,), dev)
    plain = HipEncoder(arch, _sd(arch, 224), precision=prec, device=dev)
    nopair = HipEncoder(arch, _sd(arch, 224), precision=prec, device=dev)
    nopair.set_option("mlp_pair", -1)
    want = {False: (plain.forward(x).clone(), plain.forward(x[:6].contiguous()).clone()),
            True: (nopair.forward(x).clone(), nopair.forward(x[:6].contiguous()).clone())}
    assert not torch.equal(want[False][0], want[True][0])                   # the switch is really another form at 64 crops
    for pair_off in (False, True):
        enc = HipEncoder(arch, _sd(arch, 224), precision=prec, device=dev)
        if pair_off:
            enc.set_option("mlp_pair", -1)
        enc.set_option("call_size_invariant", 1)
        inv = enc.forward(x).clone()
        assert torch.equal(inv[:6], enc.forward(x[:6].contiguous()))
        enc.set_option("call_size_invariant", 0)
        assert enc.call_size_invariant is False
        assert torch.equal(enc.forward(x), want[pair_off][0]) and torch.equal(enc.forward(x[:6].contiguous()), want[pair_off][1])


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_rows_do_not_depend_on_the_world_size(dev, prec):
    """dist.ShardedRecognizer hands rank r of a world of w the crops shard_bounds(n, r, w) of a call: in the mode the rows the ranks
    compute, put together, are the rows of the whole call for every world size (one process, the slices one after the other: the
    engines are per rank, so this is the arithmetic each rank does)."""
    from effocr_amd.dist import shard_bounds
    from effocr_amd.encoders import HipEncoder
    arch = "vit_small_patch16_224"
    enc = HipEncoder(arch, _sd(arch, 224), precision=prec, device=dev, call_size_invariant=True)
    x = _call(_probes(dev, 224), 100, (0,), dev)
    whole = enc.forward(x, normalize=True).clone()
    for world in (2, 3, 8):
        parts = [enc.forward(x[lo:hi].contiguous(), normalize=True) for lo, hi in (shard_bounds(100, r, world) for r in range(world))]
        assert torch.equal(torch.cat(parts), whole), world
    enc.check_status()


def test_the_attention_path_does_not_follow_the_batch_in_the_mode(dev):
    """qa_min_batch picks between the fused qkv+attention kernel and the token-panel pair by B.  The mode takes it as 1: a caller's
    qa_min_batch = 32 changes nothing while the mode is on (6 crops below it, 40 above: the same rows as without the switch)."""
    from effocr_amd.encoders import HipEncoder
    arch = "vit_small_patch16_224"
    enc = HipEncoder(arch, _sd(arch, 224), precision="fp16", device=dev, call_size_invariant=True)
    probes = _probes(dev, 224)
    ref = _reference(enc, probes)
    enc.set_option("qa_min_batch", 32)
    assert torch.equal(enc.forward(probes), ref[0])
    _assert_rows(enc, probes, ref, 40, (0, 34), dev, "qa_min_batch = 32")
    enc.check_status()


def test_the_other_fused_mlp_switches_still_reach_the_kernel(dev):
    """The mode sits on the line that hands the A/B switches to the fused MLP: with it off, pair_parts = 0 still selects another form
    for a 16-crop call (the 128-token parts: other bits) — before the mode was ever on and after on -> off — and with it on the switch
    changes nothing."""
    from effocr_amd.encoders import HipEncoder
    arch = "vit_small_patch16_224"
    x = _call(_probes(dev, 224), 16, (0,), dev)
    enc = HipEncoder(arch, _sd(arch, 224), precision="fp16", device=dev)
    plain = enc.forward(x).clone()
    enc.set_option("pair_parts", 0)
    parts = enc.forward(x).clone()
    assert not torch.equal(plain, parts)
    enc.set_option("call_size_invariant", 1)
    inv = enc.forward(x).clone()
    enc.set_option("pair_parts", 1)
    assert torch.equal(enc.forward(x), inv)
    enc.set_option("pair_parts", 0)
    enc.set_option("call_size_invariant", 0)
    assert torch.equal(enc.forward(x), parts)
    enc.set_option("pair_parts", 1)
    assert torch.equal(enc.forward(x), plain)


@pytest.mark.parametrize("arch", ["vit_small_patch16_224", "vit_base_patch16_224"])
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_accuracy_in_the_mode(dev, arch, prec):
    """The mode's embeddings stay within the precision's bound of the library's exact-fp32 mode."""
    from effocr_amd.encoders import HipEncoder
    probes = _probes(dev, 224, seed=24)
    ref = HipEncoder(arch, _sd(arch, 224), precision="fp32", device=dev).forward(probes, normalize=True).cpu()
    enc = HipEncoder(arch, _sd(arch, 224), precision=prec, device=dev, call_size_invariant=True)
    got = enc.forward(probes, normalize=True).cpu()
    enc.check_status()
    e = ((got - ref).abs().max() / ref.abs().max()).item()
    r2 = ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
    print(f"{arch} {prec}, call-size-invariant: rel err {e:.3e} (max norm), worst row rel L2 {r2:.3e}")
    assert e <= REL[prec] and r2 <= REL[prec]
