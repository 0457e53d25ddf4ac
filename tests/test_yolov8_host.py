"""Host side of the YOLOv8 n / s / m / l / x localizers (no GPU): the parameter tables against the module tree of tests/yolov8_ref.py and
the parameter counts ultralytics publishes, scale inference from a checkpoint and its refusals, the functional restatement against the
module tree, one hand-computed anchor of the decode, and libeffocr_yolov8.so's handle tables, sizes, refusals and exports."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

from effocr_amd import _lib
from effocr_amd.localizer_engine import (YOLOV8_SCALES, init_yolov5_state_dict, init_yolov8_state_dict, yolov5_scale, yolov8_param_shapes,
                                         yolov8_scale)
from tests.yolov8_ref import SCALES as REF_SCALES, YoloV8, decode, yolov8_forward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = "nsmlx"
# learnable parameters (conv weights, BN weight and bias, the biased 1x1 convs, the 16 DFL weights; BN running statistics are buffers):
# the nc = 80 counts are the ones ultralytics prints in its model summaries (3.2 / 11.2 / 25.9 / 43.7 / 68.2 M)
COUNTS = {80: {"n": 3157200, "s": 11166560, "m": 25902640, "l": 43691520, "x": 68229648},
          2: {"n": 3011238, "s": 11136374, "m": 25857478, "l": 43631382, "x": 68154534}}


def _learnable(shapes):
    return sum(torch.Size(s).numel() for k, s in shapes.items() if not (k.endswith("running_mean") or k.endswith("running_var")))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("nc", [80, 2])
def test_pinned_parameter_counts(scale, nc):
    assert _learnable(yolov8_param_shapes(nc, scale)) == COUNTS[nc][scale]


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("nc", [1, 2, 80])
def test_param_shapes_match_the_module_tree(scale, nc):
    """Same keys, same shapes, same (module) order; and the module tree's own parameter count at nc = 80 is the published one."""
    m = YoloV8(nc, scale)
    want = [(k, tuple(v.shape)) for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked")]
    assert [(k, tuple(v)) for k, v in yolov8_param_shapes(nc, scale).items()] == want
    assert want[-1][0] == "model.22.dfl.conv.weight"
    if nc in COUNTS:
        assert sum(p.numel() for p in m.parameters()) == COUNTS[nc][scale]
    assert YOLOV8_SCALES == REF_SCALES


@pytest.mark.parametrize("scale", SCALES)
def test_scale_round_trips(scale):
    sd = init_yolov8_state_dict(2, scale, seed=1)
    assert yolov8_scale(sd) == scale
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v) for k, v in yolov8_param_shapes(2, scale).items()}
    again = init_yolov8_state_dict(2, scale, seed=1)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    with pytest.raises(ValueError, match="unknown YOLOv8 scale"):
        yolov8_param_shapes(2, "z")


@pytest.mark.parametrize("scale", SCALES)
def test_mismatched_dicts_are_refused(scale):
    sd = init_yolov8_state_dict(2, scale, seed=1)
    bad = dict(sd)
    w = bad["model.3.conv.weight"]                                   # one channel count changed
    bad["model.3.conv.weight"] = torch.zeros(w.shape[0] + 8, *w.shape[1:])
    with pytest.raises(ValueError, match="model.3.conv.weight"):
        yolov8_scale(bad)
    last = max(int(k.split(".")[3]) for k in sd if k.startswith("model.2.m."))
    dropped = {k: v for k, v in sd.items() if not k.startswith(f"model.2.m.{last}.")}   # one bottleneck of model.2 dropped
    with pytest.raises(ValueError, match="model.2"):
        yolov8_scale(dropped)
    one = {k: v for k, v in sd.items() if k != "model.6.cv2.bn.running_var"}             # one tensor dropped
    with pytest.raises(ValueError, match="missing model.6.cv2.bn.running_var"):
        yolov8_scale(one)
    dfl = dict(sd)                                                                       # a DFL tensor that is not 0 .. 15
    dfl["model.22.dfl.conv.weight"] = sd["model.22.dfl.conv.weight"].flip(1)
    with pytest.raises(ValueError, match="model.22.dfl.conv.weight is not the constant"):
        yolov8_scale(dfl)


def test_other_networks_are_refused():
    v5 = init_yolov5_state_dict(2, "s", seed=0)
    with pytest.raises(ValueError, match="not an ultralytics YOLOv8"):
        yolov8_scale(v5)
    v8 = init_yolov8_state_dict(2, "s", seed=0)
    with pytest.raises(ValueError, match="state dict has no 'model.24.m.0.bias'"):      # and the YOLOv5 side says what it always said
        yolov5_scale(v8)
    v8["model.0.conv.weight"] = torch.zeros(24, 3, 3, 3)
    with pytest.raises(ValueError, match="24 output channels"):
        yolov8_scale(v8)


def test_l_with_a_wrong_max_channels_is_refused():
    """yolov8l caps its channels at 512: a dict with model.7 (and what follows it) widened to 1024 has l's stem and depth but is not l."""
    sd = init_yolov8_state_dict(2, "l", seed=0)
    w = sd["model.7.conv.weight"]
    sd["model.7.conv.weight"] = torch.zeros(1024, *w.shape[1:])
    for s in ("weight", "bias", "running_mean", "running_var"):
        sd[f"model.7.bn.{s}"] = torch.zeros(1024)
    with pytest.raises(ValueError, match=r"does not match yolov8l: model.7.conv.weight: shape \(1024, 512, 3, 3\) != \(512, 512, 3, 3\)"):
        yolov8_scale(sd)


@pytest.mark.parametrize("scale", SCALES)
def test_functional_restatement_matches_the_module_tree(scale):
    sd = init_yolov8_state_dict(2, scale, seed=3)
    m = YoloV8(2, scale)
    res = m.load_state_dict(sd, strict=False)                        # strict apart from BN's num_batches_tracked
    assert not res.unexpected_keys and all(k.endswith("num_batches_tracked") for k in res.missing_keys)
    m.eval()
    x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        a, b = m(x), yolov8_forward(sd, x, scale, dtype=torch.float32)
    assert a.shape == b.shape == (2, 8 * 12 + 4 * 6 + 2 * 3, 7)
    assert (a - b).abs().max().item() < 1e-5 * a.abs().max().item()
    assert (a[..., 4] == 1).all()
    wh = a[..., 2:4] / torch.tensor([8.0] * 96 + [16.0] * 24 + [32.0] * 6).view(1, -1, 1)
    assert wh.std().item() > 1.0                                     # the seeded box branch does not give every anchor the same box


def test_decode_of_one_hand_computed_anchor():
    """Level stride 16, a 2 x 3 map, anchor (y 1, x 2): side logits that are one-hot-ish give distances that can be written down.
    left: all mass on bin 3 -> 3; top: equal mass on bins 0 and 15 -> 7.5; right: uniform -> 7.5; bottom: logits ln(1), ln(3) on bins
    2 and 6 -> (2 + 18) / 4 = 5.  Anchor point (2.5, 1.5): x1 = -0.5, y1 = -6, x2 = 10, y2 = 6.5."""
    box = torch.full((1, 64, 2, 3), -1e4, dtype=torch.float64)
    box[0, 0:16, 1, 2] = -1e4
    box[0, 3, 1, 2] = 0.0
    box[0, 16 + 0, 1, 2] = box[0, 16 + 15, 1, 2] = 2.0
    box[0, 32:48, 1, 2] = 0.25
    box[0, 48 + 2, 1, 2], box[0, 48 + 6, 1, 2] = math.log(1.0), math.log(3.0)
    box[0, :, 0, 0] = 0.0                                            # every other anchor: something finite
    cls = torch.zeros((1, 2, 2, 3), dtype=torch.float64)
    cls[0, 0, 1, 2], cls[0, 1, 1, 2] = math.log(3.0), -math.log(3.0)
    row = decode(box, cls, 16.0)[0, 1 * 3 + 2]
    want = torch.tensor([(-0.5 + 10) / 2 * 16, (-6 + 6.5) / 2 * 16, 10.5 * 16, 12.5 * 16, 1.0, 0.75, 0.25], dtype=torch.float64)
    assert torch.allclose(row, want, rtol=0, atol=1e-9), (row, want)
    first = decode(box, cls, 16.0)[0, 0]                             # uniform everywhere: 7.5 bins a side around (0.5, 0.5)
    assert torch.allclose(first[:4], torch.tensor([0.5 * 16, 0.5 * 16, 15 * 16.0, 15 * 16.0], dtype=torch.float64), atol=1e-9)


# ---------------------------------------------------------------- libeffocr_yolov8.so
def _handle(L, arch, nc, h=640, w=640):
    hnd = ctypes.c_void_p()
    rc = L.effocr_yolov8_create(arch, nc, h, w, ctypes.byref(hnd))
    return rc, hnd


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("nc", [1, 2])
def test_cabi_handle_table_equals_the_python_table(scale, nc):
    L = _lib.yolov8_lib()
    rc, h = _handle(L, f"yolov8{scale}".encode(), nc)
    assert rc == 0
    try:
        n = L.effocr_yolov8_num_params(h)
        got = [(L.effocr_yolov8_param_name(h, i).decode(), L.effocr_yolov8_param_numel(h, i)) for i in range(n)]
        want = [(k, torch.Size(v).numel()) for k, v in yolov8_param_shapes(nc, scale).items()]
        assert sorted(got) == sorted(want)
        assert L.effocr_yolov8_num_predictions(h) == 8400 and L.effocr_yolov8_num_outputs(h) == nc + 5
        conv_w = sum(torch.Size(v).numel() for v in yolov8_param_shapes(nc, scale).values() if len(v) == 4)
        assert L.effocr_yolov8_weights_bytes(h) >= 4 * conv_w               # at least the folded fp32 weights
        assert L.effocr_yolov8_param_name(h, n) is None and L.effocr_yolov8_param_numel(h, n) == -1
    finally:
        L.effocr_yolov8_destroy(h)


def test_cabi_num_predictions_and_sizes_follow_shape_and_scale():
    L = _lib.yolov8_lib()
    rc, h = _handle(L, b"yolov8n", 2, 64, 96)
    assert rc == 0 and L.effocr_yolov8_num_predictions(h) == 126
    L.effocr_yolov8_destroy(h)
    ws, wb = {}, {}
    for scale in SCALES:
        rc, h = _handle(L, f"yolov8{scale}".encode(), 2)
        assert rc == 0
        ws[scale] = L.effocr_yolov8_workspace_bytes(h, 16)
        wb[scale] = L.effocr_yolov8_weights_bytes(h)
        assert L.effocr_yolov8_workspace_bytes(h, 0) == 0
        L.effocr_yolov8_set_option(h, b"direct_stem", 0)                    # the im2col rows exist only on the cross-check path
        assert L.effocr_yolov8_workspace_bytes(h, 16) == ws[scale] + 16 * 320 * 320 * 32 * 4
        L.effocr_yolov8_destroy(h)
    assert ws["n"] < ws["s"] < ws["m"] < ws["l"] < ws["x"]
    assert wb["n"] < wb["s"] < wb["m"] < wb["l"] < wb["x"]


def test_cabi_refusals():
    L = _lib.yolov8_lib()
    for bad in (b"yolov5s", b"yolov8s6", b"yolov8s-seg", b"yolov8", b"", b"yolov8z"):
        rc, h = _handle(L, bad, 2)
        assert rc == -2 and not h.value, bad
        assert b"unsupported architecture" in L.effocr_yolov8_last_error()
    for nc, hh, ww in ((0, 640, 640), (81, 640, 640), (2, 0, 640), (2, 640, 650), (2, -32, 64)):
        rc, h = _handle(L, b"yolov8s", nc, hh, ww)
        assert rc == -1 and not h.value, (nc, hh, ww)
    rc, h = _handle(L, b"yolov8n", 2, 64, 64)
    assert rc == 0
    try:
        one = (ctypes.c_float * 1)(0.0)
        assert L.effocr_yolov8_set_param(h, b"model.24.anchors", one, 1) == -1
        assert L.effocr_yolov8_set_param(h, b"model.22.dfl.conv.weight", one, 1) == -1
        assert b"expects 16 elements" in L.effocr_yolov8_last_error()
        assert L.effocr_yolov8_set_option(h, b"no_such_option", 1) == -1
        assert L.effocr_yolov8_set_option(h, b"call_size_invariant", 2) == -1
        assert L.effocr_yolov8_upload(h, ctypes.c_void_p(256), 1 << 40) == -5   # parameters never set: refused before any copy
    finally:
        L.effocr_yolov8_destroy(h)


def test_library_exports_its_header_and_nothing_of_the_product_library():
    src = open(os.path.join(ROOT, "include", "effocr_yolov8.h")).read()
    declared = sorted(set(re.findall(r"\b(effocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert len(declared) == 17                               # 15 + the two test entry points (effocr_yolov8_op_decode, _op_stem)
    assert sorted(_lib.YOLOV8_EXPORTS) == declared
    v = int(re.search(r"#define\s+EFFOCR_YOLOV8_ABI_VERSION\s+(\d+)", src).group(1))
    assert _lib.yolov8_lib().effocr_yolov8_abi_version() == v == _lib.YOLOV8_ABI_VERSION == 1
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.YOLOV8_SO_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in nm.splitlines()) == declared
    _lib.lib()
    assert not set(declared) & set(_lib.EXPORTS)
    raw = ctypes.CDLL(_lib.YOLOV8_SO_PATH)
    for hidden in ("effocr_abi_version", "effocr_localizer_create", "effocr_nms", "effocr_letterbox"):
        assert not hasattr(raw, hidden), hidden
    assert not hasattr(ctypes.CDLL(_lib.SO_PATH), "effocr_yolov8_create")
