"""Host side of the YOLOv5 n / s / m / l / x localizers (no GPU): the parameter tables against the parse_model module tree of
oracle/yolo_modules.py, scale inference from a checkpoint, tests/yolov5_ref.py against both oracle restatements, and the C ABI's
handle tables for every scale."""
import ctypes

import pytest
import torch

from effocr_amd.localizer_engine import (YOLOV5_SCALES, init_yolov5_state_dict, init_yolov5s_state_dict, yolov5_param_shapes,
                                         yolov5_scale, yolov5s_param_shapes)
from oracle.yolo_modules import YoloV5
from tests.yolov5_ref import yolov5_forward

SCALES = "nsmlx"
# learnable parameters at nc = 80: ultralytics publishes 1.9 / 7.2 / 21.2 / 46.5 / 86.7 M
PUBLISHED = {"n": 1872157, "s": 7235389, "m": 21190557, "l": 46563709, "x": 86749405}


def _module_sd(nc, scale):
    d, w = YOLOV5_SCALES[scale]
    return YoloV5(nc, d, w).state_dict()


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("nc", [1, 2, 80])
def test_param_shapes_match_the_module_tree(scale, nc):
    want = {k: tuple(v.shape) for k, v in _module_sd(nc, scale).items() if not k.endswith("num_batches_tracked")}
    got = {k: tuple(v) for k, v in yolov5_param_shapes(nc, scale).items()}
    assert got == want
    assert "model.24.anchors" in got and "model.0.bn.running_var" in got


@pytest.mark.parametrize("scale", SCALES)
def test_published_parameter_counts(scale):
    d, w = YOLOV5_SCALES[scale]
    m = YoloV5(80, d, w)
    assert sum(p.numel() for p in m.parameters()) == PUBLISHED[scale]
    learnable = sum(torch.Size(s).numel() for k, s in yolov5_param_shapes(80, scale).items()
                    if not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("anchors")))
    assert learnable == PUBLISHED[scale]


@pytest.mark.parametrize("scale", SCALES)
def test_scale_round_trips(scale):
    sd = init_yolov5_state_dict(2, scale, seed=1)
    assert yolov5_scale(sd) == scale
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v) for k, v in yolov5_param_shapes(2, scale).items()}


@pytest.mark.parametrize("scale", SCALES)
def test_mismatched_dicts_are_refused(scale):
    sd = init_yolov5_state_dict(2, scale, seed=1)
    bad = dict(sd)
    w = bad["model.3.conv.weight"]                                   # one channel count changed
    bad["model.3.conv.weight"] = torch.zeros(w.shape[0] + 8, *w.shape[1:])
    with pytest.raises(ValueError, match="model.3.conv.weight"):
        yolov5_scale(bad)
    last = max(int(k.split(".")[3]) for k in sd if k.startswith("model.2.m."))
    dropped = {k: v for k, v in sd.items() if not k.startswith(f"model.2.m.{last}.")}   # one bottleneck of model.2 dropped
    with pytest.raises(ValueError, match="model.2"):
        yolov5_scale(dropped)
    one = {k: v for k, v in sd.items() if k != "model.6.cv3.bn.running_var"}             # one tensor dropped
    with pytest.raises(ValueError, match="missing model.6.cv3.bn.running_var"):
        yolov5_scale(one)


def test_width_that_is_no_scale_is_refused():
    sd = init_yolov5_state_dict(2, "s", seed=0)
    sd["model.0.conv.weight"] = torch.zeros(24, 3, 6, 6)
    with pytest.raises(ValueError, match="24 output channels"):
        yolov5_scale(sd)
    with pytest.raises(ValueError, match="not an ultralytics YOLOv5"):
        yolov5_scale({k: v for k, v in sd.items() if not k.startswith("model.24.")})


def test_yolov5s_tables_are_the_generic_s():
    for nc in (1, 2, 80):
        assert list(yolov5s_param_shapes(nc).items()) == list(yolov5_param_shapes(nc, "s").items())
    a, b = init_yolov5s_state_dict(2, 0), init_yolov5_state_dict(2, "s", 0)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(ValueError, match="unknown YOLOv5 scale"):
        yolov5_param_shapes(2, "z")


@pytest.mark.parametrize("scale", SCALES)
def test_functional_restatement_matches_the_module_tree(scale):
    d, w = YOLOV5_SCALES[scale]
    sd = init_yolov5_state_dict(2, scale, seed=3)
    m = YoloV5(2, d, w)
    m.load_state_dict(sd, strict=False)
    m.eval()
    x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        a, b = m(x), yolov5_forward(sd, x, scale)
    assert a.shape == b.shape == (2, 3 * (8 * 12 + 4 * 6 + 2 * 3), 7)
    assert (a - b).abs().max().item() < 1e-5 * max(1.0, a.abs().max().item())


def test_functional_restatement_matches_yolov5s_forward():
    from oracle.yolo_ref import yolov5s_forward
    sd = init_yolov5s_state_dict(2, seed=5)
    x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(6))
    assert torch.allclose(yolov5_forward(sd, x, "s"), yolov5s_forward(sd, x), rtol=0, atol=1e-5)


def _handle(L, arch, nc, h=640, w=640):
    hnd = ctypes.c_void_p()
    rc = L.effocr_localizer_create(arch, nc, h, w, ctypes.byref(hnd))
    return rc, hnd


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("nc", [1, 2])
def test_cabi_handle_table_equals_the_python_table(hip_lib, scale, nc):
    L = hip_lib
    rc, h = _handle(L, f"yolov5{scale}".encode(), nc)
    assert rc == 0
    try:
        n = L.effocr_localizer_num_params(h)
        got = [(L.effocr_localizer_param_name(h, i).decode(), L.effocr_localizer_param_numel(h, i)) for i in range(n)]
        want = [(k, torch.Size(v).numel()) for k, v in yolov5_param_shapes(nc, scale).items()]
        assert sorted(got) == sorted(want)
        assert L.effocr_localizer_num_predictions(h) == 25200 and L.effocr_localizer_num_outputs(h) == nc + 5
        conv_w = sum(torch.Size(v).numel() for v in yolov5_param_shapes(nc, scale).values() if len(v) == 4)
        assert L.effocr_localizer_weights_bytes(h) >= 4 * conv_w              # at least the folded fp32 weights
    finally:
        L.effocr_localizer_destroy(h)


def test_cabi_workspace_follows_the_scale(hip_lib):
    """Workspace and weight sizes come from the built table: x needs more than s, n less."""
    L = hip_lib
    ws, wb = {}, {}
    for scale in SCALES:
        rc, h = _handle(L, f"yolov5{scale}".encode(), 2)
        assert rc == 0
        ws[scale] = L.effocr_localizer_workspace_bytes(h, 16)
        wb[scale] = L.effocr_localizer_weights_bytes(h)
        L.effocr_localizer_destroy(h)
    assert ws["n"] < ws["s"] < ws["m"] < ws["l"] < ws["x"]
    assert wb["n"] < wb["s"] < wb["m"] < wb["l"] < wb["x"]
    assert ws["x"] > 2 * ws["s"]


def test_cabi_yolov5m_create_and_unknown_arch(hip_lib):
    L = hip_lib
    rc, h = _handle(L, b"yolov5m", 2)
    assert rc == 0 and h.value
    L.effocr_localizer_destroy(h)
    for bad in (b"yolov5z", b"yolov5", b"yolov5s6", b"yolov8s"):
        rc, h = _handle(L, bad, 2)
        assert rc == -2, bad
