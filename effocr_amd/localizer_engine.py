"""``EffLocalizer`` — drop-in for onnx_engines/localizer_engine.py:14-66 (``model_backend='yolo'``) on MI355X.

The reference wraps an ONNXRuntime session over an exported ultralytics YOLOv5 model: ``run(imgs)`` letterboxes each
image to ``input_shape`` (:75-85,107-138), runs the network, and ``_postprocess`` (:54-60) applies
``non_max_suppression(pred, conf_thres, iou_thres, max_det=1000)[0]`` to every image, returning a list of ``[n,6]``
tensors ``(x1, y1, x2, y2, conf, cls)`` in letterboxed-input pixels.  The driver reads ``result[:, :4]`` and ``result[:, -1]``
(infer_effocr_onnx_multi.py:252-256: class 0 = characters, class 1 = words).

Here ``model_path`` is a torch state dict (``.pt`` / ``.pth`` / ``.safetensors``, or a dict) with the ultralytics YOLOv5 keys
(``model.0.conv.weight`` ... ``model.24.m.2.bias``, ``model.24.anchors``) of any v6 scale — n, s, m, l or x, read from the
checkpoint by ``yolov5_scale`` — instead of an ``.onnx`` graph; everything from the
uint8 image to the kept boxes runs on the device (letterbox kernel -> fp32-MFMA convolutions -> decode -> NMS kernels):
one uint8 upload and one tiny ``[n,6]`` download per image.  Only the ``yolo`` backend exists (the detectron2 / mmdetection
branches of the reference return raw session outputs and are out of scope).
"""
import ctypes
import math
import threading

import numpy as np
import torch

from . import _lib

MAX_WH = 7680.0          # localizer_engine.py:205
MAX_NMS = 30000          # :206
YOLOV5_ANCHORS = ((10, 13, 16, 30, 33, 23), (30, 61, 62, 45, 59, 119), (116, 90, 156, 198, 373, 326))   # pixels, P3 / P4 / P5
STRIDES = (8.0, 16.0, 32.0)


def letterbox_geometry(shape, new_shape=(640, 640), auto=False, scaleFill=False, scaleup=True, stride=32):
    """The arithmetic of ``EffLocalizer.letterbox`` (localizer_engine.py:107-138) without the pixels:
    (h, w) -> (new_h, new_w, top, bottom, left, right, ratio, (dw, dh))."""
    if isinstance(new_shape, int):
        new_shape = (new_shape, new_shape)
    r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
    if not scaleup:
        r = min(r, 1.0)
    ratio = r, r
    new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
    dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
    if auto:
        dw, dh = np.mod(dw, stride), np.mod(dh, stride)
    elif scaleFill:
        dw, dh = 0.0, 0.0
        new_unpad = (new_shape[1], new_shape[0])
        ratio = new_shape[1] / shape[1], new_shape[0] / shape[0]
    dw /= 2
    dh /= 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return new_unpad[1], new_unpad[0], top, bottom, left, right, ratio, (dw, dh)


# ultralytics YOLOv5 v6 scales: models/yolov5{n,s,m,l,x}.yaml are one layer table at these (depth_multiple, width_multiple)
YOLOV5_SCALES = {"n": (0.33, 0.25), "s": (0.33, 0.50), "m": (0.67, 0.75), "l": (1.00, 1.00), "x": (1.33, 1.25)}


def _yolov5_dims(scale):
    """(channels(c), repeats(n)) of parse_model at ``scale``: make_divisible(c * width, 8) and max(round(n * depth), 1)."""
    if scale not in YOLOV5_SCALES:
        raise ValueError(f"unknown YOLOv5 scale {scale!r} (one of {', '.join(YOLOV5_SCALES)})")
    depth, width = YOLOV5_SCALES[scale]
    return (lambda c: math.ceil(c * width / 8) * 8), (lambda n: max(round(n * depth), 1) if n > 1 else n)


def yolov5_param_shapes(nc, scale="s"):
    """{ultralytics key: shape} of YOLOv5<scale> (v6 yaml, ``scale`` in "nsmlx") with ``nc`` classes, in module order."""
    ch, rep = _yolov5_dims(scale)
    shapes = {}

    def conv(name, c1, c2, k):
        shapes[name + ".conv.weight"] = (c2, c1, k, k)
        for s in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{name}.bn.{s}"] = (c2,)

    def c3(name, c1, c2, n):
        c_ = c2 // 2
        conv(name + ".cv1", c1, c_, 1)
        conv(name + ".cv2", c1, c_, 1)
        conv(name + ".cv3", 2 * c_, c2, 1)
        for i in range(rep(n)):
            conv(f"{name}.m.{i}.cv1", c_, c_, 1)
            conv(f"{name}.m.{i}.cv2", c_, c_, 3)

    c64, c128, c256, c512, c1024 = ch(64), ch(128), ch(256), ch(512), ch(1024)
    conv("model.0", 3, c64, 6)
    conv("model.1", c64, c128, 3)
    c3("model.2", c128, c128, 3)
    conv("model.3", c128, c256, 3)
    c3("model.4", c256, c256, 6)
    conv("model.5", c256, c512, 3)
    c3("model.6", c512, c512, 9)
    conv("model.7", c512, c1024, 3)
    c3("model.8", c1024, c1024, 3)
    conv("model.9.cv1", c1024, c1024 // 2, 1)
    conv("model.9.cv2", c1024 // 2 * 4, c1024, 1)
    conv("model.10", c1024, c512, 1)
    c3("model.13", 2 * c512, c512, 3)
    conv("model.14", c512, c256, 1)
    c3("model.17", 2 * c256, c256, 3)
    conv("model.18", c256, c256, 3)
    c3("model.20", 2 * c256, c512, 3)
    conv("model.21", c512, c512, 3)
    c3("model.23", 2 * c512, c1024, 3)
    for l, c in enumerate((c256, c512, c1024)):
        shapes[f"model.24.m.{l}.weight"] = (3 * (nc + 5), c, 1, 1)
        shapes[f"model.24.m.{l}.bias"] = (3 * (nc + 5),)
    shapes["model.24.anchors"] = (3, 3, 2)
    return shapes


def yolov5s_param_shapes(nc):
    """{ultralytics key: shape} of YOLOv5s (v6 yaml, width 0.5 / depth 0.33) with ``nc`` classes."""
    return yolov5_param_shapes(nc, "s")


def init_yolov5_state_dict(nc=2, scale="s", seed=0):
    """Seeded random YOLOv5<scale> weights (there is no network to fetch a trained localizer): kaiming-uniform convolutions,
    BatchNorm with non-trivial statistics, ultralytics' Detect bias initialisation, the default COCO anchors."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in yolov5_param_shapes(nc, scale).items():
        if k.endswith("conv.weight") or (k.startswith("model.24.m.") and k.endswith(".weight")):
            fan_in = shp[1] * shp[2] * shp[3]
            bound = math.sqrt(3.0 / fan_in) * 1.2
            sd[k] = (torch.rand(shp, generator=g) * 2 - 1) * bound
        elif k.endswith("bn.weight"):
            sd[k] = 1.0 + 0.2 * torch.randn(shp, generator=g)
        elif k.endswith("bn.bias") or k.endswith("running_mean"):
            sd[k] = 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shp, generator=g)
        elif k.endswith(".bias"):                              # Detect._initialize_biases: obj ~ 8 objects / 640 image, cls ~ 0.6 / nc
            l = int(k.split(".")[3])
            b = 0.05 * torch.randn(3, nc + 5, generator=g)
            b[:, 4] += math.log(8 / (640 / STRIDES[l]) ** 2)
            b[:, 5:] += math.log(0.6 / (nc - 0.99999))
            sd[k] = b.reshape(-1)
        elif k == "model.24.anchors":
            sd[k] = torch.tensor(YOLOV5_ANCHORS, dtype=torch.float32).view(3, 3, 2) / torch.tensor(STRIDES).view(3, 1, 1)
    return sd


def init_yolov5s_state_dict(nc=2, seed=0):
    """Seeded random YOLOv5s weights (``init_yolov5_state_dict(nc, "s", seed)``)."""
    return init_yolov5_state_dict(nc, "s", seed)


def _shape_mismatches(state_dict, want):
    bad = [f"missing {k}" for k in want if k not in state_dict] + \
          [f"{k}: shape {tuple(state_dict[k].shape)} != {tuple(want[k])}" for k in want if k in state_dict and tuple(state_dict[k].shape) != tuple(want[k])]
    return bad


def yolov5_scale(state_dict):
    """The v6 scale ("n" | "s" | "m" | "l" | "x") of an ultralytics YOLOv5 detection state dict: width from the stem's output channels
    (``model.0.conv.weight``), depth from the number of bottlenecks in ``model.2.m``; every other key and shape must then match that
    scale's table.  ValueError names the mismatch."""
    key = "model.24.m.0.bias"
    if key not in state_dict:
        raise ValueError(f"state dict has no '{key}': not an ultralytics YOLOv5 detection model")
    if "model.0.conv.weight" not in state_dict:
        raise ValueError("state dict has no 'model.0.conv.weight': not an ultralytics YOLOv5 detection model")
    nc = int(state_dict[key].numel()) // 3 - 5
    c0 = int(state_dict["model.0.conv.weight"].shape[0])
    nm = len({k.split(".")[3] for k in state_dict if k.startswith("model.2.m.")})
    by_width = [s for s in YOLOV5_SCALES if _yolov5_dims(s)[0](64) == c0]
    if not by_width:
        raise ValueError(f"model.0.conv.weight has {c0} output channels: no YOLOv5 v6 scale has that width "
                         f"({', '.join(f'{s}: {_yolov5_dims(s)[0](64)}' for s in YOLOV5_SCALES)})")
    by_depth = [s for s in by_width if _yolov5_dims(s)[1](3) == nm]
    if not by_depth:
        raise ValueError(f"model.2.m has {nm} bottlenecks, but a stem of {c0} channels is YOLOv5{by_width[0]} with "
                         f"{_yolov5_dims(by_width[0])[1](3)}")
    scale = by_depth[0]
    bad = _shape_mismatches(state_dict, yolov5_param_shapes(nc, scale))
    if bad:
        raise ValueError(f"state dict does not match yolov5{scale}: " + "; ".join(bad[:6]) + (f" (+{len(bad) - 6} more)" if len(bad) > 6 else ""))
    return scale


# ultralytics YOLOv8 scales (yolov8.yaml `scales`): (depth_multiple, width_multiple, max_channels).  Written from the published yaml,
# nn/modules and parse_model without an ultralytics install at hand: UNVERIFIED against a real checkpoint (DESIGN.md section 3 "YOLOv8");
# the tables give the five published parameter counts (tests/test_yolov8_host.py).
YOLOV8_SCALES = {"n": (0.33, 0.25, 1024), "s": (0.33, 0.50, 1024), "m": (0.67, 0.75, 768), "l": (1.00, 1.00, 512), "x": (1.00, 1.25, 512)}
YOLOV8_DFL_KEY = "model.22.dfl.conv.weight"
YOLOV8_REG_MAX = 16


def _yolov8_dims(scale):
    """(channels(c), repeats(n)) of parse_model at ``scale``: make_divisible(min(c, max_channels) * width, 8) and max(round(n * depth), 1)."""
    if scale not in YOLOV8_SCALES:
        raise ValueError(f"unknown YOLOv8 scale {scale!r} (one of {', '.join(YOLOV8_SCALES)})")
    depth, width, max_channels = YOLOV8_SCALES[scale]
    return (lambda c: math.ceil(min(c, max_channels) * width / 8) * 8), (lambda n: max(round(n * depth), 1) if n > 1 else n)


def yolov8_param_shapes(nc, scale="s"):
    """{ultralytics key: shape} of YOLOv8<scale> (yolov8.yaml, ``scale`` in "nsmlx") with ``nc`` classes, in module order."""
    ch, rep = _yolov8_dims(scale)
    shapes = {}

    def conv(name, c1, c2, k):
        shapes[name + ".conv.weight"] = (c2, c1, k, k)
        for s in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{name}.bn.{s}"] = (c2,)

    def c2f(name, c1, c2, n):
        c = c2 // 2
        conv(name + ".cv1", c1, 2 * c, 1)
        conv(name + ".cv2", (2 + rep(n)) * c, c2, 1)
        for i in range(rep(n)):
            conv(f"{name}.m.{i}.cv1", c, c, 3)
            conv(f"{name}.m.{i}.cv2", c, c, 3)

    c64, c128, c256, c512, c1024 = ch(64), ch(128), ch(256), ch(512), ch(1024)
    conv("model.0", 3, c64, 3)
    conv("model.1", c64, c128, 3)
    c2f("model.2", c128, c128, 3)
    conv("model.3", c128, c256, 3)
    c2f("model.4", c256, c256, 6)
    conv("model.5", c256, c512, 3)
    c2f("model.6", c512, c512, 6)
    conv("model.7", c512, c1024, 3)
    c2f("model.8", c1024, c1024, 3)
    conv("model.9.cv1", c1024, c1024 // 2, 1)
    conv("model.9.cv2", c1024 // 2 * 4, c1024, 1)
    c2f("model.12", c1024 + c512, c512, 3)
    c2f("model.15", c512 + c256, c256, 3)
    conv("model.16", c256, c256, 3)
    c2f("model.18", c256 + c512, c512, 3)
    conv("model.19", c512, c512, 3)
    c2f("model.21", c512 + c1024, c1024, 3)
    c2, c3 = max(16, c256 // 4, 4 * YOLOV8_REG_MAX), max(c256, min(nc, 100))
    for branch, cb, cout in (("cv2", c2, 4 * YOLOV8_REG_MAX), ("cv3", c3, nc)):
        for l, cin in enumerate((c256, c512, c1024)):
            conv(f"model.22.{branch}.{l}.0", cin, cb, 3)
            conv(f"model.22.{branch}.{l}.1", cb, cb, 3)
            shapes[f"model.22.{branch}.{l}.2.weight"] = (cout, cb, 1, 1)
            shapes[f"model.22.{branch}.{l}.2.bias"] = (cout,)
    shapes[YOLOV8_DFL_KEY] = (1, YOLOV8_REG_MAX, 1, 1)
    return shapes


def init_yolov8_state_dict(nc=2, scale="s", seed=0):
    """Seeded random YOLOv8<scale> weights (there is no network to fetch a trained localizer): kaiming-uniform convolutions, BatchNorm with
    non-trivial statistics, ultralytics' Detect.bias_init (box 1.0, class log(5 / nc / (640 / stride)^2)), the DFL constant 0 .. 15.  The last
    box convolution has 32 x the kaiming gain: its 16-bin distributions are then peaked at bins that vary from side to side and anchor to
    anchor (at unit gain every side is near 7.5 bins and every box the same size)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in yolov8_param_shapes(nc, scale).items():
        if k == YOLOV8_DFL_KEY:
            sd[k] = torch.arange(YOLOV8_REG_MAX, dtype=torch.float32).view(shp)
        elif k.endswith(".weight") and len(shp) == 4:
            fan_in = shp[1] * shp[2] * shp[3]
            bound = math.sqrt(3.0 / fan_in) * 1.2 * (32.0 if k.startswith("model.22.cv2.") and k.endswith(".2.weight") else 1.0)
            sd[k] = (torch.rand(shp, generator=g) * 2 - 1) * bound
        elif k.endswith("bn.weight"):
            sd[k] = 1.0 + 0.2 * torch.randn(shp, generator=g)
        elif k.endswith("bn.bias") or k.endswith("running_mean"):
            sd[k] = 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shp, generator=g)
        elif k.endswith(".bias"):                              # Detect.bias_init
            l = int(k.split(".")[3])
            b = 0.05 * torch.randn(shp, generator=g)
            sd[k] = b + (1.0 if ".cv2." in k else math.log(5 / nc / (640 / STRIDES[l]) ** 2))
    return sd


def yolov8_scale(state_dict):
    """The scale ("n" | "s" | "m" | "l" | "x") of an ultralytics YOLOv8 detection state dict: width from the stem's output channels
    (``model.0.conv.weight``), depth from the number of bottlenecks in ``model.2.m``; every other key and shape must then match that
    scale's table (which is what tells a wrong ``max_channels`` apart: m, l and x differ from a uniformly widened table only in their
    deepest layers), and the DFL tensor must be the constant 0 .. 15.  ValueError names the mismatch."""
    for key in (YOLOV8_DFL_KEY, "model.22.cv3.0.2.bias", "model.0.conv.weight"):
        if key not in state_dict:
            raise ValueError(f"state dict has no '{key}': not an ultralytics YOLOv8 detection model")
    nc = int(state_dict["model.22.cv3.0.2.bias"].numel())
    c0 = int(state_dict["model.0.conv.weight"].shape[0])
    nm = len({k.split(".")[3] for k in state_dict if k.startswith("model.2.m.")})
    by_width = [s for s in YOLOV8_SCALES if _yolov8_dims(s)[0](64) == c0]
    if not by_width:
        raise ValueError(f"model.0.conv.weight has {c0} output channels: no YOLOv8 scale has that width "
                         f"({', '.join(f'{s}: {_yolov8_dims(s)[0](64)}' for s in YOLOV8_SCALES)})")
    scale = by_width[0]
    if _yolov8_dims(scale)[1](3) != nm:
        raise ValueError(f"model.2.m has {nm} bottlenecks, but a stem of {c0} channels is YOLOv8{scale} with {_yolov8_dims(scale)[1](3)}")
    bad = _shape_mismatches(state_dict, yolov8_param_shapes(nc, scale))
    if bad:
        raise ValueError(f"state dict does not match yolov8{scale}: " + "; ".join(bad[:6]) + (f" (+{len(bad) - 6} more)" if len(bad) > 6 else ""))
    dfl = state_dict[YOLOV8_DFL_KEY].detach().to("cpu", torch.float32).reshape(-1)
    if not torch.equal(dfl, torch.arange(YOLOV8_REG_MAX, dtype=torch.float32)):
        raise ValueError(f"{YOLOV8_DFL_KEY} is not the constant 0 .. {YOLOV8_REG_MAX - 1}: the decode has that projection built in")
    return scale


# ultralytics YOLO11 scales (yolo11.yaml `scales`): (depth_multiple, width_multiple, max_channels).  Written from the published yaml,
# nn/modules and parse_model without an ultralytics install at hand: UNVERIFIED against a real checkpoint (DESIGN.md section 3 "YOLO11");
# the tables give the five published parameter counts (tests/test_yolo11_host.py).
YOLO11_SCALES = {"n": (0.50, 0.25, 1024), "s": (0.50, 0.50, 1024), "m": (0.50, 1.00, 512), "l": (1.00, 1.00, 512), "x": (1.00, 1.50, 512)}
YOLO11_DFL_KEY = "model.23.dfl.conv.weight"
# init_yolo11_state_dict: the gains of the q / k rows (per PSABlock) and of the v rows of attn.qkv over the kaiming bound.  Found by
# measurement on the test inputs (tests/test_yolo11_host.py holds the result): the q / k gains give logits whose spread about each
# query's mean is about 1; the v gain of the one-block scales makes the attention branch large against the block's input, without
# which a wrong softmax hardly reaches the predictions (the stride-32 tokens of a small input are near copies of each other)
YOLO11_QK_GAIN = {"n": (67.3,), "s": (70.2,), "m": (57.9,), "l": (64.5, 2.4), "x": (48.5, 2.3)}
YOLO11_V_GAIN = {"n": 16.0, "s": 16.0, "m": 16.0, "l": 1.0, "x": 1.0}
YOLO11_CLS_GAIN = 8.0    # ... and of the last class convolution


def _yolo11_dims(scale):
    """(channels(c), repeats of a "2" row, c3k forced) of parse_model at ``scale``."""
    if scale not in YOLO11_SCALES:
        raise ValueError(f"unknown YOLO11 scale {scale!r} (one of {', '.join(YOLO11_SCALES)})")
    depth, width, max_channels = YOLO11_SCALES[scale]
    return (lambda c: math.ceil(min(c, max_channels) * width / 8) * 8), max(round(2 * depth), 1), scale in "mlx"


def yolo11_param_shapes(nc, scale="n"):
    """{ultralytics key: shape} of YOLO11<scale> (yolo11.yaml, ``scale`` in "nsmlx") with ``nc`` classes, in module order."""
    ch, n2, force_c3k = _yolo11_dims(scale)
    shapes = {}

    def conv(name, c1, c2, k, groups=1):
        shapes[name + ".conv.weight"] = (c2, c1 // groups, k, k)
        for s in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{name}.bn.{s}"] = (c2,)

    def c3k(name, c):
        c_ = c // 2
        conv(name + ".cv1", c, c_, 1)
        conv(name + ".cv2", c, c_, 1)
        conv(name + ".cv3", 2 * c_, c, 1)
        for i in range(2):
            conv(f"{name}.m.{i}.cv1", c_, c_, 3)
            conv(f"{name}.m.{i}.cv2", c_, c_, 3)

    def c3k2(name, c1, c2, is_c3k, e=0.5):
        c = int(c2 * e)
        conv(name + ".cv1", c1, 2 * c, 1)
        conv(name + ".cv2", (2 + n2) * c, c2, 1)
        for i in range(n2):
            if is_c3k or force_c3k:
                c3k(f"{name}.m.{i}", c)
            else:
                conv(f"{name}.m.{i}.cv1", c, c // 2, 3)
                conv(f"{name}.m.{i}.cv2", c // 2, c, 3)

    def c2psa(name, c1):
        c = c1 // 2
        conv(name + ".cv1", c1, 2 * c, 1)
        conv(name + ".cv2", 2 * c, c1, 1)
        for j in range(n2):
            conv(f"{name}.m.{j}.attn.qkv", c, 2 * c, 1)
            conv(f"{name}.m.{j}.attn.proj", c, c, 1)
            conv(f"{name}.m.{j}.attn.pe", c, c, 3, groups=c)
            conv(f"{name}.m.{j}.ffn.0", c, 2 * c, 1)
            conv(f"{name}.m.{j}.ffn.1", 2 * c, c, 1)

    c64, c128, c256, c512, c1024 = ch(64), ch(128), ch(256), ch(512), ch(1024)
    conv("model.0", 3, c64, 3)
    conv("model.1", c64, c128, 3)
    c3k2("model.2", c128, c256, False, 0.25)
    conv("model.3", c256, c256, 3)
    c3k2("model.4", c256, c512, False, 0.25)
    conv("model.5", c512, c512, 3)
    c3k2("model.6", c512, c512, True)
    conv("model.7", c512, c1024, 3)
    c3k2("model.8", c1024, c1024, True)
    conv("model.9.cv1", c1024, c1024 // 2, 1)
    conv("model.9.cv2", c1024 // 2 * 4, c1024, 1)
    c2psa("model.10", c1024)
    c3k2("model.13", c1024 + c512, c512, False)
    c3k2("model.16", c512 + c512, c256, False)
    conv("model.17", c256, c256, 3)
    c3k2("model.19", c256 + c512, c512, False)
    conv("model.20", c512, c512, 3)
    c3k2("model.22", c512 + c1024, c1024, True)
    feats = (c256, c512, c1024)
    c2, c3 = max(16, c256 // 4, 4 * YOLOV8_REG_MAX), max(c256, min(nc, 100))
    for l, cin in enumerate(feats):
        conv(f"model.23.cv2.{l}.0", cin, c2, 3)
        conv(f"model.23.cv2.{l}.1", c2, c2, 3)
        shapes[f"model.23.cv2.{l}.2.weight"] = (4 * YOLOV8_REG_MAX, c2, 1, 1)
        shapes[f"model.23.cv2.{l}.2.bias"] = (4 * YOLOV8_REG_MAX,)
    for l, cin in enumerate(feats):
        conv(f"model.23.cv3.{l}.0.0", cin, cin, 3, groups=cin)
        conv(f"model.23.cv3.{l}.0.1", cin, c3, 1)
        conv(f"model.23.cv3.{l}.1.0", c3, c3, 3, groups=c3)
        conv(f"model.23.cv3.{l}.1.1", c3, c3, 1)
        shapes[f"model.23.cv3.{l}.2.weight"] = (nc, c3, 1, 1)
        shapes[f"model.23.cv3.{l}.2.bias"] = (nc,)
    shapes[YOLO11_DFL_KEY] = (1, YOLOV8_REG_MAX, 1, 1)
    return shapes


def init_yolo11_state_dict(nc=2, scale="n", seed=0):
    """Seeded random YOLO11<scale> weights: as ``init_yolov8_state_dict`` (kaiming-uniform convolutions, BatchNorm statistics drawn the
    same way, Detect.bias_init, the DFL constant, 32 x the gain on the last box convolution), with two more gains.  ``YOLO11_QK_GAIN[scale][block]`` x
    the kaiming bound on the q and k rows of every attn.qkv and ``YOLO11_V_GAIN[scale]`` x on its v rows: the attention logits
    32^-1/2 q . k then have a standard deviation of order 1 about each query's mean (tests/test_yolo11_host.py measures it), so the softmax
    is neither uniform nor one-hot, and a mistake in it moves the predictions.  ``YOLO11_CLS_GAIN`` x on the last class convolution: the
    class logits then spread around the very negative bias instead of sitting on it, where the sigmoid hides every change."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in yolo11_param_shapes(nc, scale).items():
        if k == YOLO11_DFL_KEY:
            sd[k] = torch.arange(YOLOV8_REG_MAX, dtype=torch.float32).view(shp)
        elif k.endswith(".weight") and len(shp) == 4:
            fan_in = shp[1] * shp[2] * shp[3]
            gain = 32.0 if k.startswith("model.23.cv2.") and k.endswith(".2.weight") else YOLO11_CLS_GAIN if k.startswith("model.23.cv3.") and k.endswith(".2.weight") else 1.0
            sd[k] = (torch.rand(shp, generator=g) * 2 - 1) * (math.sqrt(3.0 / fan_in) * 1.2 * gain)
            if ".attn.qkv." in k:                              # rows per head: q 32 | k 32 | v 64
                sd[k].view(-1, 128, *shp[1:])[:, :64] *= YOLO11_QK_GAIN[scale][int(k.split(".")[3])]
                sd[k].view(-1, 128, *shp[1:])[:, 64:] *= YOLO11_V_GAIN[scale]
        elif k.endswith("bn.weight"):
            sd[k] = 1.0 + 0.2 * torch.randn(shp, generator=g)
        elif k.endswith("bn.bias") or k.endswith("running_mean"):
            sd[k] = 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shp, generator=g)
        elif k.endswith(".bias"):                              # Detect.bias_init
            l = int(k.split(".")[3])
            b = 0.05 * torch.randn(shp, generator=g)
            sd[k] = b + (1.0 if ".cv2." in k else math.log(5 / nc / (640 / STRIDES[l]) ** 2))
    return sd


def yolo11_scale(state_dict):
    """The scale ("n" | "s" | "m" | "l" | "x") of an ultralytics YOLO11 detection state dict: width from the stem's output channels
    (``model.0.conv.weight``), depth from the number of blocks in ``model.2.m`` (what tells m from l), the cap from the width of
    ``model.7``; every key and shape must then match that scale's table, and the DFL tensor must be the constant 0 .. 15.  ValueError
    names the first mismatches."""
    for key in (YOLO11_DFL_KEY, "model.23.cv3.0.2.bias", "model.0.conv.weight", "model.7.conv.weight"):
        if key not in state_dict:
            raise ValueError(f"state dict has no '{key}': not an ultralytics YOLO11 detection model")
    nc = int(state_dict["model.23.cv3.0.2.bias"].numel())
    c0 = int(state_dict["model.0.conv.weight"].shape[0])
    nm = len({k.split(".")[3] for k in state_dict if k.startswith("model.2.m.")})
    by_width = [s for s in YOLO11_SCALES if _yolo11_dims(s)[0](64) == c0]
    if not by_width:
        raise ValueError(f"model.0.conv.weight has {c0} output channels: no YOLO11 scale has that width "
                         f"({', '.join(f'{s}: {_yolo11_dims(s)[0](64)}' for s in YOLO11_SCALES)})")
    by_depth = [s for s in by_width if _yolo11_dims(s)[1] == nm]
    if not by_depth:
        raise ValueError(f"model.2.m has {nm} blocks, but a stem of {c0} channels is YOLO11{'/'.join(by_width)} with "
                         f"{' / '.join(str(_yolo11_dims(s)[1]) for s in by_width)}")
    scale = by_depth[0]
    bad = _shape_mismatches(state_dict, yolo11_param_shapes(nc, scale))
    if bad:
        c7, want7 = int(state_dict["model.7.conv.weight"].shape[0]), _yolo11_dims(scale)[0](1024)
        cap = f" (model.7 is {c7} wide, yolo11{scale} caps it at {want7}: another max_channels)" if c7 != want7 else ""
        raise ValueError(f"state dict does not match yolo11{scale}{cap}: " + "; ".join(bad[:6]) + (f" (+{len(bad) - 6} more)" if len(bad) > 6 else ""))
    dfl = state_dict[YOLO11_DFL_KEY].detach().to("cpu", torch.float32).reshape(-1)
    if not torch.equal(dfl, torch.arange(YOLOV8_REG_MAX, dtype=torch.float32)):
        raise ValueError(f"{YOLO11_DFL_KEY} is not the constant 0 .. {YOLOV8_REG_MAX - 1}: the decode has that projection built in")
    return scale


def _load_state_dict(model_path):
    if isinstance(model_path, dict):
        sd = model_path
    elif str(model_path).endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(str(model_path))
    else:
        sd = torch.load(str(model_path), map_location="cpu", weights_only=True)
        if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
    return {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}


class HipLocalizer:
    """Device-resident YOLOv5 (any v6 scale n / s / m / l / x): C-ABI handle + weight blob + per-stream workspaces."""

    def __init__(self, state_dict, input_shape=(640, 640), device=None, precision="fp32", arch=None, call_size_invariant=False):
        # arch (optional): "yolov5n" ... "yolov5x"; must agree with the scale the state dict has (yolov5_scale)
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"precision must be 'fp32' or 'bf16', got {precision!r}")
        self.precision = precision
        self.device = _lib.require_gpu(device)       # None / "cuda" = the current device
        self._L = _lib.lib()                         # letterbox + NMS (and, here, the network)
        self._N, self._ncheck = self._network_library()
        self.input_shape = (int(input_shape[0]), int(input_shape[1]))
        self.nc, self.scale, self.arch = self._identify(state_dict, arch)
        self.no = self.nc + 5
        self._h = ctypes.c_void_p()
        self._ncheck(self._net("create")(self.arch.encode(), self.nc, self.input_shape[0], self.input_shape[1], ctypes.byref(self._h)),
                     f"{self._PREFIX}_create")
        for i in range(self._net("num_params")(self._h)):
            name = self._net("param_name")(self._h, i).decode()
            t = state_dict[name].detach().to("cpu", torch.float32).contiguous()
            self._ncheck(self._net("set_param")(self._h, name.encode(), _lib.ptr(t), t.numel()), f"{self._PREFIX}_set_param({name})")
        nbytes = int(self._net("weights_bytes")(self._h))
        with torch.cuda.device(self.device):
            self._wblob = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._ncheck(self._net("upload")(self._h, _lib.ptr(self._wblob), nbytes), f"{self._PREFIX}_upload")
        self.set_option("bf16_operands", 1 if precision == "bf16" else 0)
        # call_size_invariant=True: an image's predictions are bitwise the same in every batch size and position (no convolution
        # splits K; DESIGN.md "Call-size-invariant mode")
        self._call_size_invariant = False
        if call_size_invariant:
            self.set_option("call_size_invariant", 1)
        self.num_predictions = int(self._net("num_predictions")(self._h))
        self._ws = {}
        self._lock = threading.Lock()

    _PREFIX = "effocr_localizer"                     # the network's entry points: <_PREFIX>_create ... <_PREFIX>_forward

    def _network_library(self):
        """(library that exports the network's entry points, its check(rc, what))."""
        return self._L, (lambda rc, what: _lib.check(rc, what, self._L))

    def _net(self, name):
        return getattr(self._N, f"{self._PREFIX}_{name}")

    @staticmethod
    def _identify(state_dict, arch):
        """(nc, scale, arch) of the checkpoint; ``arch`` (optional) must agree."""
        key = "model.24.m.0.bias"
        if key not in state_dict:
            raise ValueError(f"state dict has no '{key}': not an ultralytics YOLOv5 detection model")
        nc = int(state_dict[key].numel()) // 3 - 5
        scale = yolov5_scale(state_dict)
        if arch is not None and arch != "yolov5" + scale:
            raise ValueError(f"arch={arch!r}, but the state dict is yolov5{scale}")
        return nc, scale, "yolov5" + scale

    def set_option(self, name, value):
        self._ncheck(self._net("set_option")(self._h, name.encode(), int(value)), f"{self._PREFIX}_set_option")
        if name == "call_size_invariant":
            self._call_size_invariant = bool(value)

    @property
    def call_size_invariant(self):
        return self._call_size_invariant

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                self._net("destroy")(self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass

    def _workspace(self, tag, need):
        key = (tag, torch.cuda.current_stream(self.device).cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        return ws

    def forward(self, x):
        """x: [B,3,H,W] float32 CUDA tensor (letterboxed, RGB, 0..1) -> [B, num_predictions, 5 + nc] (async)."""
        if x.dim() != 4 or x.shape[1] != 3 or tuple(x.shape[2:]) != self.input_shape:
            raise ValueError(f"expected input [B,3,{self.input_shape[0]},{self.input_shape[1]}], got {tuple(x.shape)}")
        if x.dtype != torch.float32 or x.device != self.device:
            raise ValueError(f"expected a float32 tensor on {self.device}, got {x.dtype} on {x.device}")
        x = x.contiguous()
        B = x.shape[0]
        pred = torch.empty((B, self.num_predictions, self.no), dtype=torch.float32, device=self.device)
        if B == 0:
            return pred
        need = int(self._net("workspace_bytes")(self._h, B))
        with self._lock, torch.cuda.device(self.device):
            ws = self._workspace("fwd", need)
            self._ncheck(self._net("forward")(self._h, _lib.ptr(x), B, _lib.ptr(pred), _lib.ptr(ws), ws.numel(), _lib.current_stream(self.device)),
                         f"{self._PREFIX}_forward")
        return pred

    def letterbox(self, image, bgr=False, out=None):
        """HWC uint8 image (numpy / tensor; ``bgr=True`` for cv2.imread order) -> [1,3,H,W] float32 on the device
        (load_localizer_img, localizer_engine.py:75-85).  ``out``: an existing [1,3,H,W] slice of a batch tensor to fill."""
        t = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
        if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8:
            raise ValueError("image must be HWC uint8 with 3 channels")
        t = t.to(self.device).contiguous()
        H, W = int(t.shape[0]), int(t.shape[1])
        nh, nw, top, _, left, _, _, _ = letterbox_geometry((H, W), self.input_shape, auto=False, stride=32)
        if out is None:
            out = torch.empty((1, 3) + self.input_shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (1, 3) + self.input_shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous float32 [1,3,H,W] tensor on the localizer's device")
        with torch.cuda.device(self.device):
            _lib.check(self._L.effocr_letterbox(_lib.ptr(t), H, W, 3 * W, 1 if bgr else 0, self.input_shape[0], self.input_shape[1], nh, nw, top, left,
                                                _lib.ptr(out), _lib.current_stream(self.device)), "effocr_letterbox", self._L)
        return out

    def nms_async(self, pred, conf_thres, iou_thres, max_det=1000, agnostic=False, out=None, cnt=None):
        """pred [n, 5 + nc] (one image) -> (rows [max_det,6], count [1] int32), both on the device, no synchronisation.
        ``out`` / ``cnt``: rows of a caller's batch result to fill instead of fresh tensors (cnt must be zeroed by the caller)."""
        if not (0 <= conf_thres <= 1):
            raise AssertionError(f"Invalid Confidence threshold {conf_thres}, valid values are between 0.0 and 1.0")
        if not (0 <= iou_thres <= 1):
            raise AssertionError(f"Invalid IoU {iou_thres}, valid values are between 0.0 and 1.0")
        pred = pred.to(self.device, torch.float32).contiguous()
        n = int(pred.shape[0])
        if out is None:
            out = torch.empty((max_det, 6), dtype=torch.float32, device=self.device)
        if cnt is None:
            cnt = torch.zeros(1, dtype=torch.int32, device=self.device)
        need = int(self._L.effocr_nms_workspace_bytes(n, MAX_NMS))
        with self._lock, torch.cuda.device(self.device):
            # ONE scratch per stream, reused by every image: the launches of successive images are ordered on the stream, so the
            # candidate lists of image i are dead when image i+1's kernels start (up to ~80 MB at 25 200 candidates: not per image)
            ws = self._workspace("nms", need)
            _lib.check(self._L.effocr_nms(_lib.ptr(pred), n, self.nc, float(conf_thres), float(iou_thres), int(max_det), MAX_NMS, MAX_WH,
                                          1 if agnostic else 0, _lib.ptr(out), _lib.ptr(cnt), _lib.ptr(ws), ws.numel(),
                                          _lib.current_stream(self.device)), "effocr_nms", self._L)
        return out, cnt

    def nms_batch_async(self, pred, conf_thres, iou_thres, max_det=1000, agnostic=False, out=None, cnt=None):
        """pred [B, n, 5 + nc] (the images of one network call) -> (rows [B, max_det, 6], counts [B] int32) on the device, no
        synchronisation: effocr_nms_batch — one launch for all images when n <= 25600 (any max_det; no workspace), else the
        per-image kernels back to back.  ``out`` / ``cnt``: slices of a caller's result to fill."""
        if not (0 <= conf_thres <= 1):
            raise AssertionError(f"Invalid Confidence threshold {conf_thres}, valid values are between 0.0 and 1.0")
        if not (0 <= iou_thres <= 1):
            raise AssertionError(f"Invalid IoU {iou_thres}, valid values are between 0.0 and 1.0")
        pred = pred.to(self.device, torch.float32).contiguous()
        B, n = int(pred.shape[0]), int(pred.shape[1])
        if out is None:
            out = torch.empty((B, max_det, 6), dtype=torch.float32, device=self.device)
        if cnt is None:
            cnt = torch.zeros(B, dtype=torch.int32, device=self.device)
        assert out.is_contiguous() and cnt.is_contiguous() and out.shape == (B, max_det, 6) and cnt.shape == (B,)
        need = int(self._L.effocr_nms_batch_workspace_bytes(n, int(max_det), MAX_NMS))      # 0: the one-launch greedy path
        with self._lock, torch.cuda.device(self.device):
            ws = self._workspace("nms", max(need, 256))
            _lib.check(self._L.effocr_nms_batch(_lib.ptr(pred), B, n, self.nc, float(conf_thres), float(iou_thres), int(max_det), MAX_NMS, MAX_WH,
                                                1 if agnostic else 0, _lib.ptr(out), _lib.ptr(cnt), _lib.ptr(ws), ws.numel(),
                                                _lib.current_stream(self.device)), "effocr_nms_batch", self._L)
        return out, cnt

    def nms(self, pred, conf_thres, iou_thres, max_det=1000, agnostic=False):
        """pred [n, 5 + nc] (one image) -> [m,6] device tensor, m <= max_det (non_max_suppression(...)[0])."""
        out, cnt = self.nms_async(pred, conf_thres, iou_thres, max_det, agnostic)
        return out[: int(cnt.item())]


class HipLocalizerV8(HipLocalizer):
    """Device-resident YOLOv8 (n / s / m / l / x): the network is libeffocr_yolov8.so's (include/effocr_yolov8.h); its rows are
    (cx, cy, w, h, 1.0, class scores) — a YOLOv5 row with a constant objectness — so ``letterbox``, ``nms_async`` and ``nms_batch_async``
    are HipLocalizer's, on the product library."""

    _PREFIX = "effocr_yolov8"

    def _network_library(self):
        return _lib.yolov8_lib(), _lib.yolov8_check

    @staticmethod
    def _identify(state_dict, arch):
        scale = yolov8_scale(state_dict)
        if arch is not None and arch != "yolov8" + scale:
            raise ValueError(f"arch={arch!r}, but the state dict is yolov8{scale}")
        return int(state_dict["model.22.cv3.0.2.bias"].numel()), scale, "yolov8" + scale


class HipLocalizerV11(HipLocalizer):
    """Device-resident YOLO11 (n / s / m / l / x): the network is libeffocr_yolo11.so's (include/effocr_yolo11.h); its rows are YOLOv8's
    — (cx, cy, w, h, 1.0, class scores) — so ``letterbox``, ``nms_async`` and ``nms_batch_async`` are HipLocalizer's, on the product
    library.  An input of more than 1600 stride-32 pixels (above 1280 x 1280) is refused by the library."""

    _PREFIX = "effocr_yolo11"

    def _network_library(self):
        return _lib.yolo11_lib(), _lib.yolo11_check

    @staticmethod
    def _identify(state_dict, arch):
        scale = yolo11_scale(state_dict)
        if arch is not None and arch != "yolo11" + scale:
            raise ValueError(f"arch={arch!r}, but the state dict is yolo11{scale}")
        return int(state_dict["model.23.cv3.0.2.bias"].numel()), scale, "yolo11" + scale


class EffLocalizer:

    def __init__(self, model_path, iou_thresh=0.01, conf_thresh=0.30, vertical=False, num_cores=None, providers=None,
                 input_shape=(640, 640), model_backend='yolo', device=None, precision="fp32", arch=None, call_size_invariant=False):
        # precision (extension): "fp32" = fp32 MFMA operands (the oracle's arithmetic), "bf16" = bf16-rounded operands for every
        # convolution with an activation, fp32 accumulation and fp32 Detect heads (2-3x the network throughput)
        # arch (extension): "yolov5n" ... "yolov5x", "yolov8n" ... "yolov8x", "yolo11n" ... "yolo11x" or None; family and scale are read
        # from the state dict (a model.23.dfl.conv.weight key: YOLO11, a model.22.dfl.conv.weight key: YOLOv8) and must agree
        # num_cores / providers are ORT knobs (localizer_engine.py:17-23): accepted and ignored.
        if model_backend != 'yolo':
            raise NotImplementedError('Backend {} is not implemented'.format(model_backend))
        self.num_cores, self.providers = num_cores, providers
        self._iou_thresh, self._conf_thresh, self._vertical = iou_thresh, conf_thresh, vertical
        self._input_shape = (int(input_shape[0]), int(input_shape[1]))
        self._model_backend = model_backend
        sd = _load_state_dict(model_path)
        engine = HipLocalizerV11 if YOLO11_DFL_KEY in sd else HipLocalizerV8 if YOLOV8_DFL_KEY in sd else HipLocalizer   # the checkpoint says which network it is
        self._eng_net = engine(sd, input_shape=self._input_shape, device=device, precision=precision, arch=arch,
                               call_size_invariant=call_size_invariant)

    def __call__(self, imgs):
        return self.run(imgs)

    @property
    def call_size_invariant(self):
        return self._eng_net.call_size_invariant

    def load_localizer_img(self, input_path):
        """localizer_engine.py:75-85 with PIL instead of cv2.imread (cv2 is not installed): RGB in, so no channel swap."""
        from PIL import Image
        im0 = np.array(Image.open(input_path).convert("RGB"))
        return self._eng_net.letterbox(im0, bgr=False)

    def _letterboxed(self, imgs):
        """list entries -> one [n,3,H,W] float32 device tensor (one image per ENTRY).  A pre-letterboxed float entry may carry a
        batch: like the reference, whose ``_postprocess`` keeps ``non_max_suppression(pred)[0]`` per entry
        (localizer_engine.py:58-60), only its first image is used, so results always line up with the input list."""
        eng = self._eng_net
        x = torch.empty((len(imgs), 3) + self._input_shape, dtype=torch.float32, device=eng.device)
        for i, img in enumerate(imgs):
            if isinstance(img, str):
                from PIL import Image
                img = np.array(Image.open(img).convert("RGB"))    # load_localizer_img (:75-85), PIL instead of cv2: RGB in, no channel swap
            if (isinstance(img, np.ndarray) and img.dtype == np.uint8) or (isinstance(img, torch.Tensor) and img.dtype == torch.uint8):
                eng.letterbox(img, bgr=False, out=x[i:i + 1])
            else:
                t = torch.as_tensor(img)
                if t.dtype != torch.float32:
                    raise ValueError(f"Unexpected input data type. Actual: {t.dtype}, expected: float32")
                if t.dim() == 3:
                    t = t.unsqueeze(0)
                if t.dim() != 4 or t.shape[0] < 1 or tuple(t.shape[1:]) != (3,) + self._input_shape:
                    raise ValueError(f"expected a letterboxed [k,3,{self._input_shape[0]},{self._input_shape[1]}] array, got {tuple(t.shape)}")
                x[i].copy_(t[0], non_blocking=True)
        return x

    def run_device(self, imgs, max_det=1000):
        """``run`` without the download: -> (rows [n, max_det, 6] float32, counts [n] int32), both on the device, nothing
        synchronised — rows[i, :counts[i]] = (x1, y1, x2, y2, conf, cls) of entry i.  The letterboxed images go through the network
        in sub-batches of 16, each followed by ONE batched NMS call on the current stream."""
        eng = self._eng_net
        if not isinstance(imgs, (list, tuple)):
            imgs = [imgs]
        n = len(imgs)
        rows = torch.empty((n, max_det, 6), dtype=torch.float32, device=eng.device)
        counts = torch.zeros(n, dtype=torch.int32, device=eng.device)
        if n == 0:
            return rows, counts
        x = self._letterboxed(imgs)
        for b0 in range(0, n, 16):
            pred = eng.forward(x[b0:b0 + 16])
            eng.nms_batch_async(pred, self._conf_thresh, self._iou_thresh, max_det=max_det, out=rows[b0:b0 + 16], cnt=counts[b0:b0 + 16])
        return rows, counts

    def run(self, imgs):
        """imgs: list of image paths, of HWC uint8 arrays (RGB), or of already letterboxed float32 [1,3,H,W] arrays (what
        ``load_localizer_img`` returns in the reference) -> list (one per entry) of CPU tensors [n,6] (x1, y1, x2, y2, conf, cls).
        (The reference runs the session image by image, localizer_engine.py:52; here: batched network, ONE synchronisation.)"""
        rows, counts = self.run_device(imgs)
        if rows.shape[0] == 0:
            return []
        counts = counts.cpu().tolist()
        rows = rows[:, : max(counts + [0])].cpu()
        return [rows[i, :c].clone() for i, c in enumerate(counts)]
