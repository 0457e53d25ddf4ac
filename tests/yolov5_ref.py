"""TEST INFRASTRUCTURE — functional restatement of ultralytics YOLOv5 v6 at every scale (n / s / m / l / x).

oracle/yolo_ref.py restates yolov5s alone as literal ``torch.nn.functional`` calls; oracle/yolo_modules.py builds the module
tree of any scale from the yaml rows.  This file is the functional form for all five scales: the same layer sequence as
yolov5s_forward, with channel counts nowhere written down (they come from the state dict's weights) and the C3 repeat counts
max(round(n * depth), 1) of the published depth multiples.  tests/test_yolov5_scales_host.py checks it against both.
"""
import torch
import torch.nn.functional as F

DEPTHS = {"n": 0.33, "s": 0.33, "m": 0.67, "l": 1.00, "x": 1.33}
STRIDES = (8.0, 16.0, 32.0)


def _conv(sd, name, x, k, s):
    """ultralytics Conv: Conv2d(bias=False, padding=k//2; the 6x6 stem: 2) + BatchNorm2d(eps=1e-3) + SiLU."""
    x = F.conv2d(x, sd[name + ".conv.weight"], None, stride=s, padding=2 if k == 6 else k // 2)
    x = F.batch_norm(x, sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"], sd[name + ".bn.weight"], sd[name + ".bn.bias"],
                     training=False, eps=1e-3)
    return F.silu(x)


def _c3(sd, name, x, n, shortcut):
    a = _conv(sd, name + ".cv1", x, 1, 1)
    for i in range(n):
        y = _conv(sd, f"{name}.m.{i}.cv2", _conv(sd, f"{name}.m.{i}.cv1", a, 1, 1), 3, 1)
        a = a + y if shortcut else y
    return _conv(sd, name + ".cv3", torch.cat((a, _conv(sd, name + ".cv2", x, 1, 1)), 1), 1, 1)


def _sppf(sd, name, x):
    x = _conv(sd, name + ".cv1", x, 1, 1)
    y1 = F.max_pool2d(x, 5, 1, 2)
    y2 = F.max_pool2d(y1, 5, 1, 2)
    return _conv(sd, name + ".cv2", torch.cat((x, y1, y2, F.max_pool2d(y2, 5, 1, 2)), 1), 1, 1)


def _up(x):
    return F.interpolate(x, scale_factor=2, mode="nearest")


def yolov5_forward(sd, x, scale):
    """x [B,3,H,W] (letterboxed, 0..1) -> [B, sum(3*ny*nx), 5+nc]: output 0 of the exported YOLOv5<scale>."""
    d = DEPTHS[scale]
    r = lambda n: max(round(n * d), 1)                       # noqa: E731  (parse_model's repeat count, n > 1 rows only)
    sd = {k: v.float() for k, v in sd.items()}
    x = x.float()
    x0 = _conv(sd, "model.0", x, 6, 2)
    x1 = _conv(sd, "model.1", x0, 3, 2)
    x2 = _c3(sd, "model.2", x1, r(3), True)
    x3 = _conv(sd, "model.3", x2, 3, 2)
    x4 = _c3(sd, "model.4", x3, r(6), True)
    x5 = _conv(sd, "model.5", x4, 3, 2)
    x6 = _c3(sd, "model.6", x5, r(9), True)
    x7 = _conv(sd, "model.7", x6, 3, 2)
    x8 = _c3(sd, "model.8", x7, r(3), True)
    x9 = _sppf(sd, "model.9", x8)
    x10 = _conv(sd, "model.10", x9, 1, 1)
    x13 = _c3(sd, "model.13", torch.cat((_up(x10), x6), 1), r(3), False)
    x14 = _conv(sd, "model.14", x13, 1, 1)
    x17 = _c3(sd, "model.17", torch.cat((_up(x14), x4), 1), r(3), False)
    x20 = _c3(sd, "model.20", torch.cat((_conv(sd, "model.18", x17, 3, 2), x14), 1), r(3), False)
    x23 = _c3(sd, "model.23", torch.cat((_conv(sd, "model.21", x20, 3, 2), x10), 1), r(3), False)
    anchors = sd["model.24.anchors"]                         # [3,3,2] in stride units
    z = []
    for l, f in enumerate((x17, x20, x23)):
        y = F.conv2d(f, sd[f"model.24.m.{l}.weight"], sd[f"model.24.m.{l}.bias"])
        bs, _, ny, nx = y.shape
        no = y.shape[1] // 3
        y = y.view(bs, 3, no, ny, nx).permute(0, 1, 3, 4, 2).contiguous().sigmoid()
        yv, xv = torch.meshgrid(torch.arange(ny, dtype=torch.float32), torch.arange(nx, dtype=torch.float32), indexing="ij")
        grid = torch.stack((xv, yv), 2).expand(1, 3, ny, nx, 2) - 0.5
        anchor_grid = (anchors[l] * STRIDES[l]).view(1, 3, 1, 1, 2).expand(1, 3, ny, nx, 2)
        xy = (y[..., 0:2] * 2 + grid) * STRIDES[l]
        wh = (y[..., 2:4] * 2) ** 2 * anchor_grid
        z.append(torch.cat((xy, wh, y[..., 4:]), 4).view(bs, 3 * ny * nx, no))
    return torch.cat(z, 1)
