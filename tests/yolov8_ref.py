"""TEST INFRASTRUCTURE — two independent restatements of ultralytics YOLOv8 detection (yolov8.yaml, n / s / m / l / x), written here from the
published yaml, nn/modules and parse_model (the reference has no model code, and no ultralytics install was at hand: UNVERIFIED against
one; the parameter counts of the module tree are the five ultralytics publishes, tests/test_yolov8_host.py).

* ``YoloV8``: an ``nn.Module`` tree whose state-dict keys are the ultralytics ones (``load_state_dict(strict=True)`` apart from BN's
  ``num_batches_tracked``), channel counts from the (depth, width, max_channels) table.
* ``yolov8_forward(sd, x, scale, dtype)``: literal ``torch.nn.functional`` calls, channel counts nowhere written down (they come from the
  state dict's weights).  ``bf16=True`` emulates the engine's bf16-operand mode: weights (BN folded, as the engine folds them) and inputs of
  every activated convolution rounded to bf16, accumulation in ``dtype``; the stem and the last 1x1 convolution of each Detect branch
  keep full-precision operands.

Both emit the engine's rows [B, sum(ny * nx), 5 + nc] = (cx, cy, w, h, 1.0, class scores): ultralytics' Detect inference output
(dist2bbox(xywh) * stride, sigmoid) transposed, with the constant objectness column the YOLOv5 NMS expects.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

SCALES = {"n": (0.33, 0.25, 1024), "s": (0.33, 0.50, 1024), "m": (0.67, 0.75, 768), "l": (1.00, 1.00, 512), "x": (1.00, 1.25, 512)}
STRIDES = (8.0, 16.0, 32.0)
REG_MAX = 16


def decode(box, cls, stride):
    """box [B,64,ny,nx] logits, cls [B,nc,ny,nx] logits -> rows [B, ny*nx, 5+nc] (Detect inference + DFL + dist2bbox, xywh)."""
    B, _, ny, nx = box.shape
    p = box.view(B, 4, REG_MAX, ny * nx).softmax(2)
    d = (p * torch.arange(REG_MAX, dtype=box.dtype).view(1, 1, REG_MAX, 1)).sum(2)          # [B,4,A]  left, top, right, bottom
    yv, xv = torch.meshgrid(torch.arange(ny, dtype=box.dtype) + 0.5, torch.arange(nx, dtype=box.dtype) + 0.5, indexing="ij")
    ax, ay = xv.reshape(-1), yv.reshape(-1)
    x1, y1, x2, y2 = ax - d[:, 0], ay - d[:, 1], ax + d[:, 2], ay + d[:, 3]
    xywh = torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), 2) * stride        # [B,A,4]
    return torch.cat((xywh, torch.ones(B, ny * nx, 1, dtype=box.dtype), cls.view(B, -1, ny * nx).transpose(1, 2).sigmoid()), 2)


# ---------------------------------------------------------------- module tree
class Conv(nn.Module):
    def __init__(self, c1, c2, k=1, s=1):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, k // 2, bias=False)
        self.bn = nn.BatchNorm2d(c2, eps=1e-3, momentum=0.03)
        self.act = nn.SiLU()

    def forward(self, x):
        return self.act(self.bn(self.conv(x)))


class Bottleneck(nn.Module):
    def __init__(self, c1, c2, shortcut):
        super().__init__()
        self.cv1 = Conv(c1, c2, 3, 1)
        self.cv2 = Conv(c2, c2, 3, 1)
        self.add = shortcut and c1 == c2

    def forward(self, x):
        return x + self.cv2(self.cv1(x)) if self.add else self.cv2(self.cv1(x))


class C2f(nn.Module):
    def __init__(self, c1, c2, n, shortcut):
        super().__init__()
        self.c = c2 // 2
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(Bottleneck(self.c, self.c, shortcut) for _ in range(n))

    def forward(self, x):
        y = list(self.cv1(x).chunk(2, 1))
        y.extend(m(y[-1]) for m in self.m)
        return self.cv2(torch.cat(y, 1))


class SPPF(nn.Module):
    def __init__(self, c1, c2, k=5):
        super().__init__()
        self.cv1 = Conv(c1, c1 // 2, 1, 1)
        self.cv2 = Conv(c1 // 2 * 4, c2, 1, 1)
        self.m = nn.MaxPool2d(k, 1, k // 2)

    def forward(self, x):
        y = [self.cv1(x)]
        y.extend(self.m(y[-1]) for _ in range(3))
        return self.cv2(torch.cat(y, 1))


class DFL(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(REG_MAX, 1, 1, bias=False).requires_grad_(False)
        self.conv.weight.data[:] = torch.arange(REG_MAX, dtype=torch.float).view(1, REG_MAX, 1, 1)


class Detect(nn.Module):
    def __init__(self, nc, ch):
        super().__init__()
        c2, c3 = max(16, ch[0] // 4, REG_MAX * 4), max(ch[0], min(nc, 100))
        self.cv2 = nn.ModuleList(nn.Sequential(Conv(x, c2, 3), Conv(c2, c2, 3), nn.Conv2d(c2, 4 * REG_MAX, 1)) for x in ch)
        self.cv3 = nn.ModuleList(nn.Sequential(Conv(x, c3, 3), Conv(c3, c3, 3), nn.Conv2d(c3, nc, 1)) for x in ch)
        self.dfl = DFL()

    def forward(self, feats):
        return torch.cat([decode(self.cv2[l](f), self.cv3[l](f), STRIDES[l]) for l, f in enumerate(feats)], 1)


class YoloV8(nn.Module):
    """parse_model over the yolov8.yaml rows; ``self.model[i]`` is row i (Upsample / Concat rows hold nn.Identity: no parameters)."""

    def __init__(self, nc, scale):
        super().__init__()
        depth, width, maxc = SCALES[scale]
        ch = lambda c: math.ceil(min(c, maxc) * width / 8) * 8          # noqa: E731
        rp = lambda n: max(round(n * depth), 1) if n > 1 else n         # noqa: E731
        c64, c128, c256, c512, c1024 = ch(64), ch(128), ch(256), ch(512), ch(1024)
        I = nn.Identity
        self.model = nn.ModuleList([
            Conv(3, c64, 3, 2), Conv(c64, c128, 3, 2), C2f(c128, c128, rp(3), True), Conv(c128, c256, 3, 2), C2f(c256, c256, rp(6), True),
            Conv(c256, c512, 3, 2), C2f(c512, c512, rp(6), True), Conv(c512, c1024, 3, 2), C2f(c1024, c1024, rp(3), True), SPPF(c1024, c1024),
            I(), I(), C2f(c1024 + c512, c512, rp(3), False), I(), I(), C2f(c512 + c256, c256, rp(3), False),
            Conv(c256, c256, 3, 2), I(), C2f(c256 + c512, c512, rp(3), False), Conv(c512, c512, 3, 2), I(), C2f(c512 + c1024, c1024, rp(3), False),
            Detect(nc, (c256, c512, c1024))])

    def forward(self, x):
        m = self.model
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")  # noqa: E731
        x4 = m[4](m[3](m[2](m[1](m[0](x)))))
        x6 = m[6](m[5](x4))
        x9 = m[9](m[8](m[7](x6)))
        x12 = m[12](torch.cat((up(x9), x6), 1))
        x15 = m[15](torch.cat((up(x12), x4), 1))
        x18 = m[18](torch.cat((m[16](x15), x12), 1))
        x21 = m[21](torch.cat((m[19](x18), x9), 1))
        return m[22]((x15, x18, x21))


# ---------------------------------------------------------------- functional restatement
def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _conv(sd, name, x, k, s, bf16=False):
    """ultralytics Conv: Conv2d(bias=False, padding=k//2) + BatchNorm2d(eps=1e-3) + SiLU.  bf16: BN folded into the weights in float64 and
    rounded to fp32 (what the engine stores), then weights and input rounded to bf16; the folded shift stays full precision."""
    w, g, b = sd[name + ".conv.weight"], sd[name + ".bn.weight"], sd[name + ".bn.bias"]
    mu, var = sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"]
    if not bf16:
        return F.silu(F.batch_norm(F.conv2d(x, w, None, stride=s, padding=k // 2), mu, var, g, b, training=False, eps=1e-3))
    sc = g.double() / torch.sqrt(var.double() + 1e-3)
    wf = (w.double() * sc.view(-1, 1, 1, 1)).float()
    bf = (b.double() - mu.double() * sc).float()
    return F.silu(F.conv2d(_bf16(x), _bf16(wf).to(x.dtype), bf.to(x.dtype), stride=s, padding=k // 2))


def _c2f(sd, name, x, n, shortcut, bf16):
    y = list(_conv(sd, name + ".cv1", x, 1, 1, bf16).chunk(2, 1))
    for i in range(n):
        t = _conv(sd, f"{name}.m.{i}.cv2", _conv(sd, f"{name}.m.{i}.cv1", y[-1], 3, 1, bf16), 3, 1, bf16)
        y.append(y[-1] + t if shortcut else t)
    return _conv(sd, name + ".cv2", torch.cat(y, 1), 1, 1, bf16)


def _sppf(sd, name, x, bf16):
    x = _conv(sd, name + ".cv1", x, 1, 1, bf16)
    y1 = F.max_pool2d(x, 5, 1, 2)
    y2 = F.max_pool2d(y1, 5, 1, 2)
    return _conv(sd, name + ".cv2", torch.cat((x, y1, y2, F.max_pool2d(y2, 5, 1, 2)), 1), 1, 1, bf16)


def _up(x):
    return F.interpolate(x, scale_factor=2, mode="nearest")


def yolov8_forward(sd, x, scale, dtype=torch.float64, bf16=False):
    """x [B,3,H,W] (letterboxed, 0..1) -> [B, sum(ny*nx), 5+nc] in ``dtype``."""
    d = SCALES[scale][0]
    r = lambda n: max(round(n * d), 1)                       # noqa: E731  (parse_model's repeat count, n > 1 rows only)
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x = x.to(dtype)
    q = bf16
    x0 = _conv(sd, "model.0", x, 3, 2, False)               # the stem keeps its operands in both modes
    x1 = _conv(sd, "model.1", x0, 3, 2, q)
    x2 = _c2f(sd, "model.2", x1, r(3), True, q)
    x3 = _conv(sd, "model.3", x2, 3, 2, q)
    x4 = _c2f(sd, "model.4", x3, r(6), True, q)
    x5 = _conv(sd, "model.5", x4, 3, 2, q)
    x6 = _c2f(sd, "model.6", x5, r(6), True, q)
    x7 = _conv(sd, "model.7", x6, 3, 2, q)
    x8 = _c2f(sd, "model.8", x7, r(3), True, q)
    x9 = _sppf(sd, "model.9", x8, q)
    x12 = _c2f(sd, "model.12", torch.cat((_up(x9), x6), 1), r(3), False, q)
    x15 = _c2f(sd, "model.15", torch.cat((_up(x12), x4), 1), r(3), False, q)
    x18 = _c2f(sd, "model.18", torch.cat((_conv(sd, "model.16", x15, 3, 2, q), x12), 1), r(3), False, q)
    x21 = _c2f(sd, "model.21", torch.cat((_conv(sd, "model.19", x18, 3, 2, q), x9), 1), r(3), False, q)
    z = []
    for l, f in enumerate((x15, x18, x21)):
        br = []
        for b in ("cv2", "cv3"):
            p = f"model.22.{b}.{l}"
            t = _conv(sd, p + ".1", _conv(sd, p + ".0", f, 3, 1, q), 3, 1, q)
            br.append(F.conv2d(t, sd[p + ".2.weight"], sd[p + ".2.bias"]))
        box, cls = br
        B, _, ny, nx = box.shape
        rows = []
        for j in range(4):                                   # side j: softmax over its 16 bins, expectation with the DFL weights
            pj = F.softmax(box[:, 16 * j:16 * j + 16].reshape(B, 16, ny * nx), 1)
            rows.append((pj * sd["model.22.dfl.conv.weight"].view(1, 16, 1)).sum(1))
        gy, gx = torch.meshgrid(torch.arange(ny, dtype=dtype), torch.arange(nx, dtype=dtype), indexing="ij")
        ax, ay = gx.reshape(1, -1) + 0.5, gy.reshape(1, -1) + 0.5
        x1_, y1_, x2_, y2_ = ax - rows[0], ay - rows[1], ax + rows[2], ay + rows[3]
        out = torch.stack(((x1_ + x2_) / 2 * STRIDES[l], (y1_ + y2_) / 2 * STRIDES[l], (x2_ - x1_) * STRIDES[l], (y2_ - y1_) * STRIDES[l],
                           torch.ones_like(x1_)), 2)
        z.append(torch.cat((out, cls.reshape(B, -1, ny * nx).permute(0, 2, 1).sigmoid()), 2))
    return torch.cat(z, 1)
