"""TEST INFRASTRUCTURE — two independent restatements of ultralytics YOLO11 detection (yolo11.yaml, n / s / m / l / x), written here from the
published yaml, nn/modules and parse_model (the reference has no model code, and no ultralytics install was at hand: UNVERIFIED against
one; the parameter counts of the module tree are the five ultralytics publishes, tests/test_yolo11_host.py).

* ``Yolo11``: an ``nn.Module`` tree whose state-dict keys are the ultralytics ones (``load_state_dict(strict=True)`` apart from BN's
  ``num_batches_tracked``), channel counts from the (depth, width, max_channels) table.
* ``yolo11_forward(sd, x, scale, dtype)``: literal ``torch.nn.functional`` calls that index the state dict directly; channel counts come
  from the weights.  ``bf16=True`` emulates the engine's bf16-operand mode by the rule declared in include/effocr_yolo11.h: weights (BN
  folded, as the engine folds them) and inputs of every dense convolution rounded to bf16 — those without an activation in C2PSA
  included — accumulation in ``dtype``; the stem, the last 1x1 convolution of each Detect branch, the attention and every depthwise
  convolution keep full-precision operands.  ``mistake=`` plants one of MISTAKES (the mutation check of the host tests).
* ``attention_tiled`` / ``attention_exact`` and ``dwconv_taps``: the two kernels of yolo11.hip restated alone, for the operator tests.

Both network forms emit the engine's rows [B, sum(ny * nx), 5 + nc] = (cx, cy, w, h, 1.0, class scores), as tests/yolov8_ref.py.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.yolov8_ref import DFL, REG_MAX, SPPF, STRIDES, decode

SCALES = {"n": (0.50, 0.25, 1024), "s": (0.50, 0.50, 1024), "m": (0.50, 1.00, 512), "l": (1.00, 1.00, 512), "x": (1.00, 1.50, 512)}
MISTAKES = ("no_scale", "softmax_over_queries", "global_thirds", "pe_qkv_order", "no_pe", "head_no_shortcut", "cls_dw_no_silu")


# ---------------------------------------------------------------- module tree
class Conv(nn.Module):
    def __init__(self, c1, c2, k=1, s=1, g=1, act=True):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, k // 2, groups=g, bias=False)
        self.bn = nn.BatchNorm2d(c2, eps=1e-3, momentum=0.03)
        self.act = nn.SiLU() if act else nn.Identity()

    def forward(self, x):
        return self.act(self.bn(self.conv(x)))


class Bottleneck(nn.Module):
    def __init__(self, c1, c2, shortcut=True, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 3, 1)
        self.cv2 = Conv(c_, c2, 3, 1)
        self.add = shortcut and c1 == c2

    def forward(self, x):
        return x + self.cv2(self.cv1(x)) if self.add else self.cv2(self.cv1(x))


class C3k(nn.Module):
    def __init__(self, c1, c2, n=2):
        super().__init__()
        c_ = int(c2 * 0.5)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*(Bottleneck(c_, c_, True, e=1.0) for _ in range(n)))

    def forward(self, x):
        return self.cv3(torch.cat((self.m(self.cv1(x)), self.cv2(x)), 1))


class C3k2(nn.Module):
    def __init__(self, c1, c2, n, c3k, e=0.5):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(C3k(self.c, self.c, 2) if c3k else Bottleneck(self.c, self.c, True) for _ in range(n))

    def forward(self, x):
        y = list(self.cv1(x).chunk(2, 1))
        y.extend(m(y[-1]) for m in self.m)
        return self.cv2(torch.cat(y, 1))


class Attention(nn.Module):
    def __init__(self, dim, num_heads, attn_ratio=0.5):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.key_dim = int(self.head_dim * attn_ratio)
        self.scale = self.key_dim ** -0.5
        self.qkv = Conv(dim, dim + self.key_dim * num_heads * 2, 1, act=False)
        self.proj = Conv(dim, dim, 1, act=False)
        self.pe = Conv(dim, dim, 3, 1, g=dim, act=False)

    def forward(self, x):
        B, C, H, W = x.shape
        N = H * W
        q, k, v = self.qkv(x).view(B, self.num_heads, self.key_dim * 2 + self.head_dim, N).split([self.key_dim, self.key_dim, self.head_dim], dim=2)
        attn = ((q.transpose(-2, -1) @ k) * self.scale).softmax(dim=-1)
        x = (v @ attn.transpose(-2, -1)).view(B, C, H, W) + self.pe(v.reshape(B, C, H, W))
        return self.proj(x)


class PSABlock(nn.Module):
    def __init__(self, c, num_heads):
        super().__init__()
        self.attn = Attention(c, num_heads)
        self.ffn = nn.Sequential(Conv(c, c * 2, 1), Conv(c * 2, c, 1, act=False))

    def forward(self, x):
        x = x + self.attn(x)
        return x + self.ffn(x)


class C2PSA(nn.Module):
    def __init__(self, c1, n):
        super().__init__()
        self.c = c1 // 2
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv(2 * self.c, c1, 1)
        self.m = nn.Sequential(*(PSABlock(self.c, self.c // 64) for _ in range(n)))

    def forward(self, x):
        a, b = self.cv1(x).split((self.c, self.c), dim=1)
        return self.cv2(torch.cat((a, self.m(b)), 1))


class Detect(nn.Module):
    def __init__(self, nc, ch):
        super().__init__()
        c2, c3 = max(16, ch[0] // 4, REG_MAX * 4), max(ch[0], min(nc, 100))
        self.cv2 = nn.ModuleList(nn.Sequential(Conv(x, c2, 3), Conv(c2, c2, 3), nn.Conv2d(c2, 4 * REG_MAX, 1)) for x in ch)
        self.cv3 = nn.ModuleList(nn.Sequential(nn.Sequential(Conv(x, x, 3, g=x), Conv(x, c3, 1)), nn.Sequential(Conv(c3, c3, 3, g=c3), Conv(c3, c3, 1)),
                                               nn.Conv2d(c3, nc, 1)) for x in ch)
        self.dfl = DFL()

    def forward(self, feats):
        return torch.cat([decode(self.cv2[l](f), self.cv3[l](f), STRIDES[l]) for l, f in enumerate(feats)], 1)


class Yolo11(nn.Module):
    """parse_model over the yolo11.yaml rows; ``self.model[i]`` is row i (Upsample / Concat rows hold nn.Identity: no parameters)."""

    def __init__(self, nc, scale):
        super().__init__()
        depth, width, maxc = SCALES[scale]
        ch = lambda c: math.ceil(min(c, maxc) * width / 8) * 8          # noqa: E731
        n = max(round(2 * depth), 1)
        k = scale in "mlx"                                              # parse_model: c3k forced on for m / l / x
        c64, c128, c256, c512, c1024 = ch(64), ch(128), ch(256), ch(512), ch(1024)
        I = nn.Identity
        self.model = nn.ModuleList([
            Conv(3, c64, 3, 2), Conv(c64, c128, 3, 2), C3k2(c128, c256, n, k, 0.25), Conv(c256, c256, 3, 2), C3k2(c256, c512, n, k, 0.25),
            Conv(c512, c512, 3, 2), C3k2(c512, c512, n, True), Conv(c512, c1024, 3, 2), C3k2(c1024, c1024, n, True), SPPF(c1024, c1024),
            C2PSA(c1024, n), I(), I(), C3k2(c1024 + c512, c512, n, k), I(), I(), C3k2(c512 + c512, c256, n, k),
            Conv(c256, c256, 3, 2), I(), C3k2(c256 + c512, c512, n, k), Conv(c512, c512, 3, 2), I(), C3k2(c512 + c1024, c1024, n, True),
            Detect(nc, (c256, c512, c1024))])

    def forward(self, x):
        m = self.model
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")  # noqa: E731
        x4 = m[4](m[3](m[2](m[1](m[0](x)))))
        x6 = m[6](m[5](x4))
        x10 = m[10](m[9](m[8](m[7](x6))))
        x13 = m[13](torch.cat((up(x10), x6), 1))
        x16 = m[16](torch.cat((up(x13), x4), 1))
        x19 = m[19](torch.cat((m[17](x16), x13), 1))
        x22 = m[22](torch.cat((m[20](x19), x10), 1))
        return m[23]((x16, x19, x22))


# ---------------------------------------------------------------- functional restatement
def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _conv(sd, name, x, k, s, bf16=False, act=True, groups=1):
    """ultralytics Conv: Conv2d(bias=False, padding=k//2, groups) + BatchNorm2d(eps=1e-3) + SiLU unless act=False.  bf16: BN folded into
    the weights in float64 and rounded to fp32 (what the engine stores), then weights and input rounded to bf16; the folded shift stays
    full precision."""
    w, g, b = sd[name + ".conv.weight"], sd[name + ".bn.weight"], sd[name + ".bn.bias"]
    mu, var = sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"]
    if not bf16:
        y = F.batch_norm(F.conv2d(x, w, None, stride=s, padding=k // 2, groups=groups), mu, var, g, b, training=False, eps=1e-3)
    else:
        sc = g.double() / torch.sqrt(var.double() + 1e-3)
        wf = (w.double() * sc.view(-1, 1, 1, 1)).float()
        bf = (b.double() - mu.double() * sc).float()
        y = F.conv2d(_bf16(x), _bf16(wf).to(x.dtype), bf.to(x.dtype), stride=s, padding=k // 2, groups=groups)
    return F.silu(y) if act else y


def _bottleneck(sd, name, x, q, shortcut=True):
    t = _conv(sd, name + ".cv2", _conv(sd, name + ".cv1", x, 3, 1, q), 3, 1, q)
    return x + t if shortcut else t


def _c3k(sd, name, x, q, shortcut=True):
    t = _conv(sd, name + ".cv1", x, 1, 1, q)
    for i in range(2):
        t = _bottleneck(sd, f"{name}.m.{i}", t, q, shortcut)
    return _conv(sd, name + ".cv3", torch.cat((t, _conv(sd, name + ".cv2", x, 1, 1, q)), 1), 1, 1, q)


def _c3k2(sd, name, x, q, shortcut=True):
    y = list(_conv(sd, name + ".cv1", x, 1, 1, q).chunk(2, 1))
    i = 0
    while f"{name}.m.{i}.cv1.conv.weight" in sd:
        p = f"{name}.m.{i}"
        y.append(_c3k(sd, p, y[-1], q, shortcut) if p + ".cv3.conv.weight" in sd else _bottleneck(sd, p, y[-1], q, shortcut))
        i += 1
    return _conv(sd, name + ".cv2", torch.cat(y, 1), 1, 1, q)


def _attention(sd, name, x, q, mistake):
    """ultralytics Attention(dim, heads = dim / 64, attn_ratio 0.5): per head 32 q, 32 k and 64 v channels, IN THAT ORDER inside the
    head's 128 qkv channels."""
    B, C, H, W = x.shape
    N, heads = H * W, C // 64
    qkv = _conv(sd, name + ".qkv", x, 1, 1, q, act=False).reshape(B, 2 * C, N)
    if mistake == "global_thirds":
        qq, kk, vv = (t.reshape(B, heads, -1, N) for t in qkv.split((C // 2, C // 2, C), 1))
    else:
        t = qkv.reshape(B, heads, 128, N)
        qq, kk, vv = t[:, :, :32], t[:, :, 32:64], t[:, :, 64:]
    logits = torch.einsum("bhdn,bhdm->bhnm", qq, kk) * (1.0 if mistake == "no_scale" else 32 ** -0.5)
    attn = logits.softmax(2 if mistake == "softmax_over_queries" else 3)
    out = torch.einsum("bhnm,bhdm->bhdn", attn, vv).reshape(B, C, H, W)
    v_img = qkv[:, C:].reshape(B, C, H, W) if mistake == "pe_qkv_order" else vv.reshape(B, C, H, W)
    if mistake != "no_pe":
        out = out + _conv(sd, name + ".pe", v_img, 3, 1, False, act=False, groups=C)
    return _conv(sd, name + ".proj", out, 1, 1, q, act=False)


def _c2psa(sd, name, x, q, mistake):
    a, b = _conv(sd, name + ".cv1", x, 1, 1, q).chunk(2, 1)
    j = 0
    while f"{name}.m.{j}.attn.qkv.conv.weight" in sd:
        p = f"{name}.m.{j}"
        b = b + _attention(sd, p + ".attn", b, q, mistake)
        b = b + _conv(sd, p + ".ffn.1", _conv(sd, p + ".ffn.0", b, 1, 1, q), 1, 1, q, act=False)
        j += 1
    return _conv(sd, name + ".cv2", torch.cat((a, b), 1), 1, 1, q)


def _sppf(sd, name, x, bf16):
    x = _conv(sd, name + ".cv1", x, 1, 1, bf16)
    y1 = F.max_pool2d(x, 5, 1, 2)
    y2 = F.max_pool2d(y1, 5, 1, 2)
    return _conv(sd, name + ".cv2", torch.cat((x, y1, y2, F.max_pool2d(y2, 5, 1, 2)), 1), 1, 1, bf16)


def _up(x):
    return F.interpolate(x, scale_factor=2, mode="nearest")


def yolo11_forward(sd, x, scale=None, dtype=torch.float64, bf16=False, mistake=None):
    """x [B,3,H,W] (letterboxed, 0..1) -> [B, sum(ny*nx), 5+nc] in ``dtype``.  ``scale`` is not needed (the structure is read from the
    keys); the argument is kept for symmetry with yolov8_forward."""
    assert mistake is None or mistake in MISTAKES, mistake
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x = x.to(dtype)
    q = bf16
    hs = mistake != "head_no_shortcut"
    x0 = _conv(sd, "model.0", x, 3, 2, False)               # the stem keeps its operands in both modes
    x2 = _c3k2(sd, "model.2", _conv(sd, "model.1", x0, 3, 2, q), q)
    x4 = _c3k2(sd, "model.4", _conv(sd, "model.3", x2, 3, 2, q), q)
    x6 = _c3k2(sd, "model.6", _conv(sd, "model.5", x4, 3, 2, q), q)
    x8 = _c3k2(sd, "model.8", _conv(sd, "model.7", x6, 3, 2, q), q)
    x10 = _c2psa(sd, "model.10", _sppf(sd, "model.9", x8, q), q, mistake)
    x13 = _c3k2(sd, "model.13", torch.cat((_up(x10), x6), 1), q, hs)
    x16 = _c3k2(sd, "model.16", torch.cat((_up(x13), x4), 1), q, hs)
    x19 = _c3k2(sd, "model.19", torch.cat((_conv(sd, "model.17", x16, 3, 2, q), x13), 1), q, hs)
    x22 = _c3k2(sd, "model.22", torch.cat((_conv(sd, "model.20", x19, 3, 2, q), x10), 1), q, hs)
    z = []
    for l, f in enumerate((x16, x19, x22)):
        p = f"model.23.cv2.{l}"
        t = _conv(sd, p + ".1", _conv(sd, p + ".0", f, 3, 1, q), 3, 1, q)
        box = F.conv2d(t, sd[p + ".2.weight"], sd[p + ".2.bias"])
        p = f"model.23.cv3.{l}"
        dw_act = mistake != "cls_dw_no_silu"
        t = _conv(sd, p + ".0.1", _conv(sd, p + ".0.0", f, 3, 1, False, act=dw_act, groups=f.shape[1]), 1, 1, q)
        t = _conv(sd, p + ".1.1", _conv(sd, p + ".1.0", t, 3, 1, False, act=dw_act, groups=t.shape[1]), 1, 1, q)
        cls = F.conv2d(t, sd[p + ".2.weight"], sd[p + ".2.bias"])
        B, _, ny, nx = box.shape
        rows = []
        for j in range(4):                                   # side j: softmax over its 16 bins, expectation with the DFL weights
            pj = F.softmax(box[:, 16 * j:16 * j + 16].reshape(B, 16, ny * nx), 1)
            rows.append((pj * sd["model.23.dfl.conv.weight"].view(1, 16, 1)).sum(1))
        gy, gx = torch.meshgrid(torch.arange(ny, dtype=dtype), torch.arange(nx, dtype=dtype), indexing="ij")
        ax, ay = gx.reshape(1, -1) + 0.5, gy.reshape(1, -1) + 0.5
        x1_, y1_, x2_, y2_ = ax - rows[0], ay - rows[1], ax + rows[2], ay + rows[3]
        out = torch.stack(((x1_ + x2_) / 2 * STRIDES[l], (y1_ + y2_) / 2 * STRIDES[l], (x2_ - x1_) * STRIDES[l], (y2_ - y1_) * STRIDES[l],
                           torch.ones_like(x1_)), 2)
        z.append(torch.cat((out, cls.reshape(B, -1, ny * nx).permute(0, 2, 1).sigmoid()), 2))
    return torch.cat(z, 1)


def attention_logit_std(sd, x):
    """Standard deviation of the attention logits 32^-1/2 q . k of every PSABlock of model.10 on input x (float64), each query's logits
    taken about their mean over the keys."""
    got = []
    sd = {k: v.double() for k, v in sd.items()}
    x = x.double()
    x = _conv(sd, "model.1", _conv(sd, "model.0", x, 3, 2), 3, 2)
    for i in (2, 4, 6, 8):
        x = _c3k2(sd, f"model.{i}", x, False)
        if i < 8:
            x = _conv(sd, f"model.{i + 1}", x, 3, 2)
    a, b = _conv(sd, "model.10.cv1", _sppf(sd, "model.9", x, False), 1, 1).chunk(2, 1)
    j = 0
    while f"model.10.m.{j}.attn.qkv.conv.weight" in sd:
        p = f"model.10.m.{j}"
        B, C, H, W = b.shape
        t = _conv(sd, p + ".attn.qkv", b, 1, 1, act=False).reshape(B, C // 64, 128, H * W)
        logits = torch.einsum("bhdn,bhdm->bhnm", t[:, :, :32], t[:, :, 32:64]) * 32 ** -0.5
        got.append((logits - logits.mean(3, keepdim=True)).std().item())          # a query's common offset does not reach its softmax
        b = b + _attention(sd, p + ".attn", b, False, None)
        b = b + _conv(sd, p + ".ffn.1", _conv(sd, p + ".ffn.0", b, 1, 1), 1, 1, act=False)
        j += 1
    return got


# ---------------------------------------------------------------- the two kernels alone
def attention_exact(qkv, heads):
    """qkv [B, N, heads*128] (NHWC rows, per head q 32 | k 32 | v 64) -> [B, N, heads*64]; plain softmax in qkv's dtype."""
    B, N, _ = qkv.shape
    t = qkv.reshape(B, N, heads, 128)
    q, k, v = t[..., :32], t[..., 32:64], t[..., 64:]
    attn = (torch.einsum("bnhd,bmhd->bhnm", q, k) * 32 ** -0.5).softmax(-1)
    return torch.einsum("bhnm,bmhd->bnhd", attn, v).reshape(B, N, heads * 64)


def attention_tiled(qkv, heads, tile=64):
    """The kernel's algorithm in qkv's dtype: key tiles of ``tile`` with a running maximum m and sum l, the accumulator rescaled by
    exp(m_old - m_new) before every tile, one division at the end."""
    B, N, _ = qkv.shape
    t = qkv.reshape(B, N, heads, 128)
    q, k, v = t[..., :32], t[..., 32:64], t[..., 64:]
    m = torch.full((B, heads, N), -math.inf, dtype=qkv.dtype)
    l = torch.zeros((B, heads, N), dtype=qkv.dtype)
    acc = torch.zeros((B, heads, N, 64), dtype=qkv.dtype)
    for k0 in range(0, N, tile):
        s = torch.einsum("bnhd,bmhd->bhnm", q, k[:, k0:k0 + tile]) * qkv.new_tensor(32 ** -0.5)
        mn = torch.maximum(m, s.max(-1).values)
        corr = torch.exp(m - mn)
        p = torch.exp(s - mn.unsqueeze(-1))
        l = l * corr + p.sum(-1)
        acc = acc * corr.unsqueeze(-1) + torch.einsum("bhnm,bmhd->bhnd", p, v[:, k0:k0 + tile])
        m = mn
    return (acc / l.unsqueeze(-1)).permute(0, 2, 1, 3).reshape(B, N, heads * 64)


def dwconv_taps(x, w, bias, silu):
    """The depthwise kernel's algorithm in x's dtype: x [B,H,W,C] (NHWC), w [C,9], bias [C]; the nine taps added in ascending (ky, kx)
    order, then the bias, then x / (1 + exp(-x))."""
    B, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    acc = torch.zeros_like(x)
    for ky in range(3):
        for kx in range(3):
            acc = acc + xp[:, ky:ky + H, kx:kx + W] * w[:, ky * 3 + kx]
    y = acc + bias
    return y / (1 + torch.exp(-y)) if silu else y


# ---------------------------------------------------------------- the cases the host and the GPU tests share
BOX_REL, SCORE_ABS = 2e-4, 2e-4                              # the project's YOLOv8 bound: boxes relative to the largest coordinate, scores absolute
# (scale, (H, W), batch, nc): all five scales at 64 x 64 (4 tokens) and 96 x 160 (15 tokens), batch 1 and 3; yolo11n also at one token,
# at nc = 1 and at 640 x 640 (400 tokens: seven key tiles, the last one partial)
NET_CASES = [(s, shape, B, 2) for s in "nsmlx" for shape in ((64, 64), (96, 160)) for B in (1, 3)] + \
            [("n", (32, 32), 1, 2), ("n", (32, 32), 3, 2), ("n", (64, 64), 3, 1), ("n", (640, 640), 2, 2)]


def make_case(scale, shape, B, nc=2):
    """(state dict, input) of a network case: the seeds are part of the tests (the mutation check of tests/test_yolo11_host.py holds for
    exactly these tensors)."""
    from effocr_amd.localizer_engine import init_yolo11_state_dict
    return init_yolo11_state_dict(nc, scale, seed=1), blocky_images(B, shape, seed=3)


def blocky_images(B, shape, seed):
    """[B,3,H,W] in 0..1: uniform noise whose contrast and brightness change from one 16 x 16 block to the next (per channel).  Plain
    noise looks the same in every 32 x 32 patch, so the tokens of the stride-32 map are near copies of each other and the attention
    weights hardly matter; here the tokens differ."""
    g = torch.Generator().manual_seed(seed)
    noise = torch.rand(B, 3, *shape, generator=g)
    amp = torch.rand(B, 3, shape[0] // 16, shape[1] // 16, generator=g)
    off = torch.rand(B, 3, shape[0] // 16, shape[1] // 16, generator=g)
    amp, off = (t.repeat_interleave(16, 2).repeat_interleave(16, 3) for t in (amp, off))
    return noise * amp + (1 - amp) * off


def row_errors(got, ref):
    """(largest box error relative to the largest reference box coordinate, largest score error)."""
    err = (got.double() - ref.double()).abs()
    return (err[..., :4].max() / ref[..., :4].abs().max()).item(), err[..., 4:].max().item()
