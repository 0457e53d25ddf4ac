"""Plain-torch restatement of the LeViT encoders (timm levit.py with num_classes=0), written from the architecture and not from
effocr_amd.weights.param_shapes: a stem of four 3x3 stride-2 convolutions + BatchNorm (hardswish after the first three), three stages of
``x += Attention(x); x += MLP(x)`` blocks, a down-sampling attention (no residual) + MLP between the stages, the mean of the final tokens.
It reads the timm-keyed state dict and runs in the dtype of ``x`` (float64 or float32) with every BatchNorm UNFOLDED.
tests/test_levit_host.py pins it to an independent implementation, transformers' LevitModel; the GPU tests compare libeffocr_levit.so
against it.  ``levit_forward(..., emulate=dtype)`` is the same network in float64 with only the roundings csrc/levit.hpp and
csrc/levit_api.hip declare for a 16-bit mode (BatchNorm folded in double and the weights rounded once; activations rounded between the
kernels; the attention's P and output), computed without a GPU: the yardstick of the 16-bit bounds."""
import math
import os
import re

import torch
import torch.nn.functional as F

from effocr_amd import weights as W

EPS = 1e-5                   # every BatchNorm of levit.py
KEY_TILE = 32                # LEVIT_KTILE of csrc/levit.hpp: the 16-bit kernel rescales its running softmax once per 32 keys


def header_grids():
    """(token grids the attention tests walk, keys per MFMA tile, key tail of the 14 x 14 grid), read from csrc/levit.hpp — the one place
    that states the kernel's tile sizes."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "effocr_amd", "csrc", "levit.hpp")).read()
    grids = [int(v) for v in re.search(r"LEVIT_TEST_GRIDS\[\] = \{([^}]*)\}", src).group(1).split(",")]
    tile, tail = (int(re.search(rf"constexpr int {n} = (\d+);", src).group(1)) for n in ("LEVIT_KTILE", "LEVIT_KTAIL"))
    return grids, tile, tail


def sub(R):
    """token grid per side after the stride-2 sub-sampling"""
    return (R - 1) // 2 + 1


def bias_index(R, stride=1):
    """[Tq, Tk] int64 index into an attention_biases row of R^2 entries: |dy| R + |dx| between the query's position on the key grid
    (stride 2: the even rows and columns) and the key's."""
    Rq = sub(R) if stride == 2 else R
    ky, kx = torch.meshgrid(torch.arange(R), torch.arange(R), indexing="ij")
    qy, qx = torch.meshgrid(torch.arange(Rq) * stride, torch.arange(Rq) * stride, indexing="ij")
    dy = (qy.reshape(-1, 1) - ky.reshape(1, -1)).abs()
    dx = (qx.reshape(-1, 1) - kx.reshape(1, -1)).abs()
    return dy * R + dx


def hardswish(x):
    return x * (x + 3).clamp(0, 6) / 6


def attention_ref(q, k, v, table, R, stride=1, act=False, index=None):
    """q [B, h, Tq, kd], k [B, h, Tk, kd], v [B, h, Tk, vd], table [h, R^2] -> [B, h, Tq, vd] in the inputs' dtype."""
    idx = bias_index(R, stride) if index is None else index
    s = q @ k.transpose(-1, -2) * q.shape[-1] ** -0.5 + table.to(q.dtype)[:, idx]
    o = s.softmax(-1) @ v
    return hardswish(o) if act else o


def rounder(dtype):
    """x -> x rounded once to ``dtype`` and back (identity for None)."""
    if dtype is None:
        return lambda t: t
    return lambda t: t.to(dtype).to(t.dtype)


def attention_emulated(q, k, v, table, R, stride=1, act=False, dtype=torch.bfloat16):
    """attention_ref in float64 with only the roundings csrc/levit.hpp declares for the 16-bit kernel: the key tiles of 32 are walked
    with a running maximum; p_j = exp(s_j - running max) is rounded to ``dtype`` for P V while l sums the unrounded values; act(O / l) is
    rounded once.  q, k, v must already hold ``dtype`` values."""
    rnd = rounder(dtype)
    q, k, v = q.double(), k.double(), v.double()
    s = q @ k.transpose(-1, -2) * q.shape[-1] ** -0.5 + table.double()[:, bias_index(R, stride)]
    Tk = s.shape[-1]
    tiles = [slice(t, min(t + KEY_TILE, Tk)) for t in range(0, Tk, KEY_TILE)]
    run = torch.full(s.shape[:-1], -math.inf, dtype=torch.float64)
    maxes = []
    for t in tiles:
        run = torch.maximum(run, s[..., t].amax(-1))
        maxes.append(run)
    final = maxes[-1]
    o = torch.zeros(s.shape[:-1] + (v.shape[-1],), dtype=torch.float64)
    l = torch.zeros(s.shape[:-1], dtype=torch.float64)
    for t, m in zip(tiles, maxes):
        p = torch.exp(s[..., t] - m[..., None])
        w = torch.exp(m - final)                           # the later rescalings, exact in this emulation
        o = o + (rnd(p) @ v[..., t, :]) * w[..., None]
        l = l + p.sum(-1) * w
    o = o / l[..., None]
    return rnd(hardswish(o) if act else o)


def _bn(P, p, x, dim):
    """eval-mode BatchNorm over dimension ``dim`` of x"""
    shape = [1] * x.dim()
    shape[dim] = -1
    g, b, m, v = (P[f"{p}.{leaf}"].to(x.dtype).reshape(shape) for leaf in ("weight", "bias", "running_mean", "running_var"))
    return (x - m) / torch.sqrt(v + EPS) * g + b


def _fold(P, p):
    """(scale, shift) of the BatchNorm at ``p`` in float64"""
    g, b, m, v = (P[f"{p}.{leaf}"].double() for leaf in ("weight", "bias", "running_mean", "running_var"))
    sc = g / torch.sqrt(v + EPS)
    return sc, b - m * sc


def levit_forward(arch, sd, x, emulate=None, zero_biases=False, transpose_biases=False, drop_attention=None):
    """[B, 3, S, S] -> [B, D]: the mean of the final tokens, in x's dtype.

    emulate: None = exact arithmetic in x's dtype with BatchNorm unfolded; torch.float16 / torch.bfloat16 = float64 arithmetic with the
    roundings of that precision mode of libeffocr_levit.so (x must be float64).
    zero_biases / transpose_biases / drop_attention=(stage, block): the sensitivity switches of tests/test_gpu_levit.py — every attention
    bias zeroed, looked up with |dy| and |dx| swapped, or one block's attention branch removed."""
    widths, kd, heads, depths = W.LEVIT_CFG[arch]
    P = {k: v for k, v in sd.items()}
    rnd = rounder(emulate)
    dt = x.dtype

    def linear_norm(p, t):
        w = P[p + ".linear.weight"]
        if emulate is None:
            return _bn(P, p + ".bn", t @ w.to(dt).T, -1)
        sc, sh = _fold(P, p + ".bn")
        return t @ rnd((w.double() * sc[:, None]).float().double()).T + sh.float().double()

    def conv_norm(p, t, act, last):
        w = P[p + ".linear.weight"]
        if emulate is None:
            y = _bn(P, p + ".bn", F.conv2d(t, w.to(dt), stride=2, padding=1), 1)
            return hardswish(y) if act else y
        sc, sh = _fold(P, p + ".bn")
        y = F.conv2d(t, rnd((w.double() * sc[:, None, None, None]).float().double()), stride=2, padding=1) + sh.float().double()[None, :, None, None]
        y = hardswish(y) if act else y
        return y if last else rnd(y)                       # the last convolution writes the fp32 residual stream

    def table(p, R):
        t = P[p].to(dt)
        if zero_biases:
            t = torch.zeros_like(t)
        if transpose_biases:
            t = t.reshape(-1, R, R).transpose(1, 2).reshape(-1, R * R)
        return t

    def attend(q, k, v, tb, R, stride):
        if emulate is None:
            return attention_ref(q, k, v, tb, R, stride, act=True)
        return attention_emulated(q, k, v, tb, R, stride, act=True, dtype=emulate)

    def mlp(p, t):
        h = rnd(linear_norm(p + ".ln1", rnd(t)))
        return linear_norm(p + ".ln2", rnd(hardswish(h)))

    t = rnd(x)
    for i in range(4):
        t = conv_norm(f"stem.conv{i + 1}", t, act=i < 3, last=i == 3)
    B, C, R, _ = t.shape
    t = t.flatten(2).transpose(1, 2)                       # [B, R^2, C], token = y R + x
    for st in range(3):
        if st > 0:
            p = f"stages.{st}.downsample."
            h = widths[st - 1] // kd
            Rq = sub(R)
            kv = rnd(linear_norm(p + "attn_downsample.kv", rnd(t))).reshape(B, R * R, h, 5 * kd)
            k, v = kv[..., :kd].transpose(1, 2), kv[..., kd:].transpose(1, 2)
            tq = t.reshape(B, R, R, -1)[:, ::2, ::2].reshape(B, Rq * Rq, -1)
            q = rnd(linear_norm(p + "attn_downsample.q.ln", rnd(tq))).reshape(B, Rq * Rq, h, kd).transpose(1, 2)
            o = attend(q, k, v, table(p + "attn_downsample.attention_biases", R), R, 2)
            t = linear_norm(p + "attn_downsample.proj.ln", o.transpose(1, 2).reshape(B, Rq * Rq, h * 4 * kd))
            t = t + mlp(p + "mlp", t)
            R = Rq
        for j in range(depths[st]):
            p = f"stages.{st}.blocks.{j}."
            h = heads[st]
            qkv = rnd(linear_norm(p + "attn.qkv", rnd(t))).reshape(B, R * R, h, 4 * kd)
            q, k, v = (u.transpose(1, 2) for u in (qkv[..., :kd], qkv[..., kd:2 * kd], qkv[..., 2 * kd:]))
            if drop_attention != (st, j):
                o = attend(q, k, v, table(p + "attn.attention_biases", R), R, 1)
                t = t + linear_norm(p + "attn.proj.ln", o.transpose(1, 2).reshape(B, R * R, h * 2 * kd))
            t = t + mlp(p + "mlp", t)
    return t.mean(1)


def levit_logits(arch, sd, x):
    """levit_forward + timm's classifier: the average of the two BatchNorm1d + Linear heads, unfolded."""
    e = levit_forward(arch, sd, x)
    out = 0
    for h in ("head", "head_dist"):
        out = out + F.linear(_bn(sd, h + ".bn", e, -1), sd[h + ".linear.weight"].to(e.dtype), sd[h + ".linear.bias"].to(e.dtype))
    return out / 2


# -- transformers.LevitModel -------------------------------------------------------------------------------------------------------
def hf_config(arch, img_size):
    from transformers import LevitConfig
    widths, kd, heads, depths = W.LEVIT_CFG[arch]
    return LevitConfig(image_size=img_size, hidden_sizes=list(widths), num_attention_heads=list(heads), depths=list(depths),
                       key_dim=[kd] * 3, mlp_ratio=[2, 2, 2], attention_ratio=[2, 2, 2],
                       down_ops=[["Subsample", kd, widths[0] // kd, 4, 2, 2], ["Subsample", kd, widths[1] // kd, 4, 2, 2], [""]])


def hf_state_dict(arch, sd):
    """The timm-keyed state dict under transformers.LevitModel's names.  There the down-sampling attention and its MLP close stage i - 1
    (timm >= 0.9: they open stage i)."""
    widths, kd, heads, depths = W.LEVIT_CFG[arch]
    out = {}

    def ln(dst, src):
        out[dst + ".linear.weight"] = sd[src + ".linear.weight"]
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            out[f"{dst}.batch_norm.{leaf}"] = sd[f"{src}.bn.{leaf}"]

    for i in range(1, 5):
        out[f"patch_embeddings.embedding_layer_{i}.convolution.weight"] = sd[f"stem.conv{i}.linear.weight"]
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            out[f"patch_embeddings.embedding_layer_{i}.batch_norm.{leaf}"] = sd[f"stem.conv{i}.bn.{leaf}"]
    for st in range(3):
        base = f"encoder.stages.{st}.layers."
        n = 0
        for j in range(depths[st]):
            p = f"stages.{st}.blocks.{j}."
            out[f"{base}{n}.module.attention_biases"] = sd[p + "attn.attention_biases"]
            ln(f"{base}{n}.module.queries_keys_values", p + "attn.qkv")
            ln(f"{base}{n}.module.projection", p + "attn.proj.ln")
            ln(f"{base}{n + 1}.module.linear_up", p + "mlp.ln1")
            ln(f"{base}{n + 1}.module.linear_down", p + "mlp.ln2")
            n += 2
        if st < 2:
            p = f"stages.{st + 1}.downsample."
            out[f"{base}{n}.attention_biases"] = sd[p + "attn_downsample.attention_biases"]
            ln(f"{base}{n}.keys_values", p + "attn_downsample.kv")
            ln(f"{base}{n}.queries", p + "attn_downsample.q.ln")
            ln(f"{base}{n}.projection", p + "attn_downsample.proj.ln")
            ln(f"{base}{n + 1}.module.linear_up", p + "mlp.ln1")
            ln(f"{base}{n + 1}.module.linear_down", p + "mlp.ln2")
    return out
