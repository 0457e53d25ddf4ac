"""CPU restatement of timm's PyramidVisionTransformerV2 (pvt_v2_b0 ... pvt_v2_b5) over the timm-key state dict, in plain functional
torch, written from the architecture (timm pvt_v2.py / transformers modeling_pvt_v2.py) and not from effocr_amd.weights.param_shapes.
float64 by default: the reference of the GPU tests.  tests/test_pvt_host.py pins it to transformers.PvtV2Model.

``prec`` ("bf16" / "fp16") emulates the rounding points the library declares (csrc/pvt.hpp, csrc/pvt_api.hip: pvt_forward) in otherwise
float64 arithmetic: weights and crop pixels rounded once; every LayerNorm output except the patch embeddings' and the last stage norm;
the q, kv, fc1 and depthwise outputs; the attention's P and its output.  The residual stream, the convolution outputs in front of a
LayerNorm, all statistics and the embedding stay unrounded.

``mistake`` builds a deliberately wrong network (MISTAKES) for the sensitivity tests."""
import math

import torch
import torch.nn.functional as F

SR = (8, 4, 2, 1)
EPS = 1e-6
CFG = {   # name: (widths, heads, depths, mlp ratios)
    "pvt_v2_b0": ((32, 64, 160, 256), (1, 2, 5, 8), (2, 2, 2, 2), (8, 8, 4, 4)),
    "pvt_v2_b1": ((64, 128, 320, 512), (1, 2, 5, 8), (2, 2, 2, 2), (8, 8, 4, 4)),
    "pvt_v2_b2": ((64, 128, 320, 512), (1, 2, 5, 8), (3, 4, 6, 3), (8, 8, 4, 4)),
    "pvt_v2_b3": ((64, 128, 320, 512), (1, 2, 5, 8), (3, 4, 18, 3), (8, 8, 4, 4)),
    "pvt_v2_b4": ((64, 128, 320, 512), (1, 2, 5, 8), (3, 8, 27, 3), (8, 8, 4, 4)),
    "pvt_v2_b5": ((64, 128, 320, 512), (1, 2, 5, 8), (3, 6, 40, 3), (4, 4, 4, 4)),
    "pvt_v2_mini32_test": ((32, 64, 96, 128), (1, 2, 3, 4), (1, 1, 1, 1), (8, 8, 4, 4)),
    "pvt_v2_mini64_test": ((64, 128, 192, 256), (1, 2, 3, 4), (1, 1, 2, 1), (8, 8, 4, 4)),
}
MISTAKES = ("no_scale",        # scores not divided by sqrt(head_dim)
            "swap_kv",         # kv read as [v | k]
            "no_sr_norm",      # the reduction's LayerNorm dropped
            "gelu_first",      # GELU before the depthwise convolution
            "no_stage_norm",   # the stage norm dropped
            "token0",          # token 0 instead of the token mean
            "no_reduction")    # keys not reduced (sr = 1)
TORCH_PREC = {"bf16": torch.bfloat16, "fp16": torch.float16}


def rnd(t, prec):
    """t rounded once to prec's type (None / "fp32": unchanged), in t's own dtype."""
    if prec in (None, "fp32"):
        return t
    return t.to(TORCH_PREC[prec]).to(t.dtype)


# ---------------------------------------------------------------------------------------------------------------- operator references
def attention_ref(q, kv, B, N, M, heads, hd, scale=True, swap=False):
    """q [B*N, heads*hd], kv [B*M, 2*heads*hd] ([k | v], each split by heads) -> softmax(q k^T / sqrt(hd)) v as [B*N, heads*hd]."""
    C = heads * hd
    qh = q.reshape(B, N, heads, hd).permute(0, 2, 1, 3)
    k, v = kv.reshape(B, M, 2, heads, hd).permute(2, 0, 3, 1, 4)
    if swap:
        k, v = v, k
    s = qh @ k.transpose(-1, -2)
    if scale:
        s = s * (hd ** -0.5)
    return (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B * N, C)


def attention_emulated(q, kv, B, N, M, heads, hd, prec):
    """The same in float64 with exactly the roundings csrc/pvt.hpp declares for the 16-bit modes: p = exp(s - max) rounded to the operand
    type for the P V product while the denominator sums the unrounded p; O / l rounded once."""
    C = heads * hd
    q, kv = q.double(), kv.double()
    qh = q.reshape(B, N, heads, hd).permute(0, 2, 1, 3)
    k, v = kv.reshape(B, M, 2, heads, hd).permute(2, 0, 3, 1, 4)
    s = (qh @ k.transpose(-1, -2)) * (hd ** -0.5)
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = (rnd(p, prec) @ v) / p.sum(-1, keepdim=True)
    return rnd(o.permute(0, 2, 1, 3).reshape(B * N, C), prec)


def dwconv_gelu_ref(x, w, b, H, W, gelu_first=False):
    """x [B, H*W, C] -> GELU(depthwise 3x3 (w [C, 1, 3, 3], zero pad 1) + b), exact (erf) GELU."""
    B, _, C = x.shape
    t = x.transpose(1, 2).reshape(B, C, H, W)
    if gelu_first:
        t = F.gelu(t)
    t = F.conv2d(t, w, b, padding=1, groups=C)
    if not gelu_first:
        t = F.gelu(t)
    return t.flatten(2).transpose(1, 2)


def conv_ln_ref(img, w, b, lnw, lnb, stride, pad, norm=True):
    """img [B, Cin, H, H] -> LayerNorm over channels of conv(img) as token rows [B, OH*OH, Cout]."""
    t = F.conv2d(img, w, b, stride=stride, padding=pad).flatten(2).transpose(1, 2)
    return F.layer_norm(t, (t.shape[-1],), lnw, lnb, EPS) if norm else t


def tokens_to_img(t, H):
    B, _, C = t.shape
    return t.transpose(1, 2).reshape(B, C, H, H)


# ---------------------------------------------------------------------------------------------------------------- the network
def pvt_forward(arch, sd, x, prec=None, mistake=None, dtype=torch.float64):
    """x [B, 3, S, S] -> [B, D]: what timm.create_model(arch, num_classes=0) returns (the mean of the last stage's normalised tokens)."""
    assert mistake is None or mistake in MISTAKES, mistake
    widths, heads, depths, ratios = CFG[arch]
    P = {k: v.to(dtype) for k, v in sd.items()}

    def Wt(k):                                               # an operand weight: rounded once
        return rnd(P[k + ".weight"], prec)

    def ln(t, k):
        return F.layer_norm(t, (t.shape[-1],), P[k + ".weight"], P[k + ".bias"], EPS)

    t = rnd(x.to(dtype), prec)
    B, H = x.shape[0], x.shape[-1]
    for i, (C, nh, depth, sr) in enumerate(zip(widths, heads, depths, SR)):
        hd = C // nh
        if i == 0:
            xs = conv_ln_ref(t, Wt("patch_embed.proj"), P["patch_embed.proj.bias"], P["patch_embed.norm.weight"], P["patch_embed.norm.bias"], 4, 3)
            H = H // 4
        else:
            p = f"stages.{i}.downsample."
            xs = conv_ln_ref(tokens_to_img(t, H), Wt(p + "proj"), P[p + "proj.bias"], P[p + "norm.weight"], P[p + "norm.bias"], 2, 1)
            H = H // 2
        N = H * H
        for j in range(depth):
            p = f"stages.{i}.blocks.{j}."
            a = rnd(ln(xs, p + "norm1"), prec)
            q = rnd(F.linear(a, Wt(p + "attn.q"), P[p + "attn.q.bias"]), prec)
            if sr > 1 and mistake != "no_reduction":
                r = conv_ln_ref(tokens_to_img(a, H), Wt(p + "attn.sr"), P[p + "attn.sr.bias"], P[p + "attn.norm.weight"], P[p + "attn.norm.bias"],
                                sr, 0, norm=mistake != "no_sr_norm")
                r = rnd(r, prec)
            else:
                r = a
            M = r.shape[1]
            kv = rnd(F.linear(r, Wt(p + "attn.kv"), P[p + "attn.kv.bias"]), prec)
            if prec in (None, "fp32") or mistake is not None:
                o = attention_ref(q.reshape(B * N, C), kv.reshape(B * M, 2 * C), B, N, M, nh, hd, scale=mistake != "no_scale", swap=mistake == "swap_kv")
            else:
                o = attention_emulated(q.reshape(B * N, C), kv.reshape(B * M, 2 * C), B, N, M, nh, hd, prec).to(dtype)
            xs = xs + F.linear(o.reshape(B, N, C), Wt(p + "attn.proj"), P[p + "attn.proj.bias"])
            a = rnd(ln(xs, p + "norm2"), prec)
            h = rnd(F.linear(a, Wt(p + "mlp.fc1"), P[p + "mlp.fc1.bias"]), prec)
            h = rnd(dwconv_gelu_ref(h, Wt(p + "mlp.dwconv"), P[p + "mlp.dwconv.bias"], H, H, gelu_first=mistake == "gelu_first"), prec)
            xs = xs + F.linear(h, Wt(p + "mlp.fc2"), P[p + "mlp.fc2.bias"])
        if mistake != "no_stage_norm":
            xs = ln(xs, f"stages.{i}.norm")
        t = rnd(xs, prec) if i < 3 else xs
    return t[:, 0] if mistake == "token0" else t.mean(1)


# ---------------------------------------------------------------------------------------------------------------- transformers.PvtV2Model
def hf_config(arch, img_size):
    from transformers import PvtV2Config
    widths, heads, depths, ratios = CFG[arch]
    return PvtV2Config(image_size=img_size, depths=list(depths), hidden_sizes=list(widths), num_attention_heads=list(heads),
                       mlp_ratios=list(ratios), sr_ratios=list(SR), layer_norm_eps=EPS, qkv_bias=True, linear_attention=False,
                       hidden_act="gelu", drop_path_rate=0.0)


def hf_state_dict(arch, sd):
    """The timm-key state dict under transformers.PvtV2Model's names (kv split into key and value)."""
    widths, heads, depths, ratios = CFG[arch]
    out = {}

    def put(dst, src):
        out[dst + ".weight"], out[dst + ".bias"] = sd[src + ".weight"].clone(), sd[src + ".bias"].clone()
    for i, (C, depth, sr) in enumerate(zip(widths, depths, SR)):
        L = f"encoder.layers.{i}."
        pe = "patch_embed." if i == 0 else f"stages.{i}.downsample."
        put(L + "patch_embedding.proj", pe + "proj")
        put(L + "patch_embedding.layer_norm", pe + "norm")
        for j in range(depth):
            p, q = f"stages.{i}.blocks.{j}.", L + f"blocks.{j}."
            put(q + "layer_norm_1", p + "norm1")
            put(q + "attention.query", p + "attn.q")
            kw, kb = sd[p + "attn.kv.weight"], sd[p + "attn.kv.bias"]
            out[q + "attention.key.weight"], out[q + "attention.value.weight"] = kw[:C].clone(), kw[C:].clone()
            out[q + "attention.key.bias"], out[q + "attention.value.bias"] = kb[:C].clone(), kb[C:].clone()
            put(q + "attention.proj", p + "attn.proj")
            if sr > 1:
                put(q + "attention.spatial_reduction", p + "attn.sr")
                put(q + "attention.layer_norm", p + "attn.norm")
            put(q + "layer_norm_2", p + "norm2")
            put(q + "mlp.dense1", p + "mlp.fc1")
            put(q + "mlp.dwconv.dwconv", p + "mlp.dwconv")
            put(q + "mlp.dense2", p + "mlp.fc2")
        put(L + "layer_norm", f"stages.{i}.norm")
    return out


def hf_forward(arch, sd, x):
    """transformers.PvtV2Model on the same weights: the mean over its last hidden state's positions, float32."""
    from transformers import PvtV2Model
    m = PvtV2Model(hf_config(arch, x.shape[-1])).eval()
    missing, unexpected = m.load_state_dict(hf_state_dict(arch, sd), strict=True)
    assert not missing and not unexpected
    with torch.no_grad():
        h = m(pixel_values=x.float()).last_hidden_state
    return h.flatten(2).mean(-1)


# ---------------------------------------------------------------------------------------------------------------- test crops
def crops(n, img, seed):
    """n crops [n, 3, img, img] with structure at every stride's scale — square waves of period 8, 16, 32 and 64 pixels with per-crop,
    per-channel phases and amplitudes over a smooth ramp, plus a little noise: the token mean averages white noise away, not these."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(img, dtype=torch.float32), torch.arange(img, dtype=torch.float32), indexing="ij")
    out = torch.zeros(n, 3, img, img)
    for b in range(n):
        for c in range(3):
            v = torch.zeros(img, img)
            for period in (8, 16, 32, 64):
                ph = torch.rand(2, generator=g) * period
                amp = torch.rand(2, generator=g) + 0.25
                v += amp[0] * torch.sign(torch.sin(2 * math.pi * (xx + ph[0]) / period)) + amp[1] * torch.sign(torch.sin(2 * math.pi * (yy + ph[1]) / period))
            ramp = torch.rand(2, generator=g) - 0.5
            v = 0.35 * v + ramp[0] * xx / img + ramp[1] * yy / img
            out[b, c] = v + 0.1 * torch.randn(img, img, generator=g)
    return out
