"""Plain-torch restatement of timm's RegNetX / RegNetY (regnet.py) from timm-style keys, independent of effocr_amd/weights.py: it carries
its own copy of widths, depths and group widths.  Also: the CPU emulation of the roundings csrc/regnet.hpp declares (gconv_emulated for
the grouped convolution, regnet_forward(..., prec=...) for the whole network) and the key map to transformers.RegNetModel, the
independent pin of the architecture (timm is not installed where this project is developed: the key names are UNVERIFIED against it)."""
import re
from collections import OrderedDict

import torch
import torch.nn.functional as F

STEM = 32
BN_EPS = 1e-5
# name: (stage widths, stage depths, group width, squeeze-excite)
ARCHS = {
    "regnetx_002": ((24, 56, 152, 368), (1, 1, 4, 7), 8, False),
    "regnetx_004": ((32, 64, 160, 384), (1, 2, 7, 12), 16, False),
    "regnetx_006": ((48, 96, 240, 528), (1, 3, 5, 7), 24, False),
    "regnetx_008": ((64, 128, 288, 672), (1, 3, 7, 5), 16, False),
    "regnetx_016": ((72, 168, 408, 912), (2, 4, 10, 2), 24, False),
    "regnety_002": ((24, 56, 152, 368), (1, 1, 4, 7), 8, True),
    "regnety_004": ((48, 104, 208, 440), (1, 3, 6, 6), 8, True),
    "regnety_006": ((48, 112, 256, 608), (1, 3, 7, 4), 16, True),
    "regnety_008": ((64, 128, 320, 768), (1, 3, 8, 2), 16, True),
    "regnety_016": ((48, 120, 336, 888), (2, 6, 17, 2), 24, True),
    "regnetx_mini8_test": ((8, 24, 40, 56), (1, 1, 2, 1), 8, False),
    "regnetx_mini16_test": ((16, 32, 48, 80), (1, 1, 2, 1), 16, False),
    "regnety_mini24_test": ((24, 48, 72, 120), (1, 1, 2, 1), 24, True),
}
TEN = tuple(n for n in ARCHS if not n.endswith("_test"))
TORCH_T = {"fp16": torch.float16, "bf16": torch.bfloat16}
MISTAKES = ("groups_shifted", "no_gate", "relu_before_add", "odd_shortcut", "s1_stride1")


def header_constants(path):
    """{name: int} of the `constexpr int NAME = value` constants of a header (several per line allowed)."""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(RG_[A-Z_]+)\s*=\s*(\d+)", open(path).read())}


def split16(x, prec):
    """The activation as the kernels' two 16-bit operands: hi = rn16(x), lo = rn16(x - hi), both as fp32."""
    t = TORCH_T[prec]
    hi = x.float().to(t).float()
    lo = (x.float() - hi).to(t).float()
    return hi, lo


def round16(w, prec):
    return w.float().to(TORCH_T[prec]).float()


def gconv_ref(x, w, bias, stride, gw):
    """ReLU(grouped conv3x3 pad 1 + bias) in x's dtype.  x [B,C,H,H], w [C,gw,3,3]."""
    return F.relu(F.conv2d(x, w.to(x.dtype), bias.to(x.dtype), stride=stride, padding=1, groups=x.shape[1] // gw))


def gconv_emulated(x, w, bias, stride, gw, prec):
    """rg_gconv's declared roundings (csrc/regnet.hpp) on the CPU, fp32 in and out: the weight rounded once to the mode's type, the
    activation as hi + lo of that type, exact products accumulated in fp32 (here: two fp32 convolutions, in torch's order, added), then the
    fp32 bias and ReLU.  fp32 mode: a plain fp32 convolution."""
    x, w, bias = x.float(), w.float(), bias.float()
    groups = x.shape[1] // gw
    if prec == "fp32":
        return F.relu(F.conv2d(x, w, None, stride=stride, padding=1, groups=groups) + bias[None, :, None, None])
    hi, lo = split16(x, prec)
    w16 = round16(w, prec)
    acc = F.conv2d(hi, w16, None, stride=stride, padding=1, groups=groups) + F.conv2d(lo, w16, None, stride=stride, padding=1, groups=groups)
    return F.relu(acc + bias[None, :, None, None])


def blocks(arch):
    widths, depths, gw, se = ARCHS[arch]
    out, cin = [], STEM
    for si, (w, d) in enumerate(zip(widths, depths), start=1):
        for bi in range(1, d + 1):
            out.append(dict(key=f"s{si}.b{bi}", stage=si, cin=cin, w=w, stride=2 if bi == 1 else 1, gw=gw,
                            se=int(round(cin * 0.25)) if se else 0, down=bi == 1))
            cin = w
    return out


def regnet_forward(arch, sd, x, prec=None, mistake=None):
    """Embedding [B, w4] (the global average pool of the last block) in x's dtype (use float64 for the reference).
    prec "fp16" / "bf16": the emulation of the library's declared roundings — every BatchNorm folded in double and rounded to fp32, the
    1x1 and grouped weights rounded once more to the mode's type, every such convolution's input taken as hi + lo; stem, squeeze-excite,
    biases and adds unrounded.  Run it in float64: what remains is the roundings alone.
    mistake: one of MISTAKES, a deliberately wrong network for the sensitivity checks."""
    dt = x.dtype

    def conv_bn(t, p, stride=1, groups=1, pad=0, rounded=True):
        w = sd[p + ".conv.weight"].double()
        g, b = sd[p + ".bn.weight"].double(), sd[p + ".bn.bias"].double()
        m, v = sd[p + ".bn.running_mean"].double(), sd[p + ".bn.running_var"].double()
        sc = g / torch.sqrt(v + BN_EPS)
        if prec is None:
            y = F.conv2d(t, w.to(dt), None, stride=stride, padding=pad, groups=groups)
            return (y - m.to(dt)[None, :, None, None]) * sc.to(dt)[None, :, None, None] + b.to(dt)[None, :, None, None]
        wf = (w * sc[:, None, None, None]).float()
        bf = (b - m * sc).float()
        if rounded and prec != "fp32":
            wf = round16(wf, prec)
            hi, lo = split16(t, prec)
            t = hi.to(dt) + lo.to(dt)
        return F.conv2d(t, wf.to(dt), bf.to(dt), stride=stride, padding=pad, groups=groups)

    t = F.relu(conv_bn(x, "stem", stride=2, pad=1, rounded=False))
    for b in blocks(arch):
        p = b["key"]
        stride = 1 if (mistake == "s1_stride1" and b["stage"] == 1) else b["stride"]
        u = F.relu(conv_bn(t, p + ".conv1"))
        if mistake == "groups_shifted":
            u = torch.roll(u, b["gw"], dims=1)
        u = F.relu(conv_bn(u, p + ".conv2", stride=stride, groups=b["w"] // b["gw"], pad=1))
        if b["se"] and mistake != "no_gate":
            s = u.mean((2, 3), keepdim=True)
            s = F.relu(F.conv2d(s, sd[p + ".se.fc1.weight"].to(dt), sd[p + ".se.fc1.bias"].to(dt)))
            u = u * torch.sigmoid(F.conv2d(s, sd[p + ".se.fc2.weight"].to(dt), sd[p + ".se.fc2.bias"].to(dt)))
        u = conv_bn(u, p + ".conv3")
        if b["down"]:
            sc_in = t
            if stride == 2:
                sc_in = t[:, :, 1::2, 1::2] if mistake == "odd_shortcut" else t[:, :, ::2, ::2]
            short = conv_bn(sc_in, p + ".downsample")
        else:
            short = t
        t = F.relu(u) + short if mistake == "relu_before_add" else F.relu(u + short)
    return t.mean((2, 3))


def regnet_logits(arch, sd, x):
    return regnet_forward(arch, sd, x) @ sd["head.fc.weight"].to(x.dtype).t() + sd["head.fc.bias"].to(x.dtype)


# -- transformers.RegNetModel -----------------------------------------------------------------------------------------------------------
def hf_config(arch):
    from transformers import RegNetConfig
    widths, depths, gw, se = ARCHS[arch]
    return RegNetConfig(embedding_size=STEM, hidden_sizes=list(widths), depths=list(depths), groups_width=gw, layer_type="y" if se else "x")


def hf_state_dict(arch, sd):
    """The timm-style state dict under transformers.RegNetModel's names: embedder.embedder, encoder.stages.S.layers.L.layer.{0,1,(2 = SE),
    last}.{convolution, normalization} and .shortcut; the squeeze-excite convolutions are attention.0 / attention.2."""
    out = OrderedDict()

    def cna(dst, src):
        out[dst + ".convolution.weight"] = sd[src + ".conv.weight"]
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            out[f"{dst}.normalization.{leaf}"] = sd[f"{src}.bn.{leaf}"]
    cna("embedder.embedder", "stem")
    for b in blocks(arch):
        si, bi = (int(v[1:]) for v in b["key"].split("."))
        q = f"encoder.stages.{si - 1}.layers.{bi - 1}"
        cna(q + ".layer.0", b["key"] + ".conv1")
        cna(q + ".layer.1", b["key"] + ".conv2")
        if b["se"]:
            for i, fc in ((0, "fc1"), (2, "fc2")):
                out[f"{q}.layer.2.attention.{i}.weight"] = sd[f"{b['key']}.se.{fc}.weight"]
                out[f"{q}.layer.2.attention.{i}.bias"] = sd[f"{b['key']}.se.{fc}.bias"]
        cna(f"{q}.layer.{3 if b['se'] else 2}", b["key"] + ".conv3")
        if b["down"]:
            cna(q + ".shortcut", b["key"] + ".downsample")
    return out
