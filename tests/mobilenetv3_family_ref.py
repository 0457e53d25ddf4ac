"""CPU restatement of timm's MobileNetV3 forward (``timm.create_model(name, num_classes=0)``) for mobilenetv3_small_075,
mobilenetv3_small_100 and mobilenetv3_large_100 (mobilenetv3_small_050 too) in plain torch functional ops over the state dict of
effocr_amd.weights (timm key names).  The block tables below are written out by hand from the models' descriptions (MobileNetV3 paper,
tables 1 and 2), independently of effocr_amd.weights.mobilenetv3_blocks: only kernel, stride, activation, squeeze-excite and residual
are stated, the channel counts come from the state dict's own shapes.  tests/test_mobilenetv3_family_host.py checks this against an
nn.Module tree built from the builder; the GPU tests compare the HIP encoder against this restatement.

``signal_sd`` / ``signal_reference``: the checkpoint and crops of the GPU tests' parity case whose embedding depends on the crop."""
import functools

import torch
import torch.nn.functional as F

from effocr_amd.weights import strip_prefix

EPS = 1e-5

# key, kind, kernel, stride, activation ("re" | "hs"), squeeze-excite, residual
SMALL = (
    ("blocks.0.0", "ds", 3, 2, "re", True, False),
    ("blocks.1.0", "ir", 3, 2, "re", False, False),
    ("blocks.1.1", "ir", 3, 1, "re", False, True),
    ("blocks.2.0", "ir", 5, 2, "hs", True, False),
    ("blocks.2.1", "ir", 5, 1, "hs", True, True),
    ("blocks.2.2", "ir", 5, 1, "hs", True, True),
    ("blocks.3.0", "ir", 5, 1, "hs", True, False),      # 40 -> 48 channels: no residual (at width 0.5 both are 24: see _residual)
    ("blocks.3.1", "ir", 5, 1, "hs", True, True),
    ("blocks.4.0", "ir", 5, 2, "hs", True, False),
    ("blocks.4.1", "ir", 5, 1, "hs", True, True),
    ("blocks.4.2", "ir", 5, 1, "hs", True, True),
)
LARGE = (
    ("blocks.0.0", "ds", 3, 1, "re", False, True),
    ("blocks.1.0", "ir", 3, 2, "re", False, False),
    ("blocks.1.1", "ir", 3, 1, "re", False, True),
    ("blocks.2.0", "ir", 5, 2, "re", True, False),
    ("blocks.2.1", "ir", 5, 1, "re", True, True),
    ("blocks.2.2", "ir", 5, 1, "re", True, True),
    ("blocks.3.0", "ir", 3, 2, "hs", False, False),
    ("blocks.3.1", "ir", 3, 1, "hs", False, True),
    ("blocks.3.2", "ir", 3, 1, "hs", False, True),
    ("blocks.3.3", "ir", 3, 1, "hs", False, True),
    ("blocks.4.0", "ir", 3, 1, "hs", True, False),      # 80 -> 112 channels
    ("blocks.4.1", "ir", 3, 1, "hs", True, True),
    ("blocks.5.0", "ir", 5, 2, "hs", True, False),
    ("blocks.5.1", "ir", 5, 1, "hs", True, True),
    ("blocks.5.2", "ir", 5, 1, "hs", True, True),
)
TABLES = {
    "mobilenetv3_small_050": (SMALL, "blocks.5.0", 1024),
    "mobilenetv3_small_075": (SMALL, "blocks.5.0", 1024),
    "mobilenetv3_small_100": (SMALL, "blocks.5.0", 1024),
    "mobilenetv3_large_100": (LARGE, "blocks.6.0", 1280),
}


def mobilenetv3_family_forward(arch, sd, x, round_pw=None):
    """x [B,3,S,S] (S a multiple of 32) -> features [B, 1024 | 1280] after conv_head + hard-swish, in x's dtype.
    ``round_pw`` (torch.float16 | torch.bfloat16): every pointwise convolution (conv_pw, conv_pwl, the ds block's conv_pw, blocks.N.0's
    conv, conv_head) runs with its BatchNorm folded in and the folded weight rounded once to that type — the ONLY rounding of the HIP
    encoders' 16-bit modes that is not an fp32 one; everything else stays exact.  Without it the path is the plain one, untouched."""
    table, cn, nf = TABLES[arch]
    P = {k: v.to(x.dtype) for k, v in strip_prefix(sd).items()}

    def bn(t, p):
        return F.batch_norm(t, P[p + ".running_mean"], P[p + ".running_var"], P[p + ".weight"], P[p + ".bias"], False, 0.0, EPS)

    def pw_bn(t, wkey, p):
        if round_pw is None:
            return bn(F.conv2d(t, P[wkey]), p)
        sc = P[p + ".weight"] / torch.sqrt(P[p + ".running_var"] + EPS)
        wf = (P[wkey] * sc[:, None, None, None]).to(torch.float32).to(round_pw).to(x.dtype)
        return F.conv2d(t, wf) + (P[p + ".bias"] - P[p + ".running_mean"] * sc)[None, :, None, None]

    def act(t, a):
        return F.hardswish(t) if a == "hs" else F.relu(t)

    def dw(t, w, s):
        k = w.shape[-1]
        assert w.shape[0] == t.shape[1] and w.shape[1] == 1
        return F.conv2d(t, w, stride=s, padding=k // 2, groups=t.shape[1])

    def se(t, p):
        m = t.mean((2, 3), keepdim=True)
        m = F.relu(F.conv2d(m, P[p + ".se.conv_reduce.weight"], P[p + ".se.conv_reduce.bias"]))
        return t * F.hardsigmoid(F.conv2d(m, P[p + ".se.conv_expand.weight"], P[p + ".se.conv_expand.bias"]))

    h = F.hardswish(bn(F.conv2d(x, P["conv_stem.weight"], stride=2, padding=1), "bn1"))
    for key, kind, k, s, a, has_se, res in table:
        sc = h
        assert (key + ".se.conv_reduce.weight" in P) == has_se, key
        if kind == "ds":
            assert P[key + ".conv_dw.weight"].shape[-1] == k
            h = act(bn(dw(h, P[key + ".conv_dw.weight"], s), key + ".bn1"), a)
            if has_se:
                h = se(h, key)
            h = pw_bn(h, key + ".conv_pw.weight", key + ".bn2")
        else:
            assert P[key + ".conv_dw.weight"].shape[-1] == k
            h = act(pw_bn(h, key + ".conv_pw.weight", key + ".bn1"), a)
            h = act(bn(dw(h, P[key + ".conv_dw.weight"], s), key + ".bn2"), a)
            if has_se:
                h = se(h, key)
            h = pw_bn(h, key + ".conv_pwl.weight", key + ".bn3")
        if _residual(res, s, sc, h):
            h = h + sc
    h = F.hardswish(pw_bn(h, cn + ".conv.weight", cn + ".bn1"))
    h = h.mean((2, 3), keepdim=True)
    wh = P["conv_head.weight"] if round_pw is None else P["conv_head.weight"].to(torch.float32).to(round_pw).to(x.dtype)
    h = F.hardswish(F.conv2d(h, wh, P["conv_head.bias"]))
    assert h.shape[1] == nf
    return h.flatten(1)


def _residual(stated, stride, inp, out):
    """The table's residual column, except where a width multiplier makes a stage boundary's channel counts equal (Small 0.5:
    blocks.3.0 maps 24 -> 24): timm adds the shortcut whenever stride is 1 and the channel counts agree."""
    same = stride == 1 and inp.shape[1] == out.shape[1]
    assert not stated or same
    return same


# ---------------------------------------------------------------------------------------------------------------------------------
# A checkpoint whose embedding depends on the crop.  Under init_state_dict's "unit" rule the hard-swish + squeeze-excite blocks damp the
# input's share of the embedding to 1e-4 - 1e-3 of its norm (under the 16-bit bounds), so a parity case on it cannot see a stem that
# ignores its input or a transposed depthwise kernel.  With every convolution but the squeeze-excite ones a gain larger the input's
# share neither dies nor explodes: all-zero and transposed crops move the float64 embedding by 0.3 - 1.0 of its norm (asserted by the
# tests that use it), while a float32 run of the restatement stays <= 1.4e-6 from float64.  Large at 1.6 reaches 5.7e-5: its gain is lower.
SIGNAL_GAIN = {"mobilenetv3_small_050": 1.6, "mobilenetv3_small_075": 1.6, "mobilenetv3_small_100": 1.6, "mobilenetv3_large_100": 1.45}
SIGNAL_IMGS = (32, 64, 96)
SIGNAL_B, SIGNAL_CROP_SEED = 3, 5


def _rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


@functools.lru_cache(maxsize=None)
def signal_sd(arch, img):
    """(cached: the tensors are never written; callers that hand the dict on make a copy of it)"""
    from effocr_amd.weights import init_state_dict
    sd = init_state_dict(arch, seed=7, img_size=img)
    return {k: (v * SIGNAL_GAIN[arch] if v.dim() == 4 and ".se." not in k else v) for k, v in sd.items()}


def signal_crops(img, B=SIGNAL_B):
    return torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(SIGNAL_CROP_SEED))


@functools.lru_cache(maxsize=None)
def signal_reference(arch, img, round_pw=None, B=SIGNAL_B):
    """float64 restatement on the signal checkpoint, computed once and shared (read-only).  Plain: (embedding as float32, max-norm change
    under all-zero crops, under transposed crops); with ``round_pw``: the embedding with only the pointwise weights rounded."""
    x = signal_crops(img, B).double()
    sd = signal_sd(arch, img)
    with torch.no_grad():
        ref = mobilenetv3_family_forward(arch, sd, x, round_pw=round_pw)
        if round_pw is not None:
            return ref.float()
        zero = mobilenetv3_family_forward(arch, sd, torch.zeros_like(x))
        transposed = mobilenetv3_family_forward(arch, sd, x.transpose(2, 3))
    return ref.float(), _rel(zero, ref), _rel(transposed, ref)
