"""CPU restatement of timm's EfficientNet-B0 forward (``timm.create_model(name, num_classes=0)``) for efficientnet_b0 and
tf_efficientnet_b0 in plain torch functional ops over the state dict of effocr_amd.weights (timm key names).  The block table below is
written out by hand from the model's description (EfficientNet paper, table 1), independently of effocr_amd.weights.efficientnet_blocks:
only kernel, stride and residual are stated, the channel counts come from the state dict's own shapes.
tests/test_efficientnet_host.py pins the ``tf_`` variant against transformers.EfficientNetModel (an independent implementation of the
same network) and the plain variant against an nn.Module tree built from the builder; the GPU tests compare the HIP encoder against this
restatement."""
import torch
import torch.nn.functional as F

from effocr_amd.weights import strip_prefix

# name -> (BN eps, TensorFlow SAME padding)
VARIANTS = {"efficientnet_b0": (1e-5, False), "tf_efficientnet_b0": (1e-3, True)}

# key, kind, kernel, stride, residual
B0 = (
    ("blocks.0.0", "ds", 3, 1, False),                  # 32 -> 16 channels: no residual
    ("blocks.1.0", "ir", 3, 2, False),
    ("blocks.1.1", "ir", 3, 1, True),
    ("blocks.2.0", "ir", 5, 2, False),
    ("blocks.2.1", "ir", 5, 1, True),
    ("blocks.3.0", "ir", 3, 2, False),
    ("blocks.3.1", "ir", 3, 1, True),
    ("blocks.3.2", "ir", 3, 1, True),
    ("blocks.4.0", "ir", 5, 1, False),                  # 80 -> 112 channels
    ("blocks.4.1", "ir", 5, 1, True),
    ("blocks.4.2", "ir", 5, 1, True),
    ("blocks.5.0", "ir", 5, 2, False),
    ("blocks.5.1", "ir", 5, 1, True),
    ("blocks.5.2", "ir", 5, 1, True),
    ("blocks.5.3", "ir", 5, 1, True),
    ("blocks.6.0", "ir", 3, 1, False),                  # 192 -> 320 channels
)


def same_pad(t, k, s):
    """TensorFlow SAME: total padding max((ceil(H / s) - 1) s + k - H, 0) per axis, the smaller half in front."""
    H, Wd = t.shape[-2:]
    ph = max((-(-H // s) - 1) * s + k - H, 0)
    pw = max((-(-Wd // s) - 1) * s + k - Wd, 0)
    return F.pad(t, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))


def efficientnet_forward(arch, sd, x, round_pw=None, eps=None, tf=None):
    """x [B,3,S,S] (S a multiple of 32) -> features [B, 1280]: the global average pool of SiLU(bn2(conv_head)), in x's dtype.
    ``round_pw`` (torch.float16 | torch.bfloat16): every pointwise convolution (conv_pw, conv_pwl, blocks.0.0's conv_pw, conv_head) runs
    with its BatchNorm folded in and the folded weight rounded once to that type — the ONLY rounding of the HIP encoder's 16-bit modes
    that is not an fp32 one; everything else stays exact.  ``eps`` / ``tf`` override ONE property of the named variant (tests that tell
    the BN eps from the padding)."""
    eps, tf = (VARIANTS[arch][0] if eps is None else eps), (VARIANTS[arch][1] if tf is None else tf)
    P = {k: v.to(x.dtype) for k, v in strip_prefix(sd).items()}

    def bn(t, p):
        return F.batch_norm(t, P[p + ".running_mean"], P[p + ".running_var"], P[p + ".weight"], P[p + ".bias"], False, 0.0, eps)

    def conv(t, w, k, s, groups=1):
        if tf:
            return F.conv2d(same_pad(t, k, s), w, stride=s, groups=groups)
        return F.conv2d(t, w, stride=s, padding=k // 2, groups=groups)

    def pw_bn(t, wkey, p):
        if round_pw is None:
            return bn(F.conv2d(t, P[wkey]), p)
        sc = P[p + ".weight"] / torch.sqrt(P[p + ".running_var"] + eps)
        wf = (P[wkey] * sc[:, None, None, None]).to(torch.float32).to(round_pw).to(x.dtype)
        return F.conv2d(t, wf) + (P[p + ".bias"] - P[p + ".running_mean"] * sc)[None, :, None, None]

    def dw(t, w, s):
        assert w.shape[0] == t.shape[1] and w.shape[1] == 1
        return conv(t, w, w.shape[-1], s, groups=t.shape[1])

    def se(t, p, cin):
        assert P[p + ".se.conv_reduce.weight"].shape[0] == round(cin * 0.25), p      # a quarter of the block's INPUT channels
        m = t.mean((2, 3), keepdim=True)
        m = F.silu(F.conv2d(m, P[p + ".se.conv_reduce.weight"], P[p + ".se.conv_reduce.bias"]))
        return t * torch.sigmoid(F.conv2d(m, P[p + ".se.conv_expand.weight"], P[p + ".se.conv_expand.bias"]))

    h = F.silu(bn(conv(x, P["conv_stem.weight"], 3, 2), "bn1"))
    for key, kind, k, s, res in B0:
        sc = h
        assert P[key + ".conv_dw.weight"].shape[-1] == k
        if kind == "ds":
            h = F.silu(bn(dw(h, P[key + ".conv_dw.weight"], s), key + ".bn1"))
            h = se(h, key, sc.shape[1])
            h = pw_bn(h, key + ".conv_pw.weight", key + ".bn2")
        else:
            h = F.silu(pw_bn(h, key + ".conv_pw.weight", key + ".bn1"))
            h = F.silu(bn(dw(h, P[key + ".conv_dw.weight"], s), key + ".bn2"))
            h = se(h, key, sc.shape[1])
            h = pw_bn(h, key + ".conv_pwl.weight", key + ".bn3")
        assert res == (s == 1 and sc.shape[1] == h.shape[1]), key
        if res:
            h = h + sc
    h = F.silu(pw_bn(h, "conv_head.weight", "bn2"))
    assert h.shape[1] == 1280
    return h.mean((2, 3))
