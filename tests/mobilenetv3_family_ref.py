"""CPU restatement of timm's MobileNetV3 forward (``timm.create_model(name, num_classes=0)``) for mobilenetv3_small_075,
mobilenetv3_small_100 and mobilenetv3_large_100 (mobilenetv3_small_050 too) in plain torch functional ops over the state dict of
effocr_amd.weights (timm key names).  The block tables below are written out by hand from the models' descriptions (MobileNetV3 paper,
tables 1 and 2), independently of effocr_amd.weights.mobilenetv3_blocks: only kernel, stride, activation, squeeze-excite and residual
are stated, the channel counts come from the state dict's own shapes.  tests/test_mobilenetv3_family_host.py checks this against an
nn.Module tree built from the builder; the GPU tests compare the HIP encoder against this restatement."""
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


def mobilenetv3_family_forward(arch, sd, x):
    """x [B,3,S,S] (S a multiple of 32) -> features [B, 1024 | 1280] after conv_head + hard-swish, in x's dtype."""
    table, cn, nf = TABLES[arch]
    P = {k: v.to(x.dtype) for k, v in strip_prefix(sd).items()}

    def bn(t, p):
        return F.batch_norm(t, P[p + ".running_mean"], P[p + ".running_var"], P[p + ".weight"], P[p + ".bias"], False, 0.0, EPS)

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
            h = bn(F.conv2d(h, P[key + ".conv_pw.weight"]), key + ".bn2")
        else:
            assert P[key + ".conv_dw.weight"].shape[-1] == k
            h = act(bn(F.conv2d(h, P[key + ".conv_pw.weight"]), key + ".bn1"), a)
            h = act(bn(dw(h, P[key + ".conv_dw.weight"], s), key + ".bn2"), a)
            if has_se:
                h = se(h, key)
            h = bn(F.conv2d(h, P[key + ".conv_pwl.weight"]), key + ".bn3")
        if _residual(res, s, sc, h):
            h = h + sc
    h = F.hardswish(bn(F.conv2d(h, P[cn + ".conv.weight"]), cn + ".bn1"))
    h = h.mean((2, 3), keepdim=True)
    h = F.hardswish(F.conv2d(h, P["conv_head.weight"], P["conv_head.bias"]))
    assert h.shape[1] == nf
    return h.flatten(1)


def _residual(stated, stride, inp, out):
    """The table's residual column, except where a width multiplier makes a stage boundary's channel counts equal (Small 0.5:
    blocks.3.0 maps 24 -> 24): timm adds the shortcut whenever stride is 1 and the channel counts agree."""
    same = stride == 1 and inp.shape[1] == out.shape[1]
    assert not stated or same
    return same
