"""CPU restatement of timm's MobileNetV3-Small forward (``timm.create_model("mobilenetv3_small_050", num_classes=0)``) in plain torch
functional ops over the state dict of effocr_amd.weights (timm key names).  The block table below is written out by hand from the
model's description, independently of effocr_amd.weights.mobilenetv3_blocks; tests/test_mobilenetv3_host.py checks the two against
each other (an nn.Module tree built from the builder loads the same state dict with strict=True and must agree in float64).  The GPU
tests compare the HIP encoder against this restatement."""
import torch
import torch.nn.functional as F

from effocr_amd.weights import strip_prefix

EPS = 1e-5

# key, kind, kernel, stride, activation ("re" | "hs"), squeeze-excite, residual  (mobilenetv3_small_050)
SMALL_050 = (
    ("blocks.0.0", "ds", 3, 2, "re", True, False),
    ("blocks.1.0", "ir", 3, 2, "re", False, False),
    ("blocks.1.1", "ir", 3, 1, "re", False, True),
    ("blocks.2.0", "ir", 5, 2, "hs", True, False),
    ("blocks.2.1", "ir", 5, 1, "hs", True, True),
    ("blocks.2.2", "ir", 5, 1, "hs", True, True),
    ("blocks.3.0", "ir", 5, 1, "hs", True, True),
    ("blocks.3.1", "ir", 5, 1, "hs", True, True),
    ("blocks.4.0", "ir", 5, 2, "hs", True, False),
    ("blocks.4.1", "ir", 5, 1, "hs", True, True),
    ("blocks.4.2", "ir", 5, 1, "hs", True, True),
)


def mobilenetv3_forward(arch, sd, x):
    """x [B,3,S,S] (S a multiple of 32) -> features [B, 1024] after conv_head + hard-swish, in x's dtype."""
    assert arch == "mobilenetv3_small_050"
    P = {k: v.to(x.dtype) for k, v in strip_prefix(sd).items()}

    def bn(t, p):
        return F.batch_norm(t, P[p + ".running_mean"], P[p + ".running_var"], P[p + ".weight"], P[p + ".bias"], False, 0.0, EPS)

    def act(t, a):
        return F.hardswish(t) if a == "hs" else F.relu(t)

    def dw(t, w, s):
        k = w.shape[-1]
        return F.conv2d(t, w, stride=s, padding=k // 2, groups=t.shape[1])

    def se(t, p):
        m = t.mean((2, 3), keepdim=True)
        m = F.relu(F.conv2d(m, P[p + ".se.conv_reduce.weight"], P[p + ".se.conv_reduce.bias"]))
        return t * F.hardsigmoid(F.conv2d(m, P[p + ".se.conv_expand.weight"], P[p + ".se.conv_expand.bias"]))

    h = F.hardswish(bn(F.conv2d(x, P["conv_stem.weight"], stride=2, padding=1), "bn1"))
    for key, kind, k, s, a, has_se, res in SMALL_050:
        sc = h
        if kind == "ds":
            h = act(bn(dw(h, P[key + ".conv_dw.weight"], s), key + ".bn1"), a)
            if has_se:
                h = se(h, key)
            h = bn(F.conv2d(h, P[key + ".conv_pw.weight"]), key + ".bn2")
        else:
            h = act(bn(F.conv2d(h, P[key + ".conv_pw.weight"]), key + ".bn1"), a)
            h = act(bn(dw(h, P[key + ".conv_dw.weight"], s), key + ".bn2"), a)
            if has_se:
                h = se(h, key)
            h = bn(F.conv2d(h, P[key + ".conv_pwl.weight"]), key + ".bn3")
        if res:
            h = h + sc
    h = F.hardswish(bn(F.conv2d(h, P["blocks.5.0.conv.weight"]), "blocks.5.0.bn1"))
    h = h.mean((2, 3), keepdim=True)
    h = F.hardswish(F.conv2d(h, P["conv_head.weight"], P["conv_head.bias"]))
    return h.flatten(1)
