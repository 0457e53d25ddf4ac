"""CPU restatement of timm's ResNet-34 / ResNet-50 forward (``timm.create_model("resnet34" | "resnet50", num_classes=0)``) in plain torch
functional ops, over the state dict of effocr_amd.weights (timm key names).  The GPU tests compare the HIP encoder against it; it is pinned
to an independent implementation, transformers' ResNetModel, by tests/test_resnet_host.py.  It reads nothing outside the repository."""
import torch.nn.functional as F

from effocr_amd.weights import RESNET_CFG, strip_prefix

EPS = 1e-5


def _bn(x, P, p, relu):
    y = F.batch_norm(x, P[p + ".running_mean"], P[p + ".running_var"], P[p + ".weight"], P[p + ".bias"], False, 0.0, EPS)
    return F.relu(y) if relu else y


def resnet_forward(arch, sd, x):
    """x [B,3,S,S] fp32 (S a multiple of 32) -> globally average-pooled features [B, D] fp32 (float64 if x is float64)."""
    depths, _, block = RESNET_CFG[arch]
    sd = strip_prefix(sd)
    P = {k: v.to(x.dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    h = _bn(F.conv2d(x, P["conv1.weight"], stride=2, padding=3), P, "bn1", True)
    h = F.max_pool2d(h, 3, 2, 1)
    for li, nb in enumerate(depths, start=1):
        for bi in range(nb):
            p = f"layer{li}.{bi}."
            s = 2 if (bi == 0 and li > 1) else 1
            if block == "bottleneck":                    # timm Bottleneck: the stride sits on the 3x3 conv2
                y = _bn(F.conv2d(h, P[p + "conv1.weight"]), P, p + "bn1", True)
                y = _bn(F.conv2d(y, P[p + "conv2.weight"], stride=s, padding=1), P, p + "bn2", True)
                y = _bn(F.conv2d(y, P[p + "conv3.weight"]), P, p + "bn3", False)
            else:
                y = _bn(F.conv2d(h, P[p + "conv1.weight"], stride=s, padding=1), P, p + "bn1", True)
                y = _bn(F.conv2d(y, P[p + "conv2.weight"], padding=1), P, p + "bn2", False)
            if p + "downsample.0.weight" in P:
                h = _bn(F.conv2d(h, P[p + "downsample.0.weight"], stride=s), P, p + "downsample.1", False)
            h = F.relu(y + h)
    return h.mean(dim=(2, 3))


def hf_state_dict(sd):
    """timm key names -> transformers ResNetModel key names (layer_type "basic" / "bottleneck", downsample_in_bottleneck=False)."""
    out = {}
    for k, v in strip_prefix(sd).items():
        if k.startswith("conv1."):
            k = "embedder.embedder.convolution." + k[len("conv1."):]
        elif k.startswith("bn1."):
            k = "embedder.embedder.normalization." + k[len("bn1."):]
        elif k.startswith("layer"):
            li, bi, rest = k.split(".", 2)
            q = f"encoder.stages.{int(li[5:]) - 1}.layers.{bi}."
            if rest.startswith("downsample.0."):
                k = q + "shortcut.convolution." + rest[len("downsample.0."):]
            elif rest.startswith("downsample.1."):
                k = q + "shortcut.normalization." + rest[len("downsample.1."):]
            else:
                mod, leaf = rest.split(".", 1)          # convN / bnN
                n = int(mod[-1]) - 1
                k = q + f"layer.{n}." + ("convolution." if mod.startswith("conv") else "normalization.") + leaf
        else:
            continue                                     # the classifier fc
        out[k] = v
    return out
