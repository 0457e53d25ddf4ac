"""CPU restatement of timm's ConvNeXt forward (``timm.create_model("convnext_tiny", num_classes=0)``) in plain torch functional ops,
over the state dict of effocr_amd.weights (timm key names).  The GPU tests compare the HIP encoder against it; it is pinned to an
independent implementation, transformers' ConvNextModel, by tests/test_convnext_host.py.  It reads nothing outside the repository."""
import torch
import torch.nn.functional as F

from effocr_amd.weights import CONVNEXT_CFG, strip_prefix

EPS = 1e-6


def _ln_channels_last(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, EPS)


def convnext_forward(arch, sd, x):
    """x [B,3,S,S] fp32 (S a multiple of 32) -> pooled features [B, widths[-1]] fp32 (float64 if x is float64)."""
    depths, widths = CONVNEXT_CFG[arch]
    sd = strip_prefix(sd)
    P = {k: v.to(x.dtype) for k, v in sd.items()}
    h = F.conv2d(x, P["stem.0.weight"], P["stem.0.bias"], stride=4)
    h = _ln_channels_last(h.permute(0, 2, 3, 1), P["stem.1.weight"], P["stem.1.bias"]).permute(0, 3, 1, 2)
    for i, nb in enumerate(depths):
        p = f"stages.{i}."
        if i > 0:
            h = _ln_channels_last(h.permute(0, 2, 3, 1), P[p + "downsample.0.weight"], P[p + "downsample.0.bias"]).permute(0, 3, 1, 2)
            h = F.conv2d(h, P[p + "downsample.1.weight"], P[p + "downsample.1.bias"], stride=2)
        for j in range(nb):
            q = p + f"blocks.{j}."
            y = F.conv2d(h, P[q + "conv_dw.weight"], P[q + "conv_dw.bias"], padding=3, groups=h.shape[1])
            y = _ln_channels_last(y.permute(0, 2, 3, 1), P[q + "norm.weight"], P[q + "norm.bias"])
            y = F.linear(F.gelu(F.linear(y, P[q + "mlp.fc1.weight"], P[q + "mlp.fc1.bias"])), P[q + "mlp.fc2.weight"], P[q + "mlp.fc2.bias"])
            h = h + (y * P[q + "gamma"]).permute(0, 3, 1, 2)
    return _ln_channels_last(h.mean(dim=(2, 3)), P["head.norm.weight"], P["head.norm.bias"])


def hf_state_dict(sd):
    """timm key names -> transformers ConvNextModel key names (the mapping of the issue / DESIGN.md)."""
    out = {}
    for k, v in strip_prefix(sd).items():
        h = k
        h = h.replace("stem.0.", "embeddings.patch_embeddings.").replace("stem.1.", "embeddings.layernorm.")
        if h.startswith("stages."):
            h = "encoder." + h
            h = h.replace(".downsample.0.", ".downsampling_layer.0.").replace(".downsample.1.", ".downsampling_layer.1.")
            h = h.replace(".blocks.", ".layers.").replace(".conv_dw.", ".dwconv.").replace(".norm.", ".layernorm.")
            h = h.replace(".mlp.fc1.", ".pwconv1.").replace(".mlp.fc2.", ".pwconv2.")
            if h.endswith(".gamma"):
                h = h[: -len("gamma")] + "layer_scale_parameter"
        h = h.replace("head.norm.", "layernorm.")
        out[h] = v
    return out
