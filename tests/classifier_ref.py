"""float64 restatement of the FFNN classifier of the reference (models/classifiers.py:35-83: ``timm.create_model(name,
num_classes=N)``): the encoder's embedding before L2 normalisation, then timm's head ``Linear``.  The encoders are the project's CPU
restatements (oracle/encoders_ref.py for ViT and ResNet, tests/convnext_ref.py, tests/mobilenetv3_ref.py), run in float64."""
import torch

from convnext_ref import convnext_forward
from effocr_amd import weights as W
from mobilenetv3_ref import mobilenetv3_forward
from oracle.encoders_ref import resnet_forward, vit_forward


def embedding64(arch, sd, x):
    """x [B,3,S,S] -> [B,D] float64, the head's input."""
    sd64 = {k: v.double() for k, v in W.strip_prefix(sd).items()}
    x = x.double()
    with torch.no_grad():
        if W.is_vit(arch):
            return vit_forward(arch, sd64, x)
        if arch in W.RESNET_CFG:
            return resnet_forward(arch, sd64, x)
        if W.is_convnext(arch):
            return convnext_forward(arch, sd64, x)
        if W.is_mobilenetv3(arch):
            return mobilenetv3_forward(arch, sd64, x)
    raise NotImplementedError(arch)


def logits64(arch, sd, x):
    """-> [B,N] float64 logits of the classifier whose head sd carries."""
    sd = W.strip_prefix(sd)
    wk, bk = W.head_keys(arch)
    return embedding64(arch, sd, x) @ sd[wk].double().T + sd[bk].double()
