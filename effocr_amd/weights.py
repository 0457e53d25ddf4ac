"""Encoder parameter tables, seeded random initialisation and checkpoint I/O.

The reference obtains its encoder from ``timm.create_model(name, num_classes=0)`` and saves /
loads it as a torch state dict whose keys carry a ``net.`` prefix (models/encoders.py:56-70,
train_effocr_recognizer.py:65-72).  This module knows the parameter names and shapes of the three
architectures BASELINE.json names (resnet18, vit_small_patch16_224, vit_base_patch16_224), of resnet34 / resnet50 and of
convnext_tiny (one of the three encoders the reference README recommends for ``--auto_model_timm``)
so that a real ``enc_best.pth`` drops in, and it produces the seeded random-init weights the
benchmark and the tests use (there is no network for checkpoints).

ConvNeXt key names follow timm's ``convnext.py`` (``stem.0`` / ``stem.1``, ``stages.i.downsample.{0,1}``,
``stages.i.blocks.j.{gamma,conv_dw,norm,mlp.fc1,mlp.fc2}``, ``head.norm``).  timm is not a dependency of this
project, so those names could not be checked against timm itself here; the architecture and the parameter
shapes are pinned against ``transformers.ConvNextModel`` by the tests (tests/test_convnext_host.py), the same
caveat that applies to the faiss index layout of knn.py.

MobileNetV3 (``mobilenetv3_small_050`` / ``_075`` / ``_100``, ``mobilenetv3_large_100``) is described by timm's arch-def strings and a channel multiplier
(``mobilenetv3_blocks``), from which the key names and shapes follow (``conv_stem``, ``bn1``,
``blocks.i.j.{conv_pw,bn1,conv_dw,bn2,se.conv_reduce,se.conv_expand,conv_pwl,bn3}``, ``conv_head``); the
builder is pinned by the parameter counts of three widths (tests/test_mobilenetv3_host.py).

EfficientNet-B0 (``efficientnet_b0`` / ``tf_efficientnet_b0``) comes out of the same timm builder: timm ``efficientnet.py``,
``_gen_efficientnet`` at multipliers 1.0 / 1.0 (``efficientnet_blocks``) — a 32-channel stem, squeeze-excite in all 16 blocks at
``round(0.25 x the block's input channels)``, ``conv_head`` (no bias) + ``bn2`` + SiLU before the pool.  The two names share keys and
shapes; the ``tf_`` variant (BN eps 1e-3, TensorFlow SAME padding) cannot be told from a checkpoint and must be named.  The key names
come from timm's source as remembered and are UNVERIFIED against a timm install; the architecture is pinned against
``transformers.EfficientNetModel`` (tests/test_efficientnet_host.py).

Swin-T (``swin_tiny_patch4_window7_224``) key names follow timm's ``swin_transformer.py`` as of timm 0.9
(``patch_embed.proj`` / ``patch_embed.norm``, ``layers.i.blocks.j.{norm1,attn.relative_position_bias_table,attn.qkv,attn.proj,
norm2,mlp.fc1,mlp.fc2}``, the patch merging ``layers.i.downsample.{norm,reduction}`` at the START of stages 1-3, ``norm``, classifier
``head.fc``).  Checkpoints of timm < 0.9 (patch merging at the END of stages 0-2, classifier ``head``) are renamed to that layout by
``strip_prefix``, and the derived buffers ``relative_position_index`` / ``attn_mask`` are dropped.  timm is not installed here either:
the names could not be checked against timm itself; the architecture and the shapes are pinned against ``transformers.SwinModel``
(tests/test_swin_host.py).

BEiT (``beit_base_patch16_224`` / ``beitv2_base_patch16_224``) key names follow timm's ``beit.py`` as remembered (``cls_token``,
``patch_embed.proj``, ``blocks.i.{gamma_1,gamma_2,norm1,attn.q_bias,attn.v_bias,attn.relative_position_bias_table,attn.qkv.weight,
attn.proj,norm2,mlp.fc1,mlp.fc2}``, ``fc_norm``, classifier ``head``; no ``pos_embed`` and no ``attn.qkv.bias``) and are UNVERIFIED
against a timm install.  The two names are the same module (they differ in their pre-training), so a checkpoint cannot tell them apart
and ``infer_arch`` answers ``beit_base_patch16_224``.  The buffers ``attn.relative_position_index`` and ``attn.k_bias`` of older timm
checkpoints are dropped by ``strip_prefix``.  The architecture and the shapes are pinned against ``transformers.BeitModel``
(tests/test_beit_host.py).

BiT ResNetV2 (``resnetv2_50x1_bitm`` / ``resnetv2_101x1_bitm``; timm >= 0.9 calls the same modules ``resnetv2_50x1_bit`` / ``resnetv2_101x1_bit``)
key names follow timm's ``resnetv2.py`` as remembered (``stem.conv``, ``stages.i.blocks.j.{downsample.conv,norm1,conv1,norm2,conv2,norm3,
conv3}``, ``norm``, classifier ``head.fc`` — a 1x1 convolution, weight [N, 2048, 1, 1]) and are UNVERIFIED against a timm install.  Every
convolution is weight-standardised and has no bias, every norm is GroupNorm(32) + ReLU.  The ``_bitm`` and ``_bit`` names share keys and
shapes, so ``infer_arch`` answers the ``_bitm`` name.  The architecture and the parameter counts are pinned against
``transformers.BitModel`` (tests/test_bit_host.py).

Patch-8 ViTs (``vit_small_patch8_224`` / ``vit_base_patch8_224``) use the key names of timm's ``vision_transformer.py`` that the patch-16
ViTs above already use (``cls_token``, ``pos_embed``, ``patch_embed.proj``, ``blocks.i.{norm1,attn.qkv,attn.proj,norm2,mlp.fc1,mlp.fc2}``,
``norm``, classifier ``head``); only ``patch_embed.proj.weight`` is [D, 3, 8, 8] and ``pos_embed`` has (img_size / 8)^2 + 1 rows.  They
could not be checked against a timm install either; the architecture and the parameter counts are pinned against
``transformers.ViTModel(patch_size=8)`` (tests/test_vit8_host.py).  ``infer_arch`` tells patch 8 from patch 16 by the kernel size of
``patch_embed.proj.weight``.
"""
from collections import OrderedDict
import math
import re
import torch

VIT_CFG = {
    # name: (embed_dim, depth, heads, mlp_ratio)
    "vit_small_patch16_224": (384, 12, 6, 4),
    "vit_base_patch16_224": (768, 12, 12, 4),
    "vit_tiny_test": (128, 2, 2, 4),          # miniature used only by fast tests
}
RESNET_CFG = {
    # name: (depths, widths, block) — timm resnet.py: "basic" = BasicBlock (two 3x3 convs), "bottleneck" = Bottleneck (1x1, 3x3 with the
    # stride, 1x1 to 4 x width); 7x7/2 stem + 3x3/2 max pool, a 1x1 stride-s conv + BN shortcut where the shape changes, BN eps 1e-5
    "resnet18": ((2, 2, 2, 2), (64, 128, 256, 512), "basic"),
    "resnet34": ((3, 4, 6, 3), (64, 128, 256, 512), "basic"),
    "resnet50": ((3, 4, 6, 3), (64, 128, 256, 512), "bottleneck"),
}
CONVNEXT_CFG = {
    # name: (depths, widths) — timm convnext.py; convnext_small would be ((3, 3, 27, 3), (96, 192, 384, 768))
    "convnext_tiny": ((3, 3, 9, 3), (96, 192, 384, 768)),
}
MOBILENETV3_CFG = {
    # name: channel multiplier — timm mobilenetv3.py _gen_mobilenet_v3; _050 runs on libeffocr_hip.so (LDS-resident kernels), the other
    # three on libeffocr_mnv3.so (is_mnv3_lib)
    "mobilenetv3_small_050": 0.5,
    "mobilenetv3_small_075": 0.75,
    "mobilenetv3_small_100": 1.0,
    "mobilenetv3_large_100": 1.0,
}
MOBILENETV3_ARCH_DEF = (
    # timm's arch-def strings for MobileNetV3-Small: one list per stage; "nre" = ReLU, otherwise hard-swish
    ("ds_r1_k3_s2_e1_c16_se0.25_nre",),
    ("ir_r1_k3_s2_e4.5_c24_nre", "ir_r1_k3_s1_e3.67_c24_nre"),
    ("ir_r1_k5_s2_e4_c40_se0.25", "ir_r2_k5_s1_e6_c40_se0.25"),
    ("ir_r2_k5_s1_e3_c48_se0.25",),
    ("ir_r3_k5_s2_e6_c96_se0.25",),
    ("cn_r1_k1_s1_c576",),
)
MOBILENETV3_LARGE_ARCH_DEF = (
    # timm's arch-def strings for MobileNetV3-Large (_gen_mobilenet_v3, the non-small branch)
    ("ds_r1_k3_s1_e1_c16_nre",),
    ("ir_r1_k3_s2_e4_c24_nre", "ir_r1_k3_s1_e3_c24_nre"),
    ("ir_r3_k5_s2_e3_c40_se0.25_nre",),
    ("ir_r1_k3_s2_e6_c80", "ir_r1_k3_s1_e2.5_c80", "ir_r2_k3_s1_e2.3_c80"),
    ("ir_r2_k3_s1_e6_c112_se0.25",),
    ("ir_r3_k5_s2_e6_c160_se0.25",),
    ("cn_r1_k1_s1_c960",),
)
EFFICIENTNET_CFG = {
    # name: (BN eps, TensorFlow SAME padding) — timm efficientnet.py _gen_efficientnet(channel_multiplier=1.0, depth_multiplier=1.0); both
    # run on libeffocr_effnet.so.  b1-b7, efficientnet_lite*, efficientnetv2_* and the _ns / _ap weight tags are not supported.
    "efficientnet_b0": (1e-5, False),
    "tf_efficientnet_b0": (1e-3, True),
}
EFFICIENTNET_ARCH_DEF = (
    # timm's arch-def strings for EfficientNet-B0: every block SiLU, squeeze-excite 0.25 of the block's INPUT channels
    ("ds_r1_k3_s1_e1_c16_se0.25",),
    ("ir_r2_k3_s2_e6_c24_se0.25",),
    ("ir_r2_k5_s2_e6_c40_se0.25",),
    ("ir_r3_k3_s2_e6_c80_se0.25",),
    ("ir_r3_k5_s1_e6_c112_se0.25",),
    ("ir_r4_k5_s2_e6_c192_se0.25",),
    ("ir_r1_k3_s1_e6_c320_se0.25",),
)
EFFICIENTNET_STEM = 32
EFFICIENTNET_FEATURES = 1280          # conv_head width of EfficientNet-B0
SWIN_CFG = {
    # name: (embed_dim, depths, heads, window) — timm swin_transformer.py; head dim 32 in every stage, mlp ratio 4, patch 4
    "swin_tiny_patch4_window7_224": (96, (2, 2, 6, 2), (3, 6, 12, 24), 7),
}
BEIT_CFG = {
    # name: (embed_dim, depth, heads, mlp_ratio) — timm beit.py; patch 16, head dim 64, LayerNorm eps 1e-6, layer scale, a relative-position
    # bias table per block, no absolute position embedding; the pooled output is fc_norm(mean of the patch tokens)
    "beit_base_patch16_224": (768, 12, 12, 4),
    "beitv2_base_patch16_224": (768, 12, 12, 4),
    "beit_tiny_test": (128, 2, 2, 4),         # miniature used only by fast tests
}
BIT_CFG = {
    # name: depths — timm resnetv2.py, PreActBottleneck, width factor 1: mid widths 64-128-256-512 (x4 out), GroupNorm(32, eps 1e-5) + ReLU
    # before each weight-standardised conv, a final norm; the _bit names are timm >= 0.9's for the same modules
    "resnetv2_50x1_bitm": (3, 4, 6, 3),
    "resnetv2_50x1_bit": (3, 4, 6, 3),
    "resnetv2_101x1_bitm": (3, 4, 23, 3),
    "resnetv2_101x1_bit": (3, 4, 23, 3),
}
BIT_WIDTHS = (64, 128, 256, 512)      # bottleneck widths per stage
BIT_FEATURES = 2048
VIT8_CFG = {
    # name: (embed_dim, depth, heads, mlp_ratio) — timm vision_transformer.py with patch_size 8 (vit_small_patch8_224 carries the DINO
    # ViT-S/8 weights); the same pre-norm blocks as VIT_CFG's, 785 tokens per 224^2 crop; they run on libeffocr_vit8.so
    "vit_small_patch8_224": (384, 12, 6, 4),
    "vit_base_patch8_224": (768, 12, 12, 4),
    "vit8_tiny_test": (128, 2, 2, 4),         # miniature used only by fast tests
}
VIT8_PATCH = 8
LEVIT_CFG = {
    # name: (widths, key_dim, heads, depths) — timm levit.py (the linear-token models): a four-convolution stem to img/16 tokens per side,
    # three stages of attention + MLP blocks (mlp ratio 2, value width 2 x key_dim, BatchNorm after every linear, hardswish), between them
    # a down-sampling attention (width / key_dim heads, value width 4 x key_dim, queries at the even rows and columns) + MLP; the pooled
    # output is the mean of the final tokens; they run on libeffocr_levit.so.  levit_conv_*, levit_384_s8 and levit_512* are not supported.
    "levit_128s": ((128, 256, 384), 16, (4, 6, 8), (2, 3, 4)),
    "levit_128": ((128, 256, 384), 16, (4, 8, 12), (4, 4, 4)),
    "levit_192": ((192, 288, 384), 32, (3, 5, 6), (4, 4, 4)),
    "levit_256": ((256, 384, 512), 32, (4, 6, 8), (4, 4, 4)),
    "levit_384": ((384, 512, 768), 32, (6, 9, 12), (4, 4, 4)),
    "levit_tiny_test": ((128, 128, 128), 16, (2, 2, 4), (1, 1, 1)),       # miniatures used only by fast tests: key_dim 16 ...
    "levit_tiny32_test": ((128, 192, 256), 32, (1, 3, 2), (1, 1, 1)),     # ... and key_dim 32 with a width that is no multiple of 128
}
LEVIT_SUPPORTED = ("levit_128s", "levit_128", "levit_192", "levit_256", "levit_384")
LEVIT_BN_EPS = 1e-5
REGNET_CFG = {
    # name: (w0, wa, wm, depth, group width, squeeze-excite) — timm regnet.py (the key names and this restatement are written from memory
    # of that file, not verified against a timm install; the parameter counts equal timm's published ones): a 3x3/2 stem to 32 channels,
    # four stages whose first block has stride 2, bottleneck ratio 1, a grouped 3x3 in every block; RegNetY adds squeeze-excite of width
    # round(0.25 x the block's input width).  regnet_widths derives the stage widths and depths.  They run on libeffocr_regnet.so.
    # regnetx_032 / regnety_032 and wider, regnetz_* and regnetv_* are not supported.
    "regnetx_002": (24, 36.44, 2.49, 13, 8, False),
    "regnetx_004": (24, 24.48, 2.54, 22, 16, False),
    "regnetx_006": (48, 36.97, 2.24, 16, 24, False),
    "regnetx_008": (56, 35.73, 2.28, 16, 16, False),
    "regnetx_016": (80, 34.01, 2.25, 18, 24, False),
    "regnety_002": (24, 36.44, 2.49, 13, 8, True),
    "regnety_004": (48, 27.89, 2.09, 16, 8, True),
    "regnety_006": (48, 32.54, 2.32, 15, 16, True),
    "regnety_008": (56, 38.84, 2.40, 14, 16, True),
    "regnety_016": (48, 20.71, 2.65, 27, 24, True),
}
REGNET_SUPPORTED = tuple(REGNET_CFG)
REGNET_MINI = {
    # miniatures used only by fast tests: (stage widths, depths, group width, squeeze-excite) given directly
    "regnetx_mini8_test": ((8, 24, 40, 56), (1, 1, 2, 1), 8, False),
    "regnetx_mini16_test": ((16, 32, 48, 80), (1, 1, 2, 1), 16, False),
    "regnety_mini24_test": ((24, 48, 72, 120), (1, 1, 2, 1), 24, True),
}
REGNET_STEM = 32
REGNET_BN_EPS = 1e-5
PVT_CFG = {
    # name: (stage widths, heads, depths, mlp ratios) — timm pvt_v2.py (the key names are written from memory of that file, not verified
    # against a timm install; the architecture and the parameter counts are pinned to transformers.PvtV2Model): four stages, each an
    # overlapping patch embedding (7x7/4 on the crop, then 3x3/2) + LayerNorm, pre-norm blocks whose keys and values come from a
    # stride-sr convolution + LayerNorm of the tokens (sr = 8, 4, 2, 1) and whose MLP has a depthwise 3x3 + GELU, and a LayerNorm; the
    # embedding is the mean of the last stage's tokens.  They run on libeffocr_pvt.so.  pvt_v2_b2_li and PVT v1 are not supported.
    "pvt_v2_b0": ((32, 64, 160, 256), (1, 2, 5, 8), (2, 2, 2, 2), (8, 8, 4, 4)),
    "pvt_v2_b1": ((64, 128, 320, 512), (1, 2, 5, 8), (2, 2, 2, 2), (8, 8, 4, 4)),
    "pvt_v2_b2": ((64, 128, 320, 512), (1, 2, 5, 8), (3, 4, 6, 3), (8, 8, 4, 4)),
    "pvt_v2_b3": ((64, 128, 320, 512), (1, 2, 5, 8), (3, 4, 18, 3), (8, 8, 4, 4)),
    "pvt_v2_b4": ((64, 128, 320, 512), (1, 2, 5, 8), (3, 8, 27, 3), (8, 8, 4, 4)),
    "pvt_v2_b5": ((64, 128, 320, 512), (1, 2, 5, 8), (3, 6, 40, 3), (4, 4, 4, 4)),
    "pvt_v2_mini32_test": ((32, 64, 96, 128), (1, 2, 3, 4), (1, 1, 1, 1), (8, 8, 4, 4)),     # miniatures used only by fast tests: head width 32 ...
    "pvt_v2_mini64_test": ((64, 128, 192, 256), (1, 2, 3, 4), (1, 1, 2, 1), (8, 8, 4, 4)),   # ... and 64
}
PVT_SUPPORTED = ("pvt_v2_b0", "pvt_v2_b1", "pvt_v2_b2", "pvt_v2_b3", "pvt_v2_b4", "pvt_v2_b5")
PVT_SR = (8, 4, 2, 1)                 # spatial-reduction ratio per stage
PVT_EPS = 1e-6
MOBILENETV3_FEATURES = 1024           # conv_head width of MobileNetV3-Small (not scaled by the multiplier)
MOBILENETV3_LARGE_FEATURES = 1280     # ... and of MobileNetV3-Large
PATCH = 16


def make_divisible(v, divisor=8, min_value=None, round_limit=0.9):
    """timm layers/helpers.py make_divisible."""
    min_value = min_value or divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < round_limit * v:
        new_v += divisor
    return new_v


def _parse_block_def(bs):
    """One timm arch-def string, e.g. "ir_r2_k5_s1_e6_c40_se0.25_nre" -> ("ir", {"r": "2", "k": "5", ..., "nre": ""})."""
    ops = bs.split("_")
    opt = {}
    for o in ops[1:]:
        m = re.match(r"([a-z]+)([0-9.]*)$", o)
        opt[m.group(1)] = m.group(2)
    return ops[0], opt


def mobilenetv3_blocks(arch):
    """(stem channels, [block dicts], head width) of a MobileNetV3 (Small or Large, chosen by name), built from MOBILENETV3_ARCH_DEF /
    MOBILENETV3_LARGE_ARCH_DEF the way timm's _efficientnet_builder does.  A block dict has: key (e.g. "blocks.2.1"), type ("ds" | "ir" | "cn"), cin, mid, cout, k, stride,
    se (SE width, 0 = none), hs (hard-swish, else ReLU), res (residual)."""
    mult = MOBILENETV3_CFG[arch]
    large = is_mobilenetv3_large(arch)
    stem = 16 if mult < 0.75 else make_divisible(16 * mult)   # fix_stem = multiplier < 0.75
    blocks, cin = [], stem
    for si, stage in enumerate(MOBILENETV3_LARGE_ARCH_DEF if large else MOBILENETV3_ARCH_DEF):
        bi = 0
        for bs in stage:
            kind, opt = _parse_block_def(bs)
            for r in range(int(opt["r"])):
                cout = make_divisible(int(opt["c"]) * mult)
                stride = int(opt["s"]) if r == 0 else 1
                k = int(opt["k"])
                if kind == "ds":
                    mid = cin
                elif kind == "ir":
                    mid = make_divisible(cin * float(opt["e"]))
                else:
                    mid = cout
                se = make_divisible(mid * float(opt["se"])) if "se" in opt else 0
                blocks.append(dict(key=f"blocks.{si}.{bi}", type=kind, cin=cin, mid=mid, cout=cout, k=k, stride=stride, se=se,
                                   hs="nre" not in opt, res=(kind != "cn" and stride == 1 and cin == cout)))
                cin = cout
                bi += 1
    return stem, blocks, MOBILENETV3_LARGE_FEATURES if large else MOBILENETV3_FEATURES


def efficientnet_blocks(arch):
    """(stem channels, [block dicts], head width) of an EfficientNet-B0, built from EFFICIENTNET_ARCH_DEF the way timm's
    _efficientnet_builder does at multipliers 1.0 / 1.0.  A block dict has the keys of mobilenetv3_blocks' (hs is False: every activation
    is SiLU); it differs in the squeeze-excite width, ``round(cin x ratio)`` of the block's INPUT channels without make_divisible, and in
    having no "cn" stage."""
    if arch not in EFFICIENTNET_CFG:
        raise NotImplementedError(f"unsupported encoder architecture {arch!r}")
    blocks, cin = [], EFFICIENTNET_STEM
    for si, stage in enumerate(EFFICIENTNET_ARCH_DEF):
        bi = 0
        for bs in stage:
            kind, opt = _parse_block_def(bs)
            for r in range(int(opt["r"])):
                cout = make_divisible(int(opt["c"]))
                stride = int(opt["s"]) if r == 0 else 1
                mid = cin if kind == "ds" else make_divisible(cin * float(opt["e"]))
                blocks.append(dict(key=f"blocks.{si}.{bi}", type=kind, cin=cin, mid=mid, cout=cout, k=int(opt["k"]), stride=stride,
                                   se=int(round(cin * float(opt["se"]))), hs=False, res=(stride == 1 and cin == cout)))
                cin = cout
                bi += 1
    return EFFICIENTNET_STEM, blocks, EFFICIENTNET_FEATURES


def is_efficientnet(arch):
    """efficientnet_b0 / tf_efficientnet_b0: the encoders that run on libeffocr_effnet.so."""
    return arch in EFFICIENTNET_CFG


def is_mobilenetv3(arch):
    return arch in MOBILENETV3_CFG


def is_mobilenetv3_large(arch):
    return arch in MOBILENETV3_CFG and arch.startswith("mobilenetv3_large_")


def is_mnv3_lib(arch):
    """The MobileNetV3s that run on libeffocr_mnv3.so (activations in HBM between blocks): every one but mobilenetv3_small_050, which
    keeps its LDS-resident kernels in libeffocr_hip.so."""
    return arch in MOBILENETV3_CFG and arch != "mobilenetv3_small_050"


def is_vit(arch):
    return arch in VIT_CFG


def embed_dim(arch):
    if arch in VIT_CFG:
        return VIT_CFG[arch][0]
    if arch in RESNET_CFG:
        return RESNET_CFG[arch][1][-1] * resnet_expansion(arch)
    if arch in CONVNEXT_CFG:
        return CONVNEXT_CFG[arch][1][-1]
    if arch in MOBILENETV3_CFG:
        return MOBILENETV3_LARGE_FEATURES if is_mobilenetv3_large(arch) else MOBILENETV3_FEATURES
    if arch in SWIN_CFG:
        return SWIN_CFG[arch][0] * 8
    if arch in EFFICIENTNET_CFG:
        return EFFICIENTNET_FEATURES
    if arch in BEIT_CFG:
        return BEIT_CFG[arch][0]
    if arch in BIT_CFG:
        return BIT_FEATURES
    if arch in VIT8_CFG:
        return VIT8_CFG[arch][0]
    if arch in LEVIT_CFG:
        return LEVIT_CFG[arch][0][-1]
    if is_regnet(arch):
        return regnet_arch(arch)[0][-1]
    if arch in PVT_CFG:
        return PVT_CFG[arch][0][-1]
    _refuse_levit(arch)
    _refuse_regnet(arch)
    _refuse_pvt(arch)
    raise NotImplementedError(f"unsupported encoder architecture {arch!r}")


def _refuse_levit(arch):
    """A LeViT name this package does not build: NotImplementedError that lists the ones it does."""
    if isinstance(arch, str) and arch.startswith("levit"):
        raise NotImplementedError(f"unsupported LeViT {arch!r} (supported: {', '.join(LEVIT_SUPPORTED)}; levit_conv_*, levit_384_s8 and "
                                  "levit_512* are not)")


def _refuse_pvt(arch):
    """A PVT name this package does not build: NotImplementedError that lists the ones it does."""
    if isinstance(arch, str) and arch.startswith("pvt"):
        raise NotImplementedError(f"unsupported PVT {arch!r} (supported: {', '.join(PVT_SUPPORTED)}; pvt_v2_b2_li and PVT v1 are not)")


def is_pvt(arch):
    """pvt_v2_b0 ... pvt_v2_b5 (and the two miniatures): the encoders that run on libeffocr_pvt.so."""
    return arch in PVT_CFG


def is_levit(arch):
    """levit_128s / levit_128 / levit_192 / levit_256 / levit_384 (and the two miniatures): the encoders that run on libeffocr_levit.so."""
    return arch in LEVIT_CFG


def is_regnet(arch):
    """regnetx_002 ... regnety_016 (and the three miniatures): the encoders that run on libeffocr_regnet.so."""
    return arch in REGNET_CFG or arch in REGNET_MINI


def _refuse_regnet(arch):
    """A RegNet name this package does not build: NotImplementedError that lists the ones it does."""
    if isinstance(arch, str) and arch.startswith("regnet"):
        raise NotImplementedError(f"unsupported RegNet {arch!r} (supported: {', '.join(REGNET_SUPPORTED)}; regnetx_032 / regnety_032 and "
                                  "wider, regnetz_* and regnetv_* are not)")


def regnet_widths(w0, wa, wm, depth, group_width, q=8):
    """timm regnet.py's width generation: u_j = w0 + wa j, k_j = round(log(u_j / w0) / log(wm)), w_j = round(w0 wm^k_j / q) q; runs of
    equal widths are the stages; then every width becomes a multiple of its group width g = min(group_width, w) (bottleneck ratio 1).
    Returns (stage widths, stage depths)."""
    per_block = []
    for j in range(depth):
        k = round(math.log((w0 + wa * j) / w0) / math.log(wm))
        per_block.append(int(round(w0 * wm ** k / q) * q))
    widths, depths = [], []
    for w in per_block:
        if widths and widths[-1] == w:
            depths[-1] += 1
        else:
            widths.append(w)
            depths.append(1)
    out = []
    for w in widths:
        g = min(group_width, w)
        out.append(int(round(w / g) * g))
    return tuple(out), tuple(depths)


def regnet_arch(arch):
    """(stage widths, stage depths, group width, squeeze-excite) of a RegNet name."""
    if arch in REGNET_MINI:
        return REGNET_MINI[arch]
    w0, wa, wm, depth, gw, se = REGNET_CFG[arch]
    widths, depths = regnet_widths(w0, wa, wm, depth, gw)
    return widths, depths, gw, se


def regnet_blocks(arch):
    """The block list of a RegNet: dicts with key ("s1.b1"), cin, w, stride (2 in the first block of EVERY stage), gw, se (reduced width
    round(0.25 x the block's INPUT width), 0 for RegNetX) and down (a downsample shortcut: the first block of each stage)."""
    widths, depths, gw, se = regnet_arch(arch)
    blocks, cin = [], REGNET_STEM
    for si, (w, d) in enumerate(zip(widths, depths), start=1):
        for bi in range(1, d + 1):
            stride = 2 if bi == 1 else 1
            blocks.append(dict(key=f"s{si}.b{bi}", cin=cin, w=w, stride=stride, gw=gw, se=int(round(cin * 0.25)) if se else 0,
                               down=(stride != 1 or cin != w)))
            cin = w
    return blocks


def levit_sub(R):
    """Token grid per side after a stride-2 sub-sampling of the tokens at even rows and columns."""
    return (R - 1) // 2 + 1


def is_swin(arch):
    return arch in SWIN_CFG


def is_beit(arch):
    """beit_base_patch16_224 / beitv2_base_patch16_224 (and the miniature beit_tiny_test): the encoders that run on libeffocr_beit.so."""
    return arch in BEIT_CFG


def is_bit(arch):
    """resnetv2_50x1_bitm / resnetv2_101x1_bitm (and their timm >= 0.9 names): the encoders that run on libeffocr_bit.so."""
    return arch in BIT_CFG


def is_vit8(arch):
    """vit_small_patch8_224 / vit_base_patch8_224 (and the miniature vit8_tiny_test): the encoders that run on libeffocr_vit8.so.
    ``is_vit`` stays False for them: nothing routes them to the product library."""
    return arch in VIT8_CFG


def beit_relative_position_index(W):
    """[T, T] int64 index into a BEiT bias table of (2W-1)^2 + 3 rows for a W x W patch grid, T = W^2 + 1 tokens (token 0 = cls, token
    1 + y W + x = patch (y, x)); entry [i, j] belongs to query i and key j.  Patch pairs: (y_i - y_j + W-1)(2W-1) + (x_i - x_j + W-1);
    row 0 (cls -> any): (2W-1)^2; column 0 (any -> cls): (2W-1)^2 + 1; [0, 0]: (2W-1)^2 + 2."""
    n = (2 * W - 1) ** 2
    yy, xx = torch.meshgrid(torch.arange(W), torch.arange(W), indexing="ij")
    y, x = yy.flatten(), xx.flatten()
    idx = torch.empty(W * W + 1, W * W + 1, dtype=torch.long)
    idx[1:, 1:] = (y[:, None] - y[None, :] + W - 1) * (2 * W - 1) + (x[:, None] - x[None, :] + W - 1)
    idx[0, :] = n
    idx[:, 0] = n + 1
    idx[0, 0] = n + 2
    return idx


def resnet_expansion(arch):
    """Output channels of a residual block per unit of its width: 4 for timm's Bottleneck, 1 for BasicBlock."""
    return 4 if RESNET_CFG[arch][2] == "bottleneck" else 1


def is_resnet_lib(arch):
    """resnet34 / resnet50: the ResNets that run on libeffocr_resnet.so (16-bit convolutions); resnet18 runs on libeffocr_hip.so."""
    return arch in RESNET_CFG and arch != "resnet18"


def is_convnext(arch):
    return arch in CONVNEXT_CFG


# timm's classifier head per family: (weight key, bias key) of the nn.Linear that ``timm.create_model(name, num_classes=N)`` appends
# (models/classifiers.py:35-83).  Its input is the encoder's embedding before L2 normalisation (HipEncoder.forward(x, normalize=False)):
# resnet18 the global-pooled features, ViT norm(x)[:, 0] (fc_norm is Identity for token pooling), convnext_tiny the output of head.norm,
# mobilenetv3 conv_head + hard-swish.
# efficientnet_b0 / tf_efficientnet_b0: the global average pool of SiLU(bn2(conv_head)).
# swin_tiny_patch4_window7_224: the mean of the final norm's tokens (timm >= 0.9 names the head head.fc; strip_prefix renames timm < 0.9's head).
# beit_base_patch16_224 / beitv2_base_patch16_224: fc_norm of the mean of the patch tokens.
# vit_small_patch8_224 / vit_base_patch8_224: norm(x)[:, 0], as the patch-16 ViTs.
# resnetv2_*_bitm: the global average pool of relu(norm(x)); the head is a 1x1 convolution, its weight [N, 2048, 1, 1] (head_shapes).
HEAD_KEYS = {"resnet": ("fc.weight", "fc.bias"), "vit": ("head.weight", "head.bias"),
             "convnext": ("head.fc.weight", "head.fc.bias"), "mobilenetv3": ("classifier.weight", "classifier.bias"),
             "swin": ("head.fc.weight", "head.fc.bias"), "efficientnet": ("classifier.weight", "classifier.bias"),
             "beit": ("head.weight", "head.bias"), "bit": ("head.fc.weight", "head.fc.bias"),
             "vit8": ("head.weight", "head.bias"),
             # LeViT: two BatchNorm1d + Linear heads (head, head_dist) whose logits timm averages; these are the first head's linear
             # (head_shapes lists all twelve keys, levit_fold_heads folds them into one matrix)
             "levit": ("head.linear.weight", "head.linear.bias"),
             # regnetx_* / regnety_*: the global average pool of the last block (final_conv is the identity)
             "regnet": ("head.fc.weight", "head.fc.bias"),
             # pvt_v2_*: the mean of the last stage's normalised tokens
             "pvt": ("head.weight", "head.bias")}


def _family(arch):
    if arch in VIT_CFG:
        return "vit"
    if arch in RESNET_CFG:
        return "resnet"
    if arch in CONVNEXT_CFG:
        return "convnext"
    if arch in MOBILENETV3_CFG:
        return "mobilenetv3"
    if arch in SWIN_CFG:
        return "swin"
    if arch in EFFICIENTNET_CFG:
        return "efficientnet"
    if arch in BEIT_CFG:
        return "beit"
    if arch in BIT_CFG:
        return "bit"
    if arch in VIT8_CFG:
        return "vit8"
    if arch in LEVIT_CFG:
        return "levit"
    if is_regnet(arch):
        return "regnet"
    if arch in PVT_CFG:
        return "pvt"
    _refuse_levit(arch)
    _refuse_regnet(arch)
    _refuse_pvt(arch)
    raise NotImplementedError(f"unsupported encoder architecture {arch!r}")


def head_keys(arch):
    """(weight key, bias key) of ``arch``'s timm classifier head."""
    return HEAD_KEYS[_family(arch)]


def head_shapes(arch, num_classes):
    """Ordered {timm key: shape} of the classifier head: weight [num_classes, embed_dim] ([num_classes, embed_dim, 1, 1] for BiT, whose
    head is a 1x1 convolution), bias [num_classes] (empty for 0)."""
    s = OrderedDict()
    if num_classes:
        if num_classes < 0:
            raise ValueError(f"num_classes must be >= 0, got {num_classes}")
        if arch in LEVIT_CFG:
            D = embed_dim(arch)
            for h in ("head", "head_dist"):
                for leaf in ("weight", "bias", "running_mean", "running_var"):
                    s[f"{h}.bn.{leaf}"] = (D,)
                s[f"{h}.linear.weight"] = (int(num_classes), D)
                s[f"{h}.linear.bias"] = (int(num_classes),)
            return s
        wk, bk = head_keys(arch)
        s[wk] = (int(num_classes), embed_dim(arch)) + ((1, 1) if arch in BIT_CFG else ())
        s[bk] = (int(num_classes),)
    return s


def param_shapes(arch, img_size=224, num_classes=0):
    """Ordered {timm key: shape} for ``arch`` (buffers such as BN running stats included); with ``num_classes`` > 0 timm's classifier
    head comes last, as in timm's state dict."""
    if num_classes:
        s = param_shapes(arch, img_size)
        s.update(head_shapes(arch, num_classes))
        return s
    s = OrderedDict()
    if arch in VIT_CFG:
        D, depth, heads, r = VIT_CFG[arch]
        ntok = (img_size // PATCH) ** 2 + 1
        s["cls_token"] = (1, 1, D)
        s["pos_embed"] = (1, ntok, D)
        s["patch_embed.proj.weight"] = (D, 3, PATCH, PATCH)
        s["patch_embed.proj.bias"] = (D,)
        for i in range(depth):
            p = f"blocks.{i}."
            s[p + "norm1.weight"] = (D,)
            s[p + "norm1.bias"] = (D,)
            s[p + "attn.qkv.weight"] = (3 * D, D)
            s[p + "attn.qkv.bias"] = (3 * D,)
            s[p + "attn.proj.weight"] = (D, D)
            s[p + "attn.proj.bias"] = (D,)
            s[p + "norm2.weight"] = (D,)
            s[p + "norm2.bias"] = (D,)
            s[p + "mlp.fc1.weight"] = (r * D, D)
            s[p + "mlp.fc1.bias"] = (r * D,)
            s[p + "mlp.fc2.weight"] = (D, r * D)
            s[p + "mlp.fc2.bias"] = (D,)
        s["norm.weight"] = (D,)
        s["norm.bias"] = (D,)
        return s
    if arch in RESNET_CFG:
        depths, widths, block = RESNET_CFG[arch]
        exp = resnet_expansion(arch)

        def bn(p, c):
            s[p + ".weight"] = (c,)
            s[p + ".bias"] = (c,)
            s[p + ".running_mean"] = (c,)
            s[p + ".running_var"] = (c,)

        s["conv1.weight"] = (64, 3, 7, 7)
        bn("bn1", 64)
        cin = 64
        for li, (nb, w) in enumerate(zip(depths, widths), start=1):
            for bi in range(nb):
                p = f"layer{li}.{bi}."
                stride = 2 if (bi == 0 and li > 1) else 1
                if block == "bottleneck":
                    s[p + "conv1.weight"] = (w, cin, 1, 1)
                    bn(p + "bn1", w)
                    s[p + "conv2.weight"] = (w, w, 3, 3)
                    bn(p + "bn2", w)
                    s[p + "conv3.weight"] = (w * exp, w, 1, 1)
                    bn(p + "bn3", w * exp)
                else:
                    s[p + "conv1.weight"] = (w, cin, 3, 3)
                    bn(p + "bn1", w)
                    s[p + "conv2.weight"] = (w, w, 3, 3)
                    bn(p + "bn2", w)
                if bi == 0 and (stride != 1 or cin != w * exp):
                    s[p + "downsample.0.weight"] = (w * exp, cin, 1, 1)
                    bn(p + "downsample.1", w * exp)
                cin = w * exp
        return s
    if arch in CONVNEXT_CFG:
        depths, widths = CONVNEXT_CFG[arch]
        s["stem.0.weight"] = (widths[0], 3, 4, 4)
        s["stem.0.bias"] = (widths[0],)
        s["stem.1.weight"] = (widths[0],)             # LayerNorm over channels
        s["stem.1.bias"] = (widths[0],)
        for i, (nb, c) in enumerate(zip(depths, widths)):
            p = f"stages.{i}."
            if i > 0:
                cp = widths[i - 1]
                s[p + "downsample.0.weight"] = (cp,)  # LayerNorm over channels
                s[p + "downsample.0.bias"] = (cp,)
                s[p + "downsample.1.weight"] = (c, cp, 2, 2)
                s[p + "downsample.1.bias"] = (c,)
            for j in range(nb):
                q = p + f"blocks.{j}."
                s[q + "gamma"] = (c,)                 # (a module's own parameters come before its children's in timm's state dict)
                s[q + "conv_dw.weight"] = (c, 1, 7, 7)
                s[q + "conv_dw.bias"] = (c,)
                s[q + "norm.weight"] = (c,)
                s[q + "norm.bias"] = (c,)
                s[q + "mlp.fc1.weight"] = (4 * c, c)
                s[q + "mlp.fc1.bias"] = (4 * c,)
                s[q + "mlp.fc2.weight"] = (c, 4 * c)
                s[q + "mlp.fc2.bias"] = (c,)
        s["head.norm.weight"] = (widths[-1],)
        s["head.norm.bias"] = (widths[-1],)
        return s
    if arch in MOBILENETV3_CFG:
        return _mobilenetv3_shapes(arch)
    if arch in SWIN_CFG:
        return _swin_shapes(arch)
    if arch in EFFICIENTNET_CFG:
        return _efficientnet_shapes(arch)
    if arch in BEIT_CFG:
        return _beit_shapes(arch, img_size)
    if arch in BIT_CFG:
        return _bit_shapes(arch)
    if arch in VIT8_CFG:
        return _vit8_shapes(arch, img_size)
    if arch in LEVIT_CFG:
        return _levit_shapes(arch, img_size)
    if is_regnet(arch):
        return _regnet_shapes(arch)
    if arch in PVT_CFG:
        return _pvt_shapes(arch)
    _refuse_levit(arch)
    _refuse_regnet(arch)
    _refuse_pvt(arch)
    raise NotImplementedError(f"unsupported encoder architecture {arch!r}")


def _pvt_shapes(arch):
    """timm's state-dict order for a PyramidVisionTransformerV2 (pvt_v2.py; the key names are written from memory of that file, not
    verified against a timm install): the stem's patch embedding, then per stage its downsample (stages 1 to 3), its blocks and its
    norm.  Stage 3 has no attn.sr / attn.norm (reduction ratio 1).  The shapes do not depend on the crop size."""
    widths, heads, depths, ratios = PVT_CFG[arch]
    s = OrderedDict()

    def wb(p, *shape):
        s[p + ".weight"] = tuple(shape)
        s[p + ".bias"] = (shape[0],)
    wb("patch_embed.proj", widths[0], 3, 7, 7)
    wb("patch_embed.norm", widths[0])
    for i, (C, d, r, sr) in enumerate(zip(widths, depths, ratios, PVT_SR)):
        p = f"stages.{i}."
        if i > 0:
            wb(p + "downsample.proj", C, widths[i - 1], 3, 3)
            wb(p + "downsample.norm", C)
        for j in range(d):
            q = p + f"blocks.{j}."
            wb(q + "norm1", C)
            wb(q + "attn.q", C, C)
            wb(q + "attn.kv", 2 * C, C)
            wb(q + "attn.proj", C, C)
            if sr > 1:
                wb(q + "attn.sr", C, C, sr, sr)
                wb(q + "attn.norm", C)
            wb(q + "norm2", C)
            wb(q + "mlp.fc1", r * C, C)
            wb(q + "mlp.dwconv", r * C, 1, 3, 3)
            wb(q + "mlp.fc2", C, r * C)
        wb(p + "norm", C)
    return s


def pvt_num_learnable(arch, num_classes=0):
    """Learnable parameters of the table, with an optional classifier."""
    return sum(math.prod(shp) for shp in param_shapes(arch, 224, num_classes).values())


def _regnet_shapes(arch):
    """timm's state-dict order for a RegNet (regnet.py; the key names are written from memory of that file, not verified against a timm
    install): the stem, then per block conv1, conv2, se (RegNetY), conv3 and, in the first block of a stage, downsample.  A ConvNormAct is
    ``conv.weight`` + ``bn.*``; the squeeze-excite convolutions carry biases.  ``num_batches_tracked`` is not listed."""
    s = OrderedDict()

    def cna(p, cout, cin, k):
        s[p + ".conv.weight"] = (cout, cin, k, k)
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            s[f"{p}.bn.{leaf}"] = (cout,)
    cna("stem", REGNET_STEM, 3, 3)
    for b in regnet_blocks(arch):
        p = b["key"]
        cna(p + ".conv1", b["w"], b["cin"], 1)
        cna(p + ".conv2", b["w"], b["gw"], 3)
        if b["se"]:
            s[p + ".se.fc1.weight"] = (b["se"], b["w"], 1, 1)
            s[p + ".se.fc1.bias"] = (b["se"],)
            s[p + ".se.fc2.weight"] = (b["w"], b["se"], 1, 1)
            s[p + ".se.fc2.bias"] = (b["w"],)
        cna(p + ".conv3", b["w"], b["w"], 1)
        if b["down"]:
            cna(p + ".downsample", b["w"], b["cin"], 1)
    return s


def regnet_num_learnable(arch, num_classes=0):
    """Learnable parameters (BN running statistics excluded) of the table, with an optional classifier."""
    return sum(math.prod(shp) for k, shp in param_shapes(arch, 224, num_classes).items() if not k.endswith(("running_mean", "running_var")))


def _levit_shapes(arch, img_size):
    """timm >= 0.9's state-dict order for a Levit (levit.py; the key names are written from memory of that file, not verified against a
    timm install): the stem, then per stage its downsample (stages 1 and 2) and its blocks.  A LinearNorm is ``linear.weight`` + ``bn.*``;
    the length of an ``attention_biases`` row is the number of distinct (|dy|, |dx|) offsets of its key grid, R^2 — the crop size is part
    of the shapes.  The derived ``attention_bias_idxs`` buffers and ``num_batches_tracked`` are not listed (ignored when present)."""
    widths, kd, heads, depths = LEVIT_CFG[arch]
    if img_size % 16 or not 32 <= img_size <= 224:
        raise ValueError(f"{arch}: img_size must be a multiple of 16 from 32 to 224, got {img_size}")
    s = OrderedDict()

    def bn(p, c):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            s[f"{p}.{leaf}"] = (c,)

    def linear_norm(p, n, k):
        s[p + ".linear.weight"] = (n, k)
        bn(p + ".bn", n)

    def mlp(p, d):
        linear_norm(p + ".ln1", 2 * d, d)
        linear_norm(p + ".ln2", d, 2 * d)

    cin = 3
    for i in range(4):
        cout = widths[0] >> (3 - i)
        s[f"stem.conv{i + 1}.linear.weight"] = (cout, cin, 3, 3)
        bn(f"stem.conv{i + 1}.bn", cout)
        cin = cout
    R = img_size // 16
    for st in range(3):
        D = widths[st]
        if st > 0:
            din = widths[st - 1]
            h = din // kd
            p = f"stages.{st}.downsample.attn_downsample"
            s[p + ".attention_biases"] = (h, R * R)
            linear_norm(p + ".kv", h * 5 * kd, din)
            linear_norm(p + ".q.ln", h * kd, din)
            linear_norm(p + ".proj.ln", D, h * 4 * kd)
            mlp(f"stages.{st}.downsample.mlp", D)
            R = levit_sub(R)
        for j in range(depths[st]):
            p = f"stages.{st}.blocks.{j}."
            s[p + "attn.attention_biases"] = (heads[st], R * R)
            linear_norm(p + "attn.qkv", heads[st] * 4 * kd, D)
            linear_norm(p + "attn.proj.ln", D, heads[st] * 2 * kd)
            mlp(p + "mlp", D)
    return s


def levit_num_learnable(arch, img_size=224, num_classes=0):
    """Learnable parameters (BN running statistics excluded) of the table, with timm's two optional classifier heads."""
    return sum(math.prod(shp) for k, shp in param_shapes(arch, img_size, num_classes).items()
               if not k.endswith(("running_mean", "running_var")))


def levit_fold_heads(sd, eps=LEVIT_BN_EPS):
    """timm's Levit classifier — the average of two ``BatchNorm1d + Linear`` heads (head, head_dist) — folded in float64 into one
    weight [N, D] and bias [N] (float32) for the fp32 head library: logits = emb . W^T + b."""
    sd = strip_prefix(sd)
    Ws, bs = [], []
    for h in ("head", "head_dist"):
        g, beta = sd[h + ".bn.weight"].double(), sd[h + ".bn.bias"].double()
        mean, var = sd[h + ".bn.running_mean"].double(), sd[h + ".bn.running_var"].double()
        w, b = sd[h + ".linear.weight"].double(), sd[h + ".linear.bias"].double()
        sc = g / torch.sqrt(var + eps)
        Ws.append(w * sc[None, :])
        bs.append(b + w @ (beta - mean * sc))
    return ((Ws[0] + Ws[1]) / 2).float().contiguous(), ((bs[0] + bs[1]) / 2).float().contiguous()


def _vit8_shapes(arch, img_size):
    """timm's state-dict order for a VisionTransformer with patch_size 8: the patch-16 table with an 8x8 patch conv and
    (img_size / 8)^2 + 1 position rows."""
    D, depth, heads, r = VIT8_CFG[arch]
    if img_size % VIT8_PATCH or not VIT8_PATCH <= img_size <= 224:
        raise ValueError(f"{arch}: img_size must be a multiple of {VIT8_PATCH} from {VIT8_PATCH} to 224, got {img_size}")
    s = OrderedDict()
    s["cls_token"] = (1, 1, D)
    s["pos_embed"] = (1, (img_size // VIT8_PATCH) ** 2 + 1, D)
    s["patch_embed.proj.weight"] = (D, 3, VIT8_PATCH, VIT8_PATCH)
    s["patch_embed.proj.bias"] = (D,)
    for i in range(depth):
        p = f"blocks.{i}."
        s[p + "norm1.weight"] = (D,)
        s[p + "norm1.bias"] = (D,)
        s[p + "attn.qkv.weight"] = (3 * D, D)
        s[p + "attn.qkv.bias"] = (3 * D,)
        s[p + "attn.proj.weight"] = (D, D)
        s[p + "attn.proj.bias"] = (D,)
        s[p + "norm2.weight"] = (D,)
        s[p + "norm2.bias"] = (D,)
        s[p + "mlp.fc1.weight"] = (r * D, D)
        s[p + "mlp.fc1.bias"] = (r * D,)
        s[p + "mlp.fc2.weight"] = (D, r * D)
        s[p + "mlp.fc2.bias"] = (D,)
    s["norm.weight"] = (D,)
    s["norm.bias"] = (D,)
    return s


def _bit_shapes(arch):
    """timm's state-dict order: the shortcut convolution is the first child of a stage's first block.  No convolution has a bias and no
    norm has running statistics (GroupNorm)."""
    s = OrderedDict()
    s["stem.conv.weight"] = (64, 3, 7, 7)
    cin = 64
    for i, (nb, mid) in enumerate(zip(BIT_CFG[arch], BIT_WIDTHS)):
        for j in range(nb):
            p = f"stages.{i}.blocks.{j}."
            if j == 0:
                s[p + "downsample.conv.weight"] = (4 * mid, cin, 1, 1)
            s[p + "norm1.weight"] = (cin,)
            s[p + "norm1.bias"] = (cin,)
            s[p + "conv1.weight"] = (mid, cin, 1, 1)
            s[p + "norm2.weight"] = (mid,)
            s[p + "norm2.bias"] = (mid,)
            s[p + "conv2.weight"] = (mid, mid, 3, 3)
            s[p + "norm3.weight"] = (mid,)
            s[p + "norm3.bias"] = (mid,)
            s[p + "conv3.weight"] = (4 * mid, mid, 1, 1)
            cin = 4 * mid
    s["norm.weight"] = (cin,)
    s["norm.bias"] = (cin,)
    return s


def _beit_shapes(arch, img_size):
    """timm's state-dict order (a module's own parameters before its children's: the layer scales open a block; q_bias, v_bias and the
    bias table open its attention).  The table's length follows from the patch grid: (2 img_size/16 - 1)^2 + 3."""
    D, depth, heads, r = BEIT_CFG[arch]
    if img_size % PATCH or not PATCH <= img_size <= 224:
        raise ValueError(f"{arch}: img_size must be a multiple of {PATCH} from {PATCH} to 224, got {img_size}")
    entries = (2 * (img_size // PATCH) - 1) ** 2 + 3
    s = OrderedDict()
    s["cls_token"] = (1, 1, D)
    s["patch_embed.proj.weight"] = (D, 3, PATCH, PATCH)
    s["patch_embed.proj.bias"] = (D,)
    for i in range(depth):
        p = f"blocks.{i}."
        s[p + "gamma_1"] = (D,)
        s[p + "gamma_2"] = (D,)
        s[p + "norm1.weight"] = (D,)
        s[p + "norm1.bias"] = (D,)
        s[p + "attn.q_bias"] = (D,)
        s[p + "attn.v_bias"] = (D,)
        s[p + "attn.relative_position_bias_table"] = (entries, heads)
        s[p + "attn.qkv.weight"] = (3 * D, D)
        s[p + "attn.proj.weight"] = (D, D)
        s[p + "attn.proj.bias"] = (D,)
        s[p + "norm2.weight"] = (D,)
        s[p + "norm2.bias"] = (D,)
        s[p + "mlp.fc1.weight"] = (r * D, D)
        s[p + "mlp.fc1.bias"] = (r * D,)
        s[p + "mlp.fc2.weight"] = (D, r * D)
        s[p + "mlp.fc2.bias"] = (D,)
    s["fc_norm.weight"] = (D,)
    s["fc_norm.bias"] = (D,)
    return s


def _swin_shapes(arch):
    """timm >= 0.9 state-dict order (a module's own parameters before its children's: the bias table before qkv / proj)."""
    C0, depths, heads, ws = SWIN_CFG[arch]
    s = OrderedDict()
    s["patch_embed.proj.weight"] = (C0, 3, 4, 4)
    s["patch_embed.proj.bias"] = (C0,)
    s["patch_embed.norm.weight"] = (C0,)
    s["patch_embed.norm.bias"] = (C0,)
    for i, (nb, nh) in enumerate(zip(depths, heads)):
        c = C0 << i
        p = f"layers.{i}."
        if i > 0:
            s[p + "downsample.norm.weight"] = (2 * c,)    # LayerNorm over the 4 C_prev = 2 c gathered channels
            s[p + "downsample.norm.bias"] = (2 * c,)
            s[p + "downsample.reduction.weight"] = (c, 2 * c)
        for j in range(nb):
            q = p + f"blocks.{j}."
            s[q + "norm1.weight"] = (c,)
            s[q + "norm1.bias"] = (c,)
            s[q + "attn.relative_position_bias_table"] = ((2 * ws - 1) ** 2, nh)
            s[q + "attn.qkv.weight"] = (3 * c, c)
            s[q + "attn.qkv.bias"] = (3 * c,)
            s[q + "attn.proj.weight"] = (c, c)
            s[q + "attn.proj.bias"] = (c,)
            s[q + "norm2.weight"] = (c,)
            s[q + "norm2.bias"] = (c,)
            s[q + "mlp.fc1.weight"] = (4 * c, c)
            s[q + "mlp.fc1.bias"] = (4 * c,)
            s[q + "mlp.fc2.weight"] = (c, 4 * c)
            s[q + "mlp.fc2.bias"] = (c,)
    s["norm.weight"] = (C0 * 8,)
    s["norm.bias"] = (C0 * 8,)
    return s


def _mobilenetv3_shapes(arch, num_classes=0):
    """timm's state-dict order: a module's own parameters, then its children's; BN with running statistics (num_batches_tracked
    left out, as for the other CNNs)."""
    s = OrderedDict()

    def bn(p, c):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            s[f"{p}.{leaf}"] = (c,)

    def se(p, c, r):
        s[p + ".se.conv_reduce.weight"] = (r, c, 1, 1)
        s[p + ".se.conv_reduce.bias"] = (r,)
        s[p + ".se.conv_expand.weight"] = (c, r, 1, 1)
        s[p + ".se.conv_expand.bias"] = (c,)
    stem, blocks, nf = mobilenetv3_blocks(arch)
    s["conv_stem.weight"] = (stem, 3, 3, 3)
    bn("bn1", stem)
    for b in blocks:
        p = b["key"]
        if b["type"] == "ds":
            s[p + ".conv_dw.weight"] = (b["cin"], 1, b["k"], b["k"])
            bn(p + ".bn1", b["cin"])
            if b["se"]:
                se(p, b["cin"], b["se"])
            s[p + ".conv_pw.weight"] = (b["cout"], b["cin"], 1, 1)
            bn(p + ".bn2", b["cout"])
        elif b["type"] == "ir":
            s[p + ".conv_pw.weight"] = (b["mid"], b["cin"], 1, 1)
            bn(p + ".bn1", b["mid"])
            s[p + ".conv_dw.weight"] = (b["mid"], 1, b["k"], b["k"])
            bn(p + ".bn2", b["mid"])
            if b["se"]:
                se(p, b["mid"], b["se"])
            s[p + ".conv_pwl.weight"] = (b["cout"], b["mid"], 1, 1)
            bn(p + ".bn3", b["cout"])
        else:
            s[p + ".conv.weight"] = (b["cout"], b["cin"], 1, 1)
            bn(p + ".bn1", b["cout"])
    s["conv_head.weight"] = (nf, blocks[-1]["cout"], 1, 1)
    s["conv_head.bias"] = (nf,)
    if num_classes:
        s["classifier.weight"] = (num_classes, nf)
        s["classifier.bias"] = (num_classes,)
    return s


def _efficientnet_shapes(arch, num_classes=0):
    """timm's state-dict order, as _mobilenetv3_shapes; conv_head has no bias and is followed by bn2."""
    s = OrderedDict()

    def bn(p, c):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            s[f"{p}.{leaf}"] = (c,)

    def se(p, c, r):
        s[p + ".se.conv_reduce.weight"] = (r, c, 1, 1)
        s[p + ".se.conv_reduce.bias"] = (r,)
        s[p + ".se.conv_expand.weight"] = (c, r, 1, 1)
        s[p + ".se.conv_expand.bias"] = (c,)
    stem, blocks, nf = efficientnet_blocks(arch)
    s["conv_stem.weight"] = (stem, 3, 3, 3)
    bn("bn1", stem)
    for b in blocks:
        p = b["key"]
        if b["type"] == "ds":
            s[p + ".conv_dw.weight"] = (b["cin"], 1, b["k"], b["k"])
            bn(p + ".bn1", b["cin"])
            se(p, b["cin"], b["se"])
            s[p + ".conv_pw.weight"] = (b["cout"], b["cin"], 1, 1)
            bn(p + ".bn2", b["cout"])
        else:
            s[p + ".conv_pw.weight"] = (b["mid"], b["cin"], 1, 1)
            bn(p + ".bn1", b["mid"])
            s[p + ".conv_dw.weight"] = (b["mid"], 1, b["k"], b["k"])
            bn(p + ".bn2", b["mid"])
            se(p, b["mid"], b["se"])
            s[p + ".conv_pwl.weight"] = (b["cout"], b["mid"], 1, 1)
            bn(p + ".bn3", b["cout"])
    s["conv_head.weight"] = (nf, blocks[-1]["cout"], 1, 1)
    bn("bn2", nf)
    if num_classes:
        s["classifier.weight"] = (num_classes, nf)
        s["classifier.bias"] = (num_classes,)
    return s


def efficientnet_num_learnable(arch, num_classes=0):
    """Learnable parameters (BN running statistics excluded) of the builder's table, with an optional classifier."""
    return sum(math.prod(shp) for k, shp in _efficientnet_shapes(arch, num_classes).items()
               if not k.endswith(("running_mean", "running_var")))


def mobilenetv3_num_learnable(arch, num_classes=0):
    """Learnable parameters (BN running statistics excluded) of the builder's table, with an optional classifier."""
    n = 0
    for k, shp in _mobilenetv3_shapes(arch, num_classes).items():
        if not k.endswith(("running_mean", "running_var")):
            n += math.prod(shp)
    return n


def init_state_dict(arch, seed=0, img_size=224, scale="unit", num_classes=0):
    """Seeded random-init fp32 CPU state dict with timm key names.

    scale="timm": trunc_normal(0.02) linears / kaiming convs, LN and BN at identity — what
    timm's own initialisers give.  scale="unit" (default): fan-in-scaled weights, non-trivial
    LN/BN affine terms and running statistics, so that attention is far from uniform and every
    term of every kernel (biases, gamma/beta, BN folding) is exercised by the parity tests.
    The generator is the CPU Philox stream, identical on every machine with this torch build.
    ConvNeXt (_init_convnext) and MobileNetV3 / EfficientNet-B0 (_init_mobilenetv3) draw from generators of their own with rules of their own.
    ``num_classes`` > 0 appends timm's classifier head, drawn from a generator of its own (init_head): the encoder's
    parameters are the same with and without a head.
    """
    if num_classes:
        sd = init_state_dict(arch, seed, img_size, scale)
        sd.update(init_head(arch, num_classes, seed, scale))
        return sd
    if arch in CONVNEXT_CFG:
        return _init_convnext(arch, seed, img_size, scale)
    if arch in MOBILENETV3_CFG or arch in EFFICIENTNET_CFG:
        return _init_mobilenetv3(arch, seed, img_size, scale)
    if arch in SWIN_CFG:
        return _init_swin(arch, seed, img_size, scale)
    if is_resnet_lib(arch):
        return _init_resnet(arch, seed, img_size, scale)
    if arch in BEIT_CFG:
        return _init_beit(arch, seed, img_size, scale)
    if arch in BIT_CFG:
        return _init_bit(arch, seed, scale)
    if arch in VIT8_CFG:
        return _init_vit8(arch, seed, img_size, scale)
    if arch in LEVIT_CFG:
        return _init_levit(arch, seed, img_size, scale)
    if is_regnet(arch):
        return _init_regnet(arch, seed, scale)
    if arch in PVT_CFG:
        return _init_pvt(arch, seed, scale)
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    sd = OrderedDict()

    def randn(shape, std):
        return torch.randn(shape, generator=g, dtype=torch.float32) * std

    def uniform(shape, lo, hi):
        return torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo

    for k, shp in param_shapes(arch, img_size).items():
        leaf = k.rsplit(".", 1)[-1]
        if scale == "timm":
            if k in ("cls_token",):
                v = randn(shp, 1e-6)
            elif k == "pos_embed":
                v = randn(shp, 0.02).clamp_(-0.04, 0.04)
            elif leaf == "running_mean":
                v = torch.zeros(shp)
            elif leaf == "running_var":
                v = torch.ones(shp)
            elif len(shp) == 1:
                v = torch.ones(shp) if leaf == "weight" else torch.zeros(shp)
            elif len(shp) == 4 and arch in RESNET_CFG:
                v = randn(shp, math.sqrt(2.0 / (shp[0] * shp[2] * shp[3])))
            else:
                v = randn(shp, 0.02).clamp_(-0.04, 0.04)
        else:
            if k in ("cls_token", "pos_embed"):
                v = randn(shp, 0.5)
            elif leaf == "running_mean":
                v = randn(shp, 0.1)
            elif leaf == "running_var":
                v = uniform(shp, 0.5, 1.5)
            elif len(shp) == 1:
                is_norm = ("norm" in k) or (".bn" in k) or k.startswith("bn") or ("downsample.1" in k)
                if leaf == "weight" and is_norm:
                    v = uniform(shp, 0.5, 1.5)
                else:
                    v = randn(shp, 0.1)
            else:
                fan_in = 1
                for d in shp[1:]:
                    fan_in *= d
                gain = math.sqrt(2.0) if arch in RESNET_CFG else 1.0
                v = randn(shp, gain / math.sqrt(fan_in))
        sd[k] = v.contiguous()
    return sd


def _init_convnext(arch, seed, img_size, scale):
    """ConvNeXt seeded init.  scale="timm": what timm's initialiser gives (trunc_normal(0.02) convs and linears, zero biases,
    LayerNorms at identity, layer scale gamma = 1e-6 — every block then nearly a no-op).  scale="unit": fan-in-scaled convs and
    linears (the depthwise conv's fan-in is 49), non-trivial LayerNorm affine terms (stem.1 and downsample.0 are LayerNorms
    although their names lack "norm"), biases N(0, 0.1) and gamma = U(0.2, 1.0): every term of every kernel is exercised."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    sd = OrderedDict()

    def randn(shape, std):
        return torch.randn(shape, generator=g, dtype=torch.float32) * std

    def uniform(shape, lo, hi):
        return torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo

    for k, shp in param_shapes(arch, img_size).items():
        leaf = k.rsplit(".", 1)[-1]
        is_ln = k.startswith("stem.1.") or ".downsample.0." in k or ".norm." in k or k.startswith("head.norm.")
        if scale == "timm":
            if leaf == "gamma":
                v = torch.full(shp, 1e-6)
            elif len(shp) == 1:
                v = torch.ones(shp) if (leaf == "weight" and is_ln) else torch.zeros(shp)
            else:
                v = randn(shp, 0.02).clamp_(-0.04, 0.04)
        else:
            if leaf == "gamma":
                v = uniform(shp, 0.2, 1.0)
            elif len(shp) == 1:
                v = uniform(shp, 0.5, 1.5) if (leaf == "weight" and is_ln) else randn(shp, 0.1)
            else:
                fan_in = 1
                for d in shp[1:]:
                    fan_in *= d
                v = randn(shp, 1.0 / math.sqrt(fan_in))
        sd[k] = v.contiguous()
    return sd


def _init_mobilenetv3(arch, seed, img_size, scale):
    """MobileNetV3 (and EfficientNet-B0: the same builder's key names and shapes) seeded init.  scale="timm": timm's _init_weight_goog (convs N(0, sqrt(2 / fan_out)) with fan_out = k*k*out / groups,
    zero biases, BN at identity with running statistics 0 / 1).  scale="unit": fan-in-scaled convs, BN gains U(0.5, 1.5), shifts and
    running means N(0, 0.1), running variances U(0.5, 2.0), conv biases N(0, 0.1): every term of the BN folding is exercised."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    sd = OrderedDict()

    def randn(shape, std):
        return torch.randn(shape, generator=g, dtype=torch.float32) * std

    def uniform(shape, lo, hi):
        return torch.rand(shape, generator=g, dtype=torch.float32) * (hi - lo) + lo

    for k, shp in param_shapes(arch, img_size).items():
        leaf = k.rsplit(".", 1)[-1]
        if len(shp) == 4:
            dw = shp[1] == 1 and shp[2] > 1
            if scale == "timm":
                fan_out = shp[2] * shp[3] * (1 if dw else shp[0])
                v = randn(shp, math.sqrt(2.0 / fan_out))
            else:
                v = randn(shp, 1.0 / math.sqrt(shp[1] * shp[2] * shp[3]))
        elif scale == "timm":
            v = torch.ones(shp) if leaf in ("weight", "running_var") else torch.zeros(shp)
        elif leaf == "weight":
            v = uniform(shp, 0.5, 1.5)
        elif leaf == "running_var":
            v = uniform(shp, 0.5, 2.0)
        else:
            v = randn(shp, 0.1)
        sd[k] = v.contiguous()
    return sd


def _init_swin(arch, seed, img_size, scale):
    """Swin seeded init.  scale="timm": what timm's initialiser gives (trunc_normal(0.02) linears and bias tables, zero biases,
    LayerNorms at identity).  scale="unit": fan-in-scaled linears and patch conv, LayerNorm gains U(0.5, 1.5), biases N(0, 0.1) and
    bias tables N(0, 1) — a relative-position term as large as the scores, so a wrong index, mask or merge order shows."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    sd = OrderedDict()

    def randn(shape, std):
        return torch.randn(shape, generator=g, dtype=torch.float32) * std

    for k, shp in param_shapes(arch, img_size).items():
        leaf = k.rsplit(".", 1)[-1]
        is_ln = ".norm" in k or k.startswith("norm.") or "patch_embed.norm." in k
        if leaf == "relative_position_bias_table":
            v = randn(shp, 0.02).clamp_(-0.04, 0.04) if scale == "timm" else randn(shp, 1.0)
        elif len(shp) == 1:
            if scale == "timm":
                v = torch.ones(shp) if (leaf == "weight" and is_ln) else torch.zeros(shp)
            else:
                v = torch.rand(shp, generator=g) + 0.5 if (leaf == "weight" and is_ln) else randn(shp, 0.1)
        elif scale == "timm":
            v = randn(shp, 0.02).clamp_(-0.04, 0.04)
        else:
            v = randn(shp, 1.0 / math.sqrt(math.prod(shp[1:])))
        sd[k] = v.contiguous()
    return sd


def _init_beit(arch, seed, img_size, scale):
    """BEiT seeded init from a CPU Philox generator of its own.  Both scales set the layer scales gamma_1 / gamma_2 to 0.1 (timm's
    init_values for the base models) and draw nonzero bias tables and biases, so that no term of the forward is switched off:
    scale="timm": trunc_normal(0.02) linears, patch conv and cls token, LayerNorms at identity, bias tables and biases N(0, 0.02);
    scale="unit": fan-in-scaled linears and patch conv, cls token N(0, 0.5), LayerNorm gains U(0.5, 1.5), biases N(0, 0.1) and bias
    tables N(0, 1) — a relative-position term as large as the scores, so a wrong index shows."""
    g = torch.Generator(device="cpu")
    g.manual_seed((int(seed) * 0x9E3779B1 + 0x62656974) % (1 << 63))
    sd = OrderedDict()

    def randn(shape, std):
        return torch.randn(shape, generator=g, dtype=torch.float32) * std

    for k, shp in param_shapes(arch, img_size).items():
        leaf = k.rsplit(".", 1)[-1]
        is_ln = "norm" in k
        if leaf in ("gamma_1", "gamma_2"):
            v = torch.full(shp, 0.1)
        elif leaf == "relative_position_bias_table":
            v = randn(shp, 0.02 if scale == "timm" else 1.0)
        elif k == "cls_token":
            v = randn(shp, 0.02).clamp_(-0.04, 0.04) if scale == "timm" else randn(shp, 0.5)
        elif len(shp) == 1:
            if scale == "timm":
                v = torch.ones(shp) if (leaf == "weight" and is_ln) else (torch.zeros(shp) if is_ln else randn(shp, 0.02))
            else:
                v = torch.rand(shp, generator=g) + 0.5 if (leaf == "weight" and is_ln) else randn(shp, 0.1)
        elif scale == "timm":
            v = randn(shp, 0.02).clamp_(-0.04, 0.04)
        else:
            v = randn(shp, 1.0 / math.sqrt(math.prod(shp[1:])))
        sd[k] = v.contiguous()
    return sd


def _init_levit(arch, seed, img_size, scale):
    """LeViT seeded init from a CPU Philox generator of its own.  scale="timm": trunc_normal(0.02) weights, BatchNorms at identity except
    the last one of every residual branch (attn.proj.ln.bn, mlp.ln2.bn) at gamma 0, attention biases 0 — what timm's initialiser gives,
    and a network whose residual branches and biases are all switched off.  scale="unit" (default): fan-in-scaled weights, attention
    biases N(0, 1), BN gammas U(0.5, 1.5), betas and running means N(0, 0.1), running variances U(0.5, 1.5): no term is zero.  The last BN
    of every residual branch draws its gamma from U(0.2, 0.5) instead: with gammas around 1 the up to 24 residual additions double the
    stream's variance each (levit_128s reaches |x| ~ 60 and a 16-bit rounding error of 1.2e-2 against 3e-3).  The price is that every
    branch, the attention's among them, adds a fraction of the stream: zeroing or transposing the biases moves a 32^2 - 64^2 embedding by
    3 to 13 % depending on the seed and a 224^2 one by under 1 % — tests that rely on that sensitivity pick their seeds on the CPU
    reference (tests/test_gpu_levit.py: CKPT_SEED)."""
    if scale not in ("unit", "timm"):
        raise ValueError(f"scale must be 'unit' or 'timm', got {scale!r}")
    g = torch.Generator(device="cpu")
    g.manual_seed((int(seed) * 0x9E3779B1 + 0x6C657669) % (1 << 63))
    sd = OrderedDict()
    for k, shp in _levit_shapes(arch, img_size).items():
        leaf = k.rsplit(".", 1)[-1]
        last = (".proj.ln.bn." in k or ".mlp.ln2.bn." in k) and ".attn_downsample." not in k
        if leaf == "attention_biases":
            v = torch.zeros(shp) if scale == "timm" else torch.randn(shp, generator=g, dtype=torch.float32)
        elif len(shp) > 1:
            if scale == "timm":
                v = (torch.randn(shp, generator=g, dtype=torch.float32) * 0.02).clamp_(-0.04, 0.04)
            else:
                v = torch.randn(shp, generator=g, dtype=torch.float32) / math.sqrt(math.prod(shp[1:]))
        elif scale == "timm":
            if leaf in ("bias", "running_mean"):
                v = torch.zeros(shp)
            elif leaf == "running_var":
                v = torch.ones(shp)
            else:
                v = torch.zeros(shp) if last else torch.ones(shp)
        elif leaf == "running_var":
            v = torch.rand(shp, generator=g, dtype=torch.float32) + 0.5
        elif leaf in ("bias", "running_mean"):
            v = torch.randn(shp, generator=g, dtype=torch.float32) * 0.1
        elif last:
            v = torch.rand(shp, generator=g, dtype=torch.float32) * 0.3 + 0.2
        else:
            v = torch.rand(shp, generator=g, dtype=torch.float32) + 0.5
        sd[k] = v.contiguous()
    return sd


def _init_vit8(arch, seed, img_size, scale):
    """Patch-8 ViT seeded init from a CPU Philox generator of its own.  scale="timm": trunc_normal(0.02) linears, patch conv and
    pos_embed, cls token N(0, 1e-6), LayerNorms at identity, zero biases — what timm's initialiser gives.  scale="unit": fan-in-scaled
    linears and patch conv, cls token and pos_embed N(0, 0.5), LayerNorm gains U(0.5, 1.5), biases N(0, 0.1): attention over the 785
    tokens is far from uniform and no term of the forward is switched off.  scale="trained": the unit rule with the magnitudes of a
    trained ViT — pos_embed and cls token N(0, 0.1), attn.proj and mlp.fc2 at a quarter of the fan-in scale, so that a block adds a
    fraction of the residual stream instead of doubling its variance."""
    if scale not in ("unit", "timm", "trained"):
        raise ValueError(f"scale must be 'unit', 'timm' or 'trained', got {scale!r}")
    g = torch.Generator(device="cpu")
    g.manual_seed((int(seed) * 0x9E3779B1 + 0x76697438) % (1 << 63))
    sd = OrderedDict()

    def randn(shape, std):
        return torch.randn(shape, generator=g, dtype=torch.float32) * std

    for k, shp in _vit8_shapes(arch, img_size).items():
        leaf = k.rsplit(".", 1)[-1]
        is_ln = "norm" in k
        if scale == "timm":
            if k == "cls_token":
                v = randn(shp, 1e-6)
            elif len(shp) == 1:
                v = torch.ones(shp) if (leaf == "weight" and is_ln) else torch.zeros(shp)
            else:
                v = randn(shp, 0.02).clamp_(-0.04, 0.04)
        elif k in ("cls_token", "pos_embed"):
            v = randn(shp, 0.5 if scale == "unit" else 0.1)
        elif len(shp) == 1:
            v = torch.rand(shp, generator=g, dtype=torch.float32) + 0.5 if (leaf == "weight" and is_ln) else randn(shp, 0.1)
        else:
            gain = 0.25 if (scale == "trained" and (".attn.proj." in k or ".mlp.fc2." in k)) else 1.0
            v = randn(shp, gain / math.sqrt(math.prod(shp[1:])))
        sd[k] = v.contiguous()
    return sd


def _init_bit(arch, seed, scale):
    """BiT ResNetV2 from a CPU Philox generator of its own.  Convolutions are N(0, 1 / fan_in) in both scales (weight standardisation
    removes their mean and scale anyway; timm draws N(0, sqrt(2 / fan_out))).  scale="timm": GroupNorms at identity, with norm3's gamma 0
    (timm's zero_init_last).  scale="unit": gammas U(0.5, 1.5) and betas N(0, 0.2), norm3's gamma and beta x 0.25 — so that a residual
    branch adds a fraction of the stream, as a trained network's does, instead of doubling its variance per block."""
    g = torch.Generator(device="cpu")
    g.manual_seed((int(seed) * 0x9E3779B1 + 0x62697432) % (1 << 63))
    sd = OrderedDict()
    for k, shp in _bit_shapes(arch).items():
        leaf = k.rsplit(".", 1)[-1]
        last = ".norm3." in k
        if len(shp) == 4:
            v = torch.randn(shp, generator=g, dtype=torch.float32) / math.sqrt(shp[1] * shp[2] * shp[3])
        elif scale == "timm":
            v = torch.zeros(shp) if (leaf == "bias" or last) else torch.ones(shp)
        elif leaf == "weight":
            v = (torch.rand(shp, generator=g, dtype=torch.float32) + 0.5) * (0.25 if last else 1.0)
        else:
            v = torch.randn(shp, generator=g, dtype=torch.float32) * 0.2 * (0.25 if last else 1.0)
        sd[k] = v.contiguous()
    return sd


def _init_regnet(arch, seed, scale):
    """RegNetX / RegNetY from a CPU Philox generator of their own.  Convolutions are kaiming-normal over their fan-in (std sqrt(2 / fan_in);
    a grouped 3x3 has fan-in 9 x the group width), as the ResNets'.  scale="timm": BN at identity, conv3's gamma 0 (timm's zero_init_last),
    squeeze-excite biases 0.  scale="unit": BN running means N(0, 0.1), running variances U(0.5, 1.5), betas N(0, 0.1), gammas U(0.5, 1.5)
    except conv3's, U(0.2, 0.5) — so that the residual additions keep the stream within a few units, as a trained network's does — and
    squeeze-excite weights N(0, 4 / fan_in), biases N(0, 0.5): gates spread over (0, 1) instead of sitting at 1/2."""
    g = torch.Generator(device="cpu")
    g.manual_seed((int(seed) * 0x9E3779B1 + 0x7265676E) % (1 << 63))
    sd = OrderedDict()
    for k, shp in _regnet_shapes(arch).items():
        leaf = k.rsplit(".", 1)[-1]
        last = ".conv3.bn." in k
        if ".se." in k:
            if len(shp) == 4:
                v = torch.randn(shp, generator=g, dtype=torch.float32) * (math.sqrt(2.0 / shp[1]) if scale == "timm" else 2.0 / math.sqrt(shp[1]))
            else:
                v = torch.zeros(shp) if scale == "timm" else torch.randn(shp, generator=g, dtype=torch.float32) * 0.5
        elif len(shp) == 4:
            v = torch.randn(shp, generator=g, dtype=torch.float32) * math.sqrt(2.0 / (shp[1] * shp[2] * shp[3]))
        elif scale == "timm":
            if leaf in ("bias", "running_mean"):
                v = torch.zeros(shp)
            elif leaf == "running_var":
                v = torch.ones(shp)
            else:
                v = torch.zeros(shp) if last else torch.ones(shp)
        elif leaf == "running_var":
            v = torch.rand(shp, generator=g, dtype=torch.float32) + 0.5
        elif leaf in ("bias", "running_mean"):
            v = torch.randn(shp, generator=g, dtype=torch.float32) * 0.1
        elif last:
            v = torch.rand(shp, generator=g, dtype=torch.float32) * 0.3 + 0.2
        else:
            v = torch.rand(shp, generator=g, dtype=torch.float32) + 0.5
        sd[k] = v.contiguous()
    return sd


def _init_pvt(arch, seed, scale):
    """PVTv2 seeded init from a CPU Philox generator of its own.  scale="timm": trunc_normal(0.02) linears, convolutions N(0, 2 / fan_out)
    (fan_out = k^2 Cout / groups), LayerNorms at identity, zero biases — what timm's initialiser gives.  scale="unit" (default):
    fan-in-scaled linears and convolutions (a depthwise 3x3 has fan-in 9), LayerNorm gains U(0.5, 1.5), biases N(0, 0.1): attention over the
    reduced keys is far from uniform and no term of the forward is switched off.  scale="trained": the unit rule with attn.proj and mlp.fc2
    at a quarter of the fan-in scale, so that a block adds a fraction of the residual stream, as a trained network's does, instead of
    doubling its variance."""
    if scale not in ("unit", "timm", "trained"):
        raise ValueError(f"scale must be 'unit', 'timm' or 'trained', got {scale!r}")
    g = torch.Generator(device="cpu")
    g.manual_seed((int(seed) * 0x9E3779B1 + 0x70767432) % (1 << 63))
    sd = OrderedDict()

    def randn(shape, std):
        return torch.randn(shape, generator=g, dtype=torch.float32) * std

    for k, shp in _pvt_shapes(arch).items():
        leaf = k.rsplit(".", 1)[-1]
        is_ln = "norm" in k.rsplit(".", 2)[-2]
        if scale == "timm":
            if len(shp) == 1:
                v = torch.ones(shp) if (leaf == "weight" and is_ln) else torch.zeros(shp)
            elif len(shp) == 4:
                groups = shp[0] if shp[1] == 1 and ".dwconv." in k else 1
                v = randn(shp, math.sqrt(2.0 / (shp[2] * shp[3] * shp[0] / groups)))
            else:
                v = randn(shp, 0.02).clamp_(-0.04, 0.04)
        elif len(shp) == 1:
            v = torch.rand(shp, generator=g, dtype=torch.float32) + 0.5 if (leaf == "weight" and is_ln) else randn(shp, 0.1)
        else:
            gain = 0.25 if (scale == "trained" and (".attn.proj." in k or ".mlp.fc2." in k)) else 1.0
            v = randn(shp, gain / math.sqrt(math.prod(shp[1:])))
        sd[k] = v.contiguous()
    return sd


def _init_resnet(arch, seed, img_size, scale):
    """resnet34 / resnet50 from a CPU Philox generator of their own (resnet18 keeps the generic stream of init_state_dict).
    Convolutions are kaiming-normal (std sqrt(2 / fan_in)), as timm's.  scale="timm": BN at identity, with the last BN of every residual
    branch at gamma 0 (timm's zero_init_last).  scale="unit": BN running means N(0, 0.1), running variances U(0.5, 1.5), betas N(0, 0.1),
    gammas U(0.5, 1.5) except the last BN of a branch, U(0.2, 0.5) — so that the 16 residual additions keep the stream within a few
    units, as a trained network's does, instead of doubling its variance per block."""
    g = torch.Generator(device="cpu")
    g.manual_seed((int(seed) * 0x9E3779B1 + 0x7265736E) % (1 << 63))
    last = "bn3" if RESNET_CFG[arch][2] == "bottleneck" else "bn2"
    sd = OrderedDict()
    for k, shp in param_shapes(arch, img_size).items():
        leaf = k.rsplit(".", 1)[-1]
        bn = k.rsplit(".", 1)[0].rsplit(".", 1)[-1]
        if len(shp) == 4:
            v = torch.randn(shp, generator=g, dtype=torch.float32) * math.sqrt(2.0 / (shp[1] * shp[2] * shp[3]))
        elif scale == "timm":
            if leaf in ("bias", "running_mean"):
                v = torch.zeros(shp)
            elif leaf == "running_var":
                v = torch.ones(shp)
            else:
                v = torch.zeros(shp) if bn == last else torch.ones(shp)
        elif leaf == "running_var":
            v = torch.rand(shp, generator=g, dtype=torch.float32) + 0.5
        elif leaf in ("bias", "running_mean"):
            v = torch.randn(shp, generator=g, dtype=torch.float32) * 0.1
        elif bn == last:
            v = torch.rand(shp, generator=g, dtype=torch.float32) * 0.3 + 0.2
        else:
            v = torch.rand(shp, generator=g, dtype=torch.float32) + 0.5
        sd[k] = v.contiguous()
    return sd


def init_head(arch, num_classes, seed=0, scale="unit"):
    """Seeded classifier head from a CPU Philox generator of its own (seeded from ``seed`` and the tag 0x68656164): scale="unit"
    gives weights N(0, 1/D) and biases N(0, 0.1), so logits are O(1) for O(1) embeddings; scale="timm" gives timm's
    trunc_normal(0.02) weight and zero bias."""
    g = torch.Generator(device="cpu")
    g.manual_seed((int(seed) * 0x9E3779B1 + 0x68656164) % (1 << 63))
    out = OrderedDict()
    if arch in LEVIT_CFG:
        # two BatchNorm1d + Linear heads: scale="unit" gives both non-trivial statistics and affine terms; scale="timm" BN at identity
        for k, shp in head_shapes(arch, num_classes).items():
            leaf = k.rsplit(".", 1)[-1]
            if len(shp) == 2:
                v = (torch.randn(shp, generator=g, dtype=torch.float32) * 0.02).clamp_(-0.04, 0.04) if scale == "timm" else \
                    torch.randn(shp, generator=g, dtype=torch.float32) / math.sqrt(shp[1])
            elif scale == "timm":
                v = torch.ones(shp) if (leaf in ("weight", "running_var") and ".bn." in k) else torch.zeros(shp)
            elif leaf == "running_var" or (leaf == "weight" and ".bn." in k):
                v = torch.rand(shp, generator=g, dtype=torch.float32) + 0.5
            else:
                v = torch.randn(shp, generator=g, dtype=torch.float32) * 0.1
            out[k] = v.contiguous()
        return out
    (wk, wshape), (bk, bshape) = head_shapes(arch, num_classes).items()
    if scale == "timm":
        out[wk] = (torch.randn(wshape, generator=g, dtype=torch.float32) * 0.02).clamp_(-0.04, 0.04).contiguous()
        out[bk] = torch.zeros(bshape)
    else:
        out[wk] = (torch.randn(wshape, generator=g, dtype=torch.float32) / math.sqrt(wshape[1])).contiguous()
        out[bk] = (torch.randn(bshape, generator=g, dtype=torch.float32) * 0.1).contiguous()
    return out


def infer_num_classes(sd):
    """Classes of the timm classifier head a checkpoint carries (rows of its head weight), 0 when it has none."""
    sd = strip_prefix(sd)
    for wk, bk in HEAD_KEYS.values():
        if wk in sd and bk in sd and (sd[wk].dim() == 2 or (sd[wk].dim() == 4 and tuple(sd[wk].shape[2:]) == (1, 1))):
            return int(sd[wk].shape[0])
    return 0


def strip_prefix(sd, prefix="net."):
    """models/encoders.py:60 keeps the timm module as ``self.net`` -> keys ``net.<timm key>``.  A Swin state dict also comes out in
    timm >= 0.9's layout (swin_canonical) and a BEiT state dict without its derived buffers; every other state dict only loses the prefix."""
    keys = list(sd.keys())
    if keys and all(k.startswith(prefix) for k in keys):
        sd = OrderedDict((k[len(prefix):], v) for k, v in sd.items())
    if "layers.0.blocks.0.attn.relative_position_bias_table" in sd:
        return swin_canonical(sd)
    if any(".mlp.dwconv.dwconv." in k for k in sd):
        # PVTv2: the original repository wraps the depthwise convolution in a module of its own (mlp.dwconv.dwconv.*)
        return OrderedDict((k.replace(".mlp.dwconv.dwconv.", ".mlp.dwconv."), v) for k, v in sd.items())
    if "blocks.0.attn.relative_position_bias_table" in sd:
        # BEiT: the derived buffers of older timm checkpoints are dropped (the kernels compute the index from the geometry; k_bias is zeros)
        return OrderedDict((k, v) for k, v in sd.items() if not k.endswith((".attn.relative_position_index", ".attn.k_bias")))
    return OrderedDict(sd)


_SWIN_OLD_DOWNSAMPLE = re.compile(r"^layers\.(\d+)\.downsample\.")


def swin_canonical(sd):
    """A Swin state dict in timm >= 0.9's layout.  timm < 0.9 keeps the patch merging at the END of stages 0-2 (``layers.i.downsample``,
    i = 0..2) and names the classifier ``head``; timm >= 0.9 keeps it at the START of stages 1-3 and names the classifier ``head.fc``.
    The layouts are told apart by the downsample indices (a ``layers.0.downsample`` exists only in the old one).  The derived buffers
    ``relative_position_index`` and ``attn_mask`` are dropped: the kernels compute both from the geometry."""
    old = any(k.startswith("layers.0.downsample.") for k in sd)
    out = OrderedDict()
    for k, v in sd.items():
        if k.endswith((".relative_position_index", ".attn_mask")):
            continue
        if old:
            m = _SWIN_OLD_DOWNSAMPLE.match(k)
            if m:
                k = f"layers.{int(m.group(1)) + 1}.downsample." + k[m.end():]
            elif k in ("head.weight", "head.bias"):
                k = "head.fc." + k[len("head."):]
        out[k] = v
    return out


def load_checkpoint(path):
    """Read encoder weights the way ``AutoEncoder.load`` does (models/encoders.py:66-70), but with
    ``map_location='cpu'`` so that it works on any box; also accepts ``.safetensors``."""
    path = str(path)
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(path)
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
    return strip_prefix(sd)


def save_checkpoint(sd, path, prefix="net."):
    """Write a state dict with the reference's ``net.`` key prefix (train_effocr_recognizer.py:65-72)."""
    out = OrderedDict((prefix + k, v.detach().cpu().contiguous()) for k, v in strip_prefix(sd).items())
    path = str(path)
    if path.endswith(".safetensors"):
        from safetensors.torch import save_file
        save_file(out, path)
    else:
        torch.save(out, path)


def beit_img_size(sd):
    """Crop size a BEiT checkpoint was built for, from the length (2W-1)^2 + 3 of its bias tables (W = img_size / 16 patches per side)."""
    n = int(strip_prefix(sd)["blocks.0.attn.relative_position_bias_table"].shape[0])
    w2 = math.isqrt(max(n - 3, 0))
    if n < 4 or w2 * w2 != n - 3 or w2 % 2 == 0 or (w2 + 1) // 2 > 224 // PATCH:
        raise ValueError(f"unsupported BEiT: a relative_position_bias_table of {n} rows is not (2W-1)^2 + 3 for a patch grid W <= 14")
    return (w2 + 1) // 2 * PATCH


def vit8_img_size(sd):
    """Crop size a patch-8 ViT checkpoint was built for, from the (img_size / 8)^2 + 1 rows of its ``pos_embed``."""
    n = int(strip_prefix(sd)["pos_embed"].shape[-2])
    w = math.isqrt(max(n - 1, 0))
    if n < 2 or w * w != n - 1 or w > 224 // VIT8_PATCH:
        raise ValueError(f"unsupported patch-8 ViT: a pos_embed of {n} rows is not W^2 + 1 for a patch grid W <= 28")
    return w * VIT8_PATCH


def levit_img_size(sd):
    """Crop size a LeViT checkpoint was built for: the first block's ``attention_biases`` has one column per (|dy|, |dx|) offset of the
    (img_size / 16)^2 token grid."""
    n = int(strip_prefix(sd)["stages.0.blocks.0.attn.attention_biases"].shape[-1])
    r = math.isqrt(n)
    if r * r != n or not 2 <= r <= 14:
        raise ValueError(f"unsupported LeViT: attention_biases of {n} columns is not R^2 for a token grid 2 <= R <= 14")
    return 16 * r


def _infer_regnet(sd):
    """The RegNet a checkpoint holds: se.fc1 tells Y from X; the stage widths, the depths and conv2's second dimension (the group width)
    pick the name, and every shape must then match.  Anything else is a ValueError that lists the supported names."""
    supported = "supported: " + ", ".join(REGNET_SUPPORTED)
    se = "s1.b1.se.fc1.weight" in sd
    depths = tuple(max((int(k.split(".")[1][1:]) for k in sd if k.startswith(f"s{i}.b") and k.split(".")[1][1:].isdigit()), default=0)
                   for i in range(1, 5))
    widths = tuple(int(sd[f"s{i}.b1.conv1.conv.weight"].shape[0]) if f"s{i}.b1.conv1.conv.weight" in sd else -1 for i in range(1, 5))
    c2 = sd.get("s1.b1.conv2.conv.weight")
    gw = int(c2.shape[1]) if c2 is not None and c2.dim() == 4 else -1
    kind = "RegNetY" if se else "RegNetX"
    for name in tuple(REGNET_CFG) + tuple(REGNET_MINI):
        w, d, g, s = regnet_arch(name)
        if (w, d, g, s) != (widths, depths, gw, se):
            continue
        want = _regnet_shapes(name)
        bad = [k for k, shp in want.items() if k not in sd or tuple(sd[k].shape) != shp]
        extra = [k for k in sd if ".se." in k and k not in want]
        if bad or extra:
            raise ValueError(f"unsupported RegNet: widths {widths}, depths {depths} and group width {gw} are {name}'s, but "
                             f"{(bad + extra)[0]} does not fit it ({supported})")
        return name
    if not se and any(".se." in k for k in sd):
        kind = "RegNetX with squeeze-excite keys"
    raise ValueError(f"unsupported RegNet: {kind}, widths {widths}, depths {depths}, group width {gw} ({supported})")


def _infer_pvt(sd):
    """The PVTv2 a checkpoint holds: C0 and the depths pick the name, then every shape must match.  Pooled "linear" attention (attn.pool),
    PVT v1 (position embeddings; no reduction in the overlapping form) and anything else is a ValueError that lists the supported names."""
    supported = "supported: " + ", ".join(PVT_SUPPORTED)
    if any(".attn.pool." in k for k in sd):
        raise ValueError(f"unsupported PVT: pooled linear attention (pvt_v2_b2_li: attn.pool keys) ({supported})")
    if any(k.startswith("pos_embed") or ".pos_embed" in k or k.startswith("cls_token") for k in sd):
        raise ValueError(f"unsupported PVT: position embeddings (PVT v1) ({supported})")
    pw = sd.get("patch_embed.proj.weight")
    if "stages.0.blocks.0.attn.sr.weight" not in sd or pw is None or pw.dim() != 4 or tuple(pw.shape[1:]) != (3, 7, 7):
        raise ValueError(f"unsupported PVT: no stage-0 spatial reduction (attn.sr) behind a 7x7 patch embedding ({supported})")
    c0 = int(pw.shape[0])
    depths = tuple(1 + max((int(k.split(".")[3]) for k in sd if k.startswith(f"stages.{i}.blocks.")), default=-1) for i in range(4))
    first_bad = None
    for name, (widths, _, dep, _) in PVT_CFG.items():
        if widths[0] != c0 or dep != depths:
            continue
        bad = [k for k, shp in _pvt_shapes(name).items() if k not in sd or tuple(sd[k].shape) != shp]
        if not bad:
            return name
        first_bad = first_bad or (name, bad[0])
    if first_bad:
        raise ValueError(f"unsupported PVT: stem width {c0} and depths {depths} are {first_bad[0]}'s, but {first_bad[1]} does not fit it ({supported})")
    raise ValueError(f"unsupported PVT: stem width {c0}, depths {depths} ({supported})")


def infer_arch(sd):
    """Guess the architecture of a checkpoint from its parameter shapes."""
    sd = strip_prefix(sd)
    if any(k in sd for k in ("stages.0.blocks.0.attn.sr.weight", "stages.0.blocks.0.attn.kv.weight", "stages.0.blocks.0.attn.pool.weight")):
        return _infer_pvt(sd)                              # PVTv2 (before the pos_embed branch: a PVT with position embeddings is refused there)
    if "stem.conv1.linear.weight" in sd or "patch_embed.0.c.weight" in sd:
        # LeViT: the shapes at the checkpoint's own crop size name the model
        supported = "supported: " + ", ".join(LEVIT_SUPPORTED) + " in timm >= 0.9's key layout"
        if "stem.conv1.linear.weight" not in sd:
            raise ValueError(f"unsupported LeViT: the flat key layout of timm < 0.9 (patch_embed.0.c.weight, blocks.N.m.*) ({supported})")
        qkv = sd.get("stages.0.blocks.0.attn.qkv.linear.weight")
        if qkv is None or qkv.dim() != 2:
            raise ValueError(f"unsupported LeViT: a convolutional variant (levit_conv_*) or an unknown layout ({supported})")
        img = levit_img_size(sd)
        for name in LEVIT_CFG:
            want = param_shapes(name, img)
            if all(k in sd and tuple(sd[k].shape) == shp for k, shp in want.items()):
                return name
        raise ValueError(f"unsupported LeViT: stem width {int(sd['stem.conv4.linear.weight'].shape[0])} with these block shapes matches "
                         f"no supported model ({supported})")
    if "s1.b1.conv1.conv.weight" in sd:
        return _infer_regnet(sd)
    if "conv1.weight" in sd and "layer4.0.conv1.weight" in sd:
        # every ResNet has conv1 and layer4: the depth of layer3 and conv3 (Bottleneck) tell them apart
        depths = tuple(1 + max((int(k.split(".")[1]) for k in sd if k.startswith(f"layer{i}.")), default=-1) for i in range(1, 5))
        block = "bottleneck" if "layer1.0.conv3.weight" in sd else "basic"
        for name, (dep, _, blk) in RESNET_CFG.items():
            if dep == depths and blk == block:
                return name
        raise ValueError(f"unsupported ResNet: {block} blocks, depths {depths} (supported: "
                         + ", ".join(f"{n} {c[2]} {c[0]}" for n, c in RESNET_CFG.items()) + ")")
    if "stem.conv.weight" in sd and "stages.3.blocks.0.conv3.weight" in sd and "stages.0.blocks.0.norm1.weight" in sd:
        # BiT ResNetV2 (pre-activation bottlenecks; ConvNeXt's stem is stem.0): the depths tell 50 from 101, the shapes pin the width
        depths = tuple(1 + max((int(k.split(".")[3]) for k in sd if k.startswith(f"stages.{i}.blocks.")), default=-1) for i in range(4))
        for name, dep in BIT_CFG.items():
            want = _bit_shapes(name)
            if dep == depths and all(k in sd and tuple(sd[k].shape) == shp for k, shp in want.items()):
                return name
        width = int(sd["stages.0.blocks.0.conv3.weight"].shape[0]) // 256
        raise ValueError(f"unsupported BiT ResNetV2: depths {depths}, width factor {width} (supported: resnetv2_50x1_bitm (3, 4, 6, 3) and "
                         "resnetv2_101x1_bitm (3, 4, 23, 3), width factor 1)")
    if "pos_embed" in sd:
        D = sd["pos_embed"].shape[-1]
        depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
        pw = sd.get("patch_embed.proj.weight")
        if pw is not None and pw.dim() == 4 and int(pw.shape[-1]) == VIT8_PATCH:
            # the same keys as the patch-16 ViTs: the kernel size of the patch conv tells them apart
            for name, (d, dep, _, _) in VIT8_CFG.items():
                if d == D and dep == depth:
                    return name
            raise ValueError(f"unsupported patch-8 ViT: width {D}, depth {depth} (supported: small, width 384, and base, width 768, depth 12)")
        for name, (d, dep, _, _) in VIT_CFG.items():
            if d == D and dep == depth:
                return name
    if ("cls_token" in sd and "blocks.0.attn.relative_position_bias_table" in sd and "blocks.0.gamma_1" in sd
            and "fc_norm.weight" in sd):
        # BEiT (no pos_embed: the ViT branch above did not take it).  beitv2_base_patch16_224 has the same keys and shapes and must be
        # named by the caller
        img = beit_img_size(sd)
        D = int(sd["cls_token"].shape[-1])
        depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
        for name, (d, dep, _, _) in BEIT_CFG.items():
            if d == D and dep == depth:
                check_state_dict(name, sd, img)
                return name
        raise ValueError(f"unsupported BEiT: width {D}, depth {depth} (supported: base, width 768, depth 12)")
    if "stem.0.weight" in sd and any(k.startswith("stages.3.blocks.") for k in sd):
        depths = tuple(1 + max((int(k.split(".")[3]) for k in sd if k.startswith(f"stages.{i}.blocks.")), default=-1)
                       for i in range(4))
        widths = tuple(int(sd[f"stages.{i}.blocks.0.gamma"].shape[0]) if f"stages.{i}.blocks.0.gamma" in sd else -1
                       for i in range(4))
        for name, (dep, wid) in CONVNEXT_CFG.items():
            if dep == depths and wid == widths:
                return name
    if "patch_embed.proj.weight" in sd and "layers.0.blocks.0.attn.relative_position_bias_table" in sd:
        for name in SWIN_CFG:
            want = param_shapes(name)
            if all(k in sd and tuple(sd[k].shape) == shp for k, shp in want.items()):
                return name
    if ("conv_stem.weight" in sd and "conv_head.weight" in sd and "bn2.weight" in sd and "conv_head.bias" not in sd
            and sd["conv_stem.weight"].shape[0] == EFFICIENTNET_STEM):
        # conv_head without a bias, followed by bn2, behind a 32-channel stem: EfficientNet.  tf_efficientnet_b0 has the same keys and
        # shapes (it differs in BN eps and padding) and must be named by the caller
        want = param_shapes("efficientnet_b0")
        if all(k in sd and tuple(sd[k].shape) == shp for k, shp in want.items()):
            return "efficientnet_b0"
        raise ValueError("unsupported EfficientNet: only efficientnet_b0 / tf_efficientnet_b0 shapes are supported")
    if "conv_stem.weight" in sd and "conv_head.weight" in sd:
        # Large has a seventh stage (blocks.6.0, the 960-wide ConvBnAct), Small ends at blocks.5.0; the width follows from the shapes
        large = "blocks.6.0.conv.weight" in sd
        for name in MOBILENETV3_CFG:
            if is_mobilenetv3_large(name) != large:
                continue
            want = param_shapes(name)
            if all(k in sd and tuple(sd[k].shape) == shp for k, shp in want.items()):
                return name
    raise ValueError("cannot infer encoder architecture from checkpoint keys")


def check_state_dict(arch, sd, img_size=224, num_classes=0):
    """Raise ValueError listing missing / mis-shaped parameters (num_batches_tracked etc. ignored); with ``num_classes`` > 0 the
    classifier head is required too."""
    want = param_shapes(arch, img_size, num_classes)
    bad = []
    for k, shp in want.items():
        if k not in sd:
            bad.append(f"missing {k}")
        elif arch in BIT_CFG and k == "head.fc.weight" and tuple(sd[k].shape) == tuple(shp[:2]):
            continue                                   # the 1x1-conv head as a matrix [N, 2048] is accepted too
        elif tuple(sd[k].shape) != tuple(shp):
            bad.append(f"{k}: shape {tuple(sd[k].shape)} != {tuple(shp)}")
    if bad:
        raise ValueError(f"state dict does not match {arch}: " + "; ".join(bad[:8]) +
                         (f" (+{len(bad) - 8} more)" if len(bad) > 8 else ""))
