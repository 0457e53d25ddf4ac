"""EfficientNet-B0 host side (-m "not gpu"): efficientnet_b0 / tf_efficientnet_b0 — the builder against timm's published parameter
counts and against transformers.EfficientNetModel's shapes, the hand-written float64 restatement (tests/efficientnet_ref.py) pinned
to transformers.EfficientNetModel (tf_ variant) and to an nn.Module tree built from the builder (plain variant), architecture inference,
checkpoint I/O, the factories, and the C ABI of libeffocr_effnet.so up to the device — none of it needs a GPU."""
import ctypes
import math
from collections import Counter

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from effocr_amd import _lib
from effocr_amd import weights as W
from tests.efficientnet_ref import efficientnet_forward

ARCHS = ["efficientnet_b0", "tf_efficientnet_b0"]
COUNT, COUNT_1000 = 4_007_548, 5_288_548      # learnable parameters without / with a 1000-class classifier (timm's published 5.29 M with it)
SE_WIDTHS = [8, 4, 6, 6, 10, 10, 20, 20, 20, 28, 28, 28, 48, 48, 48, 48]
_BN = ("weight", "bias", "running_mean", "running_var")


# ---------------------------------------------------------------------------------------------------- the builder
@pytest.mark.parametrize("arch", ARCHS)
def test_block_table_and_counts(arch):
    stem, blocks, nf = W.efficientnet_blocks(arch)
    assert stem == 32 and nf == 1280 and W.embed_dim(arch) == 1280 and len(blocks) == 16
    assert [b["key"] for b in blocks] == ["blocks.0.0", "blocks.1.0", "blocks.1.1", "blocks.2.0", "blocks.2.1", "blocks.3.0", "blocks.3.1",
                                          "blocks.3.2", "blocks.4.0", "blocks.4.1", "blocks.4.2", "blocks.5.0", "blocks.5.1", "blocks.5.2",
                                          "blocks.5.3", "blocks.6.0"]
    assert [b["se"] for b in blocks] == SE_WIDTHS
    assert [b["type"] for b in blocks] == ["ds"] + ["ir"] * 15
    assert [b["mid"] for b in blocks] == [32, 96, 144, 144, 240, 240, 480, 480, 480, 672, 672, 672, 1152, 1152, 1152, 1152]
    assert [b["k"] for b in blocks] == [3, 3, 3, 5, 5, 3, 3, 3, 5, 5, 5, 5, 5, 5, 5, 3]
    assert [b["stride"] for b in blocks] == [1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1]
    assert [b["res"] for b in blocks] == [False, False, True, False, True, False, True, True, False, True, True, False, True, True, True, False]
    assert W.efficientnet_num_learnable(arch) == COUNT
    assert W.efficientnet_num_learnable(arch, num_classes=1000) == COUNT_1000
    shapes = W.param_shapes(arch)
    assert shapes["conv_head.weight"] == (1280, 320, 1, 1) and "conv_head.bias" not in shapes and shapes["bn2.running_var"] == (1280,)
    assert list(shapes)[-5:] == ["conv_head.weight", "bn2.weight", "bn2.bias", "bn2.running_mean", "bn2.running_var"]
    assert shapes["blocks.0.0.conv_pw.weight"] == (16, 32, 1, 1) and "blocks.0.0.conv_pwl.weight" not in shapes
    assert W.head_shapes(arch, 7) == {"classifier.weight": (7, 1280), "classifier.bias": (7,)}
    assert list(W.param_shapes(arch, num_classes=7))[-2:] == ["classifier.weight", "classifier.bias"]


def test_macs_are_the_published_figure():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("efficientnet_time", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools",
                                                                                      "efficientnet_time.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    macs = tool.macs_per_crop("efficientnet_b0")
    assert 0.38e9 < macs < 0.40e9, macs                    # "0.39 GMAC" per 224^2 crop
    assert tool.macs_per_crop("tf_efficientnet_b0") == macs


# ---------------------------------------------------------------------------------------------------- transformers.EfficientNetModel
def hf_name_map():
    """{timm key: transformers.EfficientNetModel key} for every parameter and BN buffer of EfficientNet-B0."""
    m = {"conv_stem.weight": "embeddings.convolution.weight", "conv_head.weight": "encoder.top_conv.weight"}
    for leaf in _BN:
        m[f"bn1.{leaf}"] = f"embeddings.batchnorm.{leaf}"
        m[f"bn2.{leaf}"] = f"encoder.top_bn.{leaf}"
    for i, b in enumerate(W.efficientnet_blocks("efficientnet_b0")[1]):
        t, h = b["key"], f"encoder.blocks.{i}"
        ds = b["type"] == "ds"
        if not ds:
            m[f"{t}.conv_pw.weight"] = f"{h}.expansion.expand_conv.weight"
        m[f"{t}.conv_dw.weight"] = f"{h}.depthwise_conv.depthwise_conv.weight"
        m[f"{t}.{'conv_pw' if ds else 'conv_pwl'}.weight"] = f"{h}.projection.project_conv.weight"
        for leaf in _BN:
            if not ds:
                m[f"{t}.bn1.{leaf}"] = f"{h}.expansion.expand_bn.{leaf}"
            m[f"{t}.{'bn1' if ds else 'bn2'}.{leaf}"] = f"{h}.depthwise_conv.depthwise_norm.{leaf}"
            m[f"{t}.{'bn2' if ds else 'bn3'}.{leaf}"] = f"{h}.projection.project_bn.{leaf}"
        for leaf in ("weight", "bias"):
            m[f"{t}.se.conv_reduce.{leaf}"] = f"{h}.squeeze_excite.reduce.{leaf}"
            m[f"{t}.se.conv_expand.{leaf}"] = f"{h}.squeeze_excite.expand.{leaf}"
    return m


@pytest.fixture(scope="module")
def hf_model():
    from transformers import EfficientNetConfig, EfficientNetModel
    cfg = EfficientNetConfig(width_coefficient=1.0, depth_coefficient=1.0, image_size=224, hidden_dim=1280)
    assert cfg.batch_norm_eps == 1e-3
    return EfficientNetModel(cfg).double().eval()


def test_shapes_equal_transformers(hf_model):
    hf = {k: tuple(v.shape) for k, v in hf_model.state_dict().items() if not k.endswith("num_batches_tracked")}
    assert sum(p.numel() for p in hf_model.parameters()) == COUNT
    ours = W.param_shapes("tf_efficientnet_b0")
    assert Counter(hf.values()) == Counter(ours.values())                 # the same multiset of shapes
    nm = hf_name_map()
    assert sorted(nm) == sorted(ours) and sorted(nm.values()) == sorted(hf)     # a bijection between the two key sets
    assert all(ours[k] == hf[v] for k, v in nm.items())
    for i, r in enumerate(SE_WIDTHS):
        assert hf[f"encoder.blocks.{i}.squeeze_excite.reduce.weight"][0] == r


@pytest.mark.parametrize("img,B", [(64, 2), (96, 1)])
def test_pin_against_transformers(hf_model, img, B):
    sd = W.init_state_dict("tf_efficientnet_b0", seed=11, img_size=img)          # "unit": random non-trivial BN statistics
    assert sd["blocks.3.1.bn2.running_mean"].abs().max() > 0.01 and (sd["bn2.running_var"] - 1).abs().max() > 0.1
    tracked = {k: v for k, v in hf_model.state_dict().items() if k.endswith("num_batches_tracked")}
    hf_model.load_state_dict({**tracked, **{v: sd[k].double() for k, v in hf_name_map().items()}}, strict=True)
    x = torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(img), dtype=torch.float64)
    with torch.no_grad():
        want = hf_model(x).pooler_output
    got = efficientnet_forward("tf_efficientnet_b0", sd, x)
    assert got.shape == want.shape == (B, 1280) and got.dtype == torch.float64
    rel = ((got - want).abs().max() / want.abs().max()).item()
    print(f"tf_efficientnet_b0 restatement vs transformers.EfficientNetModel at {img}^2: {rel:.2e}")
    assert rel <= 1e-10
    assert want.abs().max() > 1e-3
    # each flag on its own must do something: SAME -> symmetric padding at the same eps, and eps 1e-3 -> 1e-5 at the same padding
    pad_only = efficientnet_forward("tf_efficientnet_b0", sd, x, tf=False)
    eps_only = efficientnet_forward("tf_efficientnet_b0", sd, x, eps=1e-5)
    d_pad, d_eps = (((o - want).abs().max() / want.abs().max()).item() for o in (pad_only, eps_only))
    print(f"padding alone moves the output by {d_pad:.2e}, eps alone by {d_eps:.2e}")
    assert d_pad > 1e-3 and d_eps > 1e-4
    assert torch.equal(efficientnet_forward("efficientnet_b0", sd, x), efficientnet_forward("tf_efficientnet_b0", sd, x, tf=False, eps=1e-5))


# ---------------------------------------------------------------------------------------------------- the nn.Module restatement
class _SE(nn.Module):
    def __init__(self, c, r):
        super().__init__()
        self.conv_reduce = nn.Conv2d(c, r, 1, bias=True)
        self.conv_expand = nn.Conv2d(r, c, 1, bias=True)

    def forward(self, x):
        return x * torch.sigmoid(self.conv_expand(F.silu(self.conv_reduce(x.mean((2, 3), keepdim=True)))))


class _Block(nn.Module):
    """One entry of weights.efficientnet_blocks as timm's DepthwiseSeparableConv / InvertedResidual (symmetric padding, eps 1e-5)."""

    def __init__(self, b):
        super().__init__()
        self.t, self.res = b["type"], b["res"]
        k, s = b["k"], b["stride"]
        if self.t == "ds":
            self.conv_dw = nn.Conv2d(b["cin"], b["cin"], k, s, k // 2, groups=b["cin"], bias=False)
            self.bn1 = nn.BatchNorm2d(b["cin"], eps=1e-5)
            self.se = _SE(b["cin"], b["se"])
            self.conv_pw = nn.Conv2d(b["cin"], b["cout"], 1, bias=False)
            self.bn2 = nn.BatchNorm2d(b["cout"], eps=1e-5)
        else:
            self.conv_pw = nn.Conv2d(b["cin"], b["mid"], 1, bias=False)
            self.bn1 = nn.BatchNorm2d(b["mid"], eps=1e-5)
            self.conv_dw = nn.Conv2d(b["mid"], b["mid"], k, s, k // 2, groups=b["mid"], bias=False)
            self.bn2 = nn.BatchNorm2d(b["mid"], eps=1e-5)
            self.se = _SE(b["mid"], b["se"])
            self.conv_pwl = nn.Conv2d(b["mid"], b["cout"], 1, bias=False)
            self.bn3 = nn.BatchNorm2d(b["cout"], eps=1e-5)

    def forward(self, x):
        if self.t == "ds":
            y = self.bn2(self.conv_pw(self.se(F.silu(self.bn1(self.conv_dw(x))))))
        else:
            y = F.silu(self.bn1(self.conv_pw(x)))
            y = self.bn3(self.conv_pwl(self.se(F.silu(self.bn2(self.conv_dw(y))))))
        return y + x if self.res else y


class _EfficientNet(nn.Module):
    def __init__(self, arch):
        super().__init__()
        stem, blocks, nf = W.efficientnet_blocks(arch)
        self.conv_stem = nn.Conv2d(3, stem, 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(stem, eps=1e-5)
        stages = {}
        for b in blocks:
            stages.setdefault(int(b["key"].split(".")[1]), []).append(_Block(b))
        self.blocks = nn.Sequential(*[nn.Sequential(*stages[i]) for i in sorted(stages)])
        self.conv_head = nn.Conv2d(blocks[-1]["cout"], nf, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(nf, eps=1e-5)

    def forward(self, x):
        x = self.blocks(F.silu(self.bn1(self.conv_stem(x))))
        return F.silu(self.bn2(self.conv_head(x))).mean((2, 3))


@pytest.mark.parametrize("img,B", [(64, 2), (32, 3)])
def test_restatement_equals_module_tree(img, B):
    arch = "efficientnet_b0"
    sd = W.init_state_dict(arch, seed=5, img_size=img)
    m = _EfficientNet(arch).double().eval()
    assert sum(p.numel() for p in m.parameters()) == COUNT
    full = dict(sd)
    for k in list(sd):
        if k.endswith(".running_var"):                  # a real checkpoint carries these; loading ignores their values
            full[k[: -len("running_var")] + "num_batches_tracked"] = torch.tensor(0)
    m.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in full.items()}, strict=True)
    x = torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(img), dtype=torch.float64)
    ref = efficientnet_forward(arch, sd, x)
    with torch.no_grad():
        mod = m(x)
    rel = ((ref - mod).abs().max() / ref.abs().max()).item()
    print(f"efficientnet_b0: functional vs nn.Module restatement at {img}^2: {rel:.2e}")
    assert ref.shape == (B, 1280) and rel <= 1e-12 and ref.abs().max() > 1e-3
    # same weights and eps, SAME padding instead of symmetric: the module tree pins the padding flag on its own
    pad_only = efficientnet_forward("efficientnet_b0", sd, x, tf=True)
    assert ((pad_only - ref).abs().max() / ref.abs().max()).item() > 1e-3


def test_rounded_pointwise_restatement_is_close_to_exact():
    """The restatement's round_pw path (the GPU test's e_w) folds BN into the weights: with no rounding to speak of it must give the
    plain path's result."""
    sd = W.init_state_dict("tf_efficientnet_b0", seed=2, img_size=32)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    a = efficientnet_forward("tf_efficientnet_b0", sd, x)
    b = efficientnet_forward("tf_efficientnet_b0", sd, x, round_pw=torch.float32)
    c = efficientnet_forward("tf_efficientnet_b0", sd, x, round_pw=torch.bfloat16)
    assert ((a - b).abs().max() / a.abs().max()).item() < 1e-5
    assert 1e-5 < ((a - c).abs().max() / a.abs().max()).item() < 0.1


# ---------------------------------------------------------------------------------------------------- tables, I/O, init
def test_init_is_seeded_and_deterministic():
    a = W.init_state_dict("efficientnet_b0", seed=4, img_size=64)
    b = W.init_state_dict("tf_efficientnet_b0", seed=4, img_size=224)
    c = W.init_state_dict("efficientnet_b0", seed=5)
    assert list(a) == list(b) == list(W.param_shapes("efficientnet_b0"))
    assert all(torch.equal(a[k], b[k]) for k in a) and any(not torch.equal(a[k], c[k]) for k in a)
    t = W.init_state_dict("efficientnet_b0", seed=4, scale="timm")
    assert torch.equal(t["bn2.running_var"], torch.ones(1280)) and torch.equal(t["blocks.3.0.se.conv_reduce.bias"], torch.zeros(10))
    h = W.init_state_dict("efficientnet_b0", seed=4, num_classes=9)
    assert all(torch.equal(a[k], h[k]) for k in a) and tuple(h["classifier.weight"].shape) == (9, 1280)


def test_check_state_dict_and_infer_arch():
    arch = "efficientnet_b0"
    sd = W.init_state_dict(arch, seed=0)
    for a in ARCHS:
        W.check_state_dict(a, sd)
    assert W.infer_arch(sd) == arch                         # the tf_ variant cannot be told from a checkpoint: it must be named
    assert W.infer_arch({"net." + k: v for k, v in sd.items()}) == arch
    tracked = dict(sd)
    tracked["bn1.num_batches_tracked"] = torch.tensor(7)
    W.check_state_dict(arch, tracked)                       # ignored
    assert W.infer_arch(tracked) == arch
    with_head = W.init_state_dict(arch, seed=0, num_classes=11)
    assert W.infer_arch(with_head) == arch and W.infer_num_classes(with_head) == 11
    W.check_state_dict(arch, with_head, num_classes=11)
    with pytest.raises(ValueError, match="classifier.weight"):
        W.check_state_dict(arch, sd, num_classes=11)
    bad = dict(sd)
    bad["blocks.2.1.se.conv_reduce.weight"] = torch.zeros(60, 240, 1, 1)          # the width MobileNetV3's rule would give
    with pytest.raises(ValueError, match="blocks.2.1.se.conv_reduce.weight"):
        W.check_state_dict(arch, bad)
    with pytest.raises(ValueError, match="missing bn2.running_mean"):
        W.check_state_dict(arch, {k: v for k, v in sd.items() if k != "bn2.running_mean"})
    with pytest.raises(ValueError):
        W.infer_arch({k: v for k, v in sd.items() if not k.startswith("blocks.5.3.")})       # (what efficientnet_b1 is not, either)
    assert W.infer_arch(W.init_state_dict("mobilenetv3_large_100", seed=0)) == "mobilenetv3_large_100"


@pytest.mark.parametrize("ext", ["pth", "safetensors"])
@pytest.mark.parametrize("arch", ARCHS)
def test_checkpoint_round_trip_and_factory(arch, ext, tmp_path):
    from effocr_amd.encoders import AutoEncoderFactory
    sd = W.init_state_dict(arch, seed=2)
    path = tmp_path / f"enc_best.{ext}"
    W.save_checkpoint(sd, path)
    if ext == "pth":
        assert all(k.startswith("net.") for k in torch.load(path, weights_only=True))
    back = W.load_checkpoint(path)
    assert sorted(back) == sorted(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    cls = AutoEncoderFactory("timm", arch)
    assert cls.arch == arch
    params = list(cls().named_parameters())
    assert all(k.startswith("net.") for k, _ in params) and sum(p.numel() for _, p in params) == COUNT
    got = cls.load(str(path)).state_dict()                 # CPU only: the engine is built on first forward
    assert all(torch.equal(got["net." + k], v) for k, v in sd.items())
    wrong = dict(sd)
    wrong["conv_head.weight"] = torch.zeros(1280, 192, 1, 1)
    with pytest.raises(ValueError, match="conv_head.weight"):
        cls().load_state_dict(wrong)


def test_classifier_factory_loads_a_head(tmp_path):
    from effocr_amd.classifiers import AutoClassifierFactory
    arch = "tf_efficientnet_b0"
    sd = W.init_state_dict(arch, seed=3, num_classes=7)
    path = tmp_path / "clf.pth"
    W.save_checkpoint(sd, path)
    cls = AutoClassifierFactory("timm", arch, n_classes=7)
    clf = cls.load(str(path))
    assert cls.num_classes == 7 and torch.equal(clf.state_dict()["net.classifier.weight"], sd["classifier.weight"])
    assert sum(p.numel() for p in clf.parameters()) == COUNT + 7 * 1280 + 7
    with pytest.raises(ValueError, match="classifier"):
        cls().load_state_dict(W.init_state_dict(arch, seed=3))          # an encoder-only checkpoint has no head


def test_dispatch_and_refusals():
    from effocr_amd import encoders as E
    from effocr_amd.classifiers import AutoClassifierFactory
    assert all(W.is_efficientnet(a) for a in ARCHS) and not W.is_efficientnet("mobilenetv3_large_100") and not W.is_mnv3_lib(ARCHS[0])
    assert issubclass(E.EfficientNetEncoder, E.HipEncoder)
    for name in ("efficientnet_b1", "efficientnet_lite0", "tf_efficientnet_b0_ns", "efficientnetv2_s", "efficientnet_b0_ap"):
        with pytest.raises(NotImplementedError):
            W.embed_dim(name)
        with pytest.raises(NotImplementedError):
            E.AutoEncoderFactory("timm", name)
        with pytest.raises(NotImplementedError):
            AutoClassifierFactory("timm", name, n_classes=3)
    with pytest.raises(NotImplementedError):
        E.AutoEncoderFactory("hf", "efficientnet_b0")


def test_no_gpu_is_a_loud_error():
    if torch.cuda.is_available():
        return                                              # (on a GPU box the GPU tests cover the engines)
    from effocr_amd.encoders import AutoEncoderFactory, make_encoder
    from effocr_amd.recognizer_engine import EffRecognizer
    sd = W.init_state_dict("efficientnet_b0", seed=0, img_size=32)
    with pytest.raises(_lib.EffOCRHipError):
        make_encoder("efficientnet_b0", sd, img_size=32)
    with pytest.raises(_lib.EffOCRHipError):
        AutoEncoderFactory("timm", "tf_efficientnet_b0", img_size=32)()(torch.zeros(1, 3, 32, 32))
    with pytest.raises(_lib.EffOCRHipError):
        EffRecognizer(sd, arch="tf_efficientnet_b0", img_size=32)


# ---------------------------------------------------------------------------------------------------- libeffocr_effnet.so without a GPU
def _create(arch, img=224, prec=1):
    L = _lib.effnet_lib()
    h = ctypes.c_void_p()
    rc = L.effocr_effnet_create(arch.encode(), img, prec, ctypes.byref(h))
    return L, rc, h


def test_every_symbol_resolves():
    L = _lib.effnet_lib()
    assert len(_lib.EFFNET_EXPORTS) == 19 and all(n.startswith("effocr_effnet_") for n in _lib.EFFNET_EXPORTS)
    for name in _lib.EFFNET_EXPORTS:
        assert getattr(L, name) is not None
    assert L.effocr_effnet_abi_version() == _lib.EFFNET_ABI_VERSION == 1


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_c_handle_tables_without_gpu(arch, prec):
    """The C side derives its block list from the name alone: its parameter names, order and sizes must be weights.param_shapes'."""
    L, rc, h = _create(arch, 224, _lib.PREC[prec])
    assert rc == 0, L.effocr_effnet_last_error()
    try:
        assert L.effocr_effnet_embed_dim(h) == 1280
        shapes = W.param_shapes(arch)
        n = L.effocr_effnet_num_params(h)
        names = [L.effocr_effnet_param_name(h, i).decode() for i in range(n)]
        assert names == list(shapes)
        for i, k in enumerate(names):
            assert L.effocr_effnet_param_numel(h, i) == math.prod(shapes[k])
        assert L.effocr_effnet_param_name(h, n) is None and L.effocr_effnet_param_numel(h, -1) == -1
        es = 4 if prec == "fp32" else 2
        assert L.effocr_effnet_weights_bytes(h) >= es * COUNT * 0.99
        assert L.effocr_effnet_workspace_bytes(h, 0) == 0
        ws1, ws16, ws4096 = (L.effocr_effnet_workspace_bytes(h, b) for b in (1, 16, 4096))
        assert 112 * 112 * 96 * 4 < ws1 < ws16 <= ws4096 <= 512 << 20            # the default sub-batch keeps the workspace within 512 MiB
        assert L.effocr_effnet_set_chunk(h, 8) == 0
        assert L.effocr_effnet_workspace_bytes(h, 4096) == L.effocr_effnet_workspace_bytes(h, 8) < ws16
        assert L.effocr_effnet_set_chunk(h, -1) == -1
        assert L.effocr_effnet_set_chunk(h, 65536) == -1 and b"65535" in L.effocr_effnet_last_error()       # (crops are a grid dimension)
        assert L.effocr_effnet_workspace_bytes(h, 4096) == L.effocr_effnet_workspace_bytes(h, 8)             # a refused setting changes nothing
        assert L.effocr_effnet_set_chunk(h, 65535) == 0 and L.effocr_effnet_set_chunk(h, 8) == 0
        t = torch.zeros(5)
        assert L.effocr_effnet_set_param(h, b"bn1.weight", _lib.ptr(t), 5) == -1
        assert L.effocr_effnet_set_param(h, b"classifier.weight", _lib.ptr(t), 5) == -1
        assert L.effocr_effnet_set_param(h, b"conv_head.bias", _lib.ptr(t), 5) == -1
        p = ctypes.c_void_p(256)
        assert L.effocr_effnet_forward(h, p, 2, 1, p, 0, p, 1 << 40, None) == -5     # forward before upload: refused on the host
        assert L.effocr_effnet_forward(h, p, 1, 1, p, 0, p, 1 << 40, None) == -2     # 16-bit crops: unsupported
        assert b"16-bit" in L.effocr_effnet_last_error()
        assert L.effocr_effnet_upload(h, p, 1 << 40) == -5                           # a parameter was never set
    finally:
        L.effocr_effnet_destroy(h)


@pytest.mark.parametrize("img", [0, 16, 48, 100, -32, 256])
def test_c_create_rejects_bad_img_size(img):
    L, rc, h = _create("efficientnet_b0", img)
    assert rc == -1 and b"img_size" in L.effocr_effnet_last_error()


@pytest.mark.parametrize("img", [32, 64, 96, 160, 224])
def test_c_create_accepts_multiples_of_32(img):
    L, rc, h = _create("tf_efficientnet_b0", img)
    assert rc == 0
    L.effocr_effnet_destroy(h)


@pytest.mark.parametrize("prec", [-1, 3, 7])
def test_c_create_rejects_bad_precision(prec):
    L, rc, h = _create("efficientnet_b0", 224, prec)
    assert rc == -1 and b"precision" in L.effocr_effnet_last_error()


def test_c_create_rejects_other_archs_and_other_libraries_unchanged():
    for a in ("efficientnet_b1", "efficientnet_lite0", "tf_efficientnet_b0_ns", "mobilenetv3_large_100", ""):
        L, rc, h = _create(a)
        assert rc == -2, a
    h = ctypes.c_void_p()
    for a in ARCHS:
        assert _lib.lib().effocr_encoder_create(a.encode(), 224, 1, ctypes.byref(h)) == -2       # the product library ...
        assert _lib.mnv3_lib().effocr_mnv3_create(a.encode(), 224, 1, ctypes.byref(h)) == -2     # ... and the MobileNetV3 one refuse them
    assert _lib.lib().effocr_abi_version() == 9 and _lib.mnv3_lib().effocr_mnv3_abi_version() == 1
    assert len(_lib.MNV3_EXPORTS) == 21                       # 15 + the six test entry points (effocr_mnv3_op_*)


def test_op_tiles():
    L = _lib.effnet_lib()
    assert [L.effocr_effnet_op_tiles(n) for n in (0, 1, 16, 17, 28, 56, 112)] == [0, 1, 1, 4, 4, 16, 49]
