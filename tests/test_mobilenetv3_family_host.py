"""MobileNetV3 family host side (-m "not gpu"): mobilenetv3_small_075 / mobilenetv3_small_100 / mobilenetv3_large_100 — the builder
against timm's published parameter counts, the hand-written float64 restatement (tests/mobilenetv3_family_ref.py) against an nn.Module
tree built from the builder, architecture inference, checkpoint I/O, the factory, and the C ABI of libeffocr_mnv3.so up to the device —
none of it needs a GPU."""
import ctypes
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from effocr_amd import _lib
from effocr_amd import weights as W
from tests import mobilenetv3_family_ref as MR
from tests.mobilenetv3_family_ref import mobilenetv3_family_forward
from tests.mobilenetv3_ref import mobilenetv3_forward

ARCHS = ["mobilenetv3_small_075", "mobilenetv3_small_100", "mobilenetv3_large_100"]
LARGE = "mobilenetv3_large_100"
# learnable parameters without / with a 1000-class classifier (timm's published 2.04 M, 2.54 M, 5.48 M with it)
COUNTS = {"mobilenetv3_small_050": (568_224, 1_593_224), "mobilenetv3_small_075": (1_016_872, 2_041_872),
          "mobilenetv3_small_100": (1_517_856, 2_542_856), LARGE: (4_202_032, 5_483_032)}


# ---------------------------------------------------------------------------------------------------- the builder
@pytest.mark.parametrize("arch", sorted(COUNTS))
def test_builder_counts(arch):
    assert W.mobilenetv3_num_learnable(arch) == COUNTS[arch][0]
    assert W.mobilenetv3_num_learnable(arch, num_classes=1000) == COUNTS[arch][1]


def test_large_table():
    stem, blocks, nf = W.mobilenetv3_blocks(LARGE)
    assert stem == 16 and nf == 1280 and W.embed_dim(LARGE) == 1280
    assert W.MOBILENETV3_FEATURES == 1024 and all(W.embed_dim(a) == 1024 for a in ARCHS[:2])
    assert [b["key"] for b in blocks] == ["blocks.0.0", "blocks.1.0", "blocks.1.1", "blocks.2.0", "blocks.2.1", "blocks.2.2", "blocks.3.0",
                                          "blocks.3.1", "blocks.3.2", "blocks.3.3", "blocks.4.0", "blocks.4.1", "blocks.5.0", "blocks.5.1",
                                          "blocks.5.2", "blocks.6.0"]
    assert [b["mid"] for b in blocks if b["type"] == "ir"] == [64, 72, 72, 120, 120, 240, 200, 184, 184, 480, 672, 672, 960, 960]
    assert [b["se"] for b in blocks if b["se"]] == [24, 32, 32, 120, 168, 168, 240, 240]
    shapes = W.param_shapes(LARGE)
    assert shapes["blocks.0.0.conv_pw.weight"] == (16, 16, 1, 1) and "blocks.0.0.se.conv_reduce.weight" not in shapes
    assert shapes["blocks.2.0.conv_dw.weight"] == (72, 1, 5, 5)
    assert shapes["blocks.6.0.conv.weight"] == (960, 160, 1, 1)
    assert shapes["conv_head.weight"] == (1280, 960, 1, 1) and shapes["conv_head.bias"] == (1280,)
    assert W.head_shapes(LARGE, 7) == {"classifier.weight": (7, 1280), "classifier.bias": (7,)}
    macs, H = 112 * 112 * 27 * 16, 112
    for b in blocks:
        Ho = (H - 1) // b["stride"] + 1
        if b["type"] == "ir":
            macs += H * H * b["cin"] * b["mid"]
        if b["type"] != "cn":
            macs += Ho * Ho * b["mid"] * b["k"] ** 2 + 2 * b["mid"] * b["se"]
        macs += Ho * Ho * (b["cin"] if b["type"] == "cn" else b["mid"]) * b["cout"]
        H = Ho
    macs += 960 * 1280
    assert 210e6 < macs < 220e6, macs                      # "about 215 M" multiply-accumulates per 224^2 crop


# ---------------------------------------------------------------------------------------------------- the nn.Module restatement
def _bn(c):
    return nn.BatchNorm2d(c, eps=1e-5)


class _SE(nn.Module):
    def __init__(self, c, r):
        super().__init__()
        self.conv_reduce = nn.Conv2d(c, r, 1, bias=True)
        self.conv_expand = nn.Conv2d(r, c, 1, bias=True)

    def forward(self, x):
        s = x.mean((2, 3), keepdim=True)
        return x * F.hardsigmoid(self.conv_expand(F.relu(self.conv_reduce(s))))


class _Block(nn.Module):
    """One entry of weights.mobilenetv3_blocks as timm's DepthwiseSeparableConv / InvertedResidual / ConvBnAct."""

    def __init__(self, b):
        super().__init__()
        self.t, self.res = b["type"], b["res"]
        self.act = nn.Hardswish() if b["hs"] else nn.ReLU()
        k, s = b["k"], b["stride"]
        if self.t == "ds":
            self.conv_dw = nn.Conv2d(b["cin"], b["cin"], k, s, k // 2, groups=b["cin"], bias=False)
            self.bn1 = _bn(b["cin"])
            self.se = _SE(b["cin"], b["se"]) if b["se"] else nn.Identity()
            self.conv_pw = nn.Conv2d(b["cin"], b["cout"], 1, bias=False)
            self.bn2 = _bn(b["cout"])
        elif self.t == "ir":
            self.conv_pw = nn.Conv2d(b["cin"], b["mid"], 1, bias=False)
            self.bn1 = _bn(b["mid"])
            self.conv_dw = nn.Conv2d(b["mid"], b["mid"], k, s, k // 2, groups=b["mid"], bias=False)
            self.bn2 = _bn(b["mid"])
            self.se = _SE(b["mid"], b["se"]) if b["se"] else nn.Identity()
            self.conv_pwl = nn.Conv2d(b["mid"], b["cout"], 1, bias=False)
            self.bn3 = _bn(b["cout"])
        else:
            self.conv = nn.Conv2d(b["cin"], b["cout"], 1, bias=False)
            self.bn1 = _bn(b["cout"])

    def forward(self, x):
        if self.t == "ds":
            y = self.bn2(self.conv_pw(self.se(self.act(self.bn1(self.conv_dw(x))))))
        elif self.t == "ir":
            y = self.act(self.bn1(self.conv_pw(x)))
            y = self.bn3(self.conv_pwl(self.se(self.act(self.bn2(self.conv_dw(y))))))
        else:
            return self.act(self.bn1(self.conv(x)))
        return y + x if self.res else y


class _MobileNetV3(nn.Module):
    def __init__(self, arch):
        super().__init__()
        stem, blocks, nf = W.mobilenetv3_blocks(arch)
        self.conv_stem = nn.Conv2d(3, stem, 3, 2, 1, bias=False)
        self.bn1 = _bn(stem)
        stages = {}
        for b in blocks:
            stages.setdefault(int(b["key"].split(".")[1]), []).append(_Block(b))
        self.blocks = nn.Sequential(*[nn.Sequential(*stages[i]) for i in sorted(stages)])
        self.conv_head = nn.Conv2d(blocks[-1]["cout"], nf, 1, bias=True)

    def forward(self, x):
        x = self.blocks(F.hardswish(self.bn1(self.conv_stem(x))))
        x = F.hardswish(self.conv_head(x.mean((2, 3), keepdim=True)))
        return x.flatten(1)


def _module(arch, sd):
    m = _MobileNetV3(arch).double().eval()
    full = dict(sd)
    for k in list(sd):
        if k.endswith(".running_var"):                  # a real checkpoint carries these; loading ignores their values
            full[k[: -len("running_var")] + "num_batches_tracked"] = torch.tensor(0)
    m.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in full.items()}, strict=True)
    return m


@pytest.mark.parametrize("arch", ARCHS)
def test_module_parameter_count(arch):
    assert sum(p.numel() for p in _MobileNetV3(arch).parameters()) == COUNTS[arch][0]


@pytest.mark.parametrize("img,B", [(224, 2), (64, 3)])
@pytest.mark.parametrize("arch", ARCHS)
def test_restatements_agree(arch, img, B):
    sd = W.init_state_dict(arch, seed=5, img_size=img)
    x = torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(img), dtype=torch.float64)
    ref = mobilenetv3_family_forward(arch, sd, x)
    with torch.no_grad():
        mod = _module(arch, sd)(x)
    assert ref.shape == (B, W.embed_dim(arch)) and ref.dtype == torch.float64
    rel = ((ref - mod).abs().max() / ref.abs().max()).item()
    print(f"{arch}: functional vs nn.Module restatement at {img}^2: {rel:.2e}")
    assert rel <= 1e-12
    assert ref.abs().max() > 1e-3


def test_family_restatement_equals_the_050_restatement():
    from tests.mobilenetv3_ref import mobilenetv3_forward
    arch = "mobilenetv3_small_050"
    sd = W.init_state_dict(arch, seed=6, img_size=64)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    assert torch.equal(mobilenetv3_family_forward(arch, sd, x), mobilenetv3_forward(arch, sd, x))


# ---------------------------------------------------------------------------------------------------- tables, I/O, init
@pytest.mark.parametrize("arch", ARCHS)
def test_check_state_dict_and_infer_arch(arch):
    sd = W.init_state_dict(arch, seed=0)
    W.check_state_dict(arch, sd)
    assert W.infer_arch(sd) == arch
    assert W.infer_arch({"net." + k: v for k, v in sd.items()}) == arch
    with_head = W.init_state_dict(arch, seed=0, num_classes=11)
    assert W.infer_arch(with_head) == arch and W.infer_num_classes(with_head) == 11
    W.check_state_dict(arch, with_head, num_classes=11)
    assert tuple(with_head["classifier.weight"].shape) == (11, W.embed_dim(arch))
    for scale in ("unit", "timm"):
        W.check_state_dict(arch, W.init_state_dict(arch, seed=3, scale=scale))
    bad = dict(sd)
    bad["blocks.2.1.conv_pw.weight"] = torch.zeros(144, 23, 1, 1)
    with pytest.raises(ValueError, match="blocks.2.1.conv_pw.weight"):
        W.check_state_dict(arch, bad)
    last = "blocks.5.2." if arch == LARGE else "blocks.4.2."
    with pytest.raises(ValueError):
        W.infer_arch({k: v for k, v in sd.items() if not k.startswith(last)})


@pytest.mark.parametrize("arch", ARCHS)
def test_checkpoint_round_trip_and_factory(arch, tmp_path):
    from effocr_amd.encoders import AutoEncoderFactory
    sd = W.init_state_dict(arch, seed=2)
    path = tmp_path / "enc_best.pth"
    W.save_checkpoint(sd, path)
    back = W.load_checkpoint(path)
    assert sorted(back) == sorted(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    assert W.infer_arch(back) == arch
    cls = AutoEncoderFactory("timm", arch)
    params = list(cls().named_parameters())
    assert all(k.startswith("net.") for k, _ in params)
    assert sum(p.numel() for _, p in params) == COUNTS[arch][0]
    got = cls.load(str(path)).state_dict()                 # CPU only: the engine is built on first forward
    assert all(torch.equal(got["net." + k], v) for k, v in sd.items())
    wrong = dict(sd)
    wrong["conv_head.weight"] = torch.zeros(1024 if arch == LARGE else 1280, sd["conv_head.weight"].shape[1], 1, 1)
    with pytest.raises(ValueError, match="conv_head.weight"):
        cls().load_state_dict(wrong)


def test_dispatch():
    from effocr_amd import encoders as E
    assert all(W.is_mnv3_lib(a) for a in ARCHS) and not W.is_mnv3_lib("mobilenetv3_small_050") and not W.is_mnv3_lib("resnet50")
    assert issubclass(E.MobileNetV3Encoder, E.HipEncoder)
    with pytest.raises(NotImplementedError):
        W.embed_dim("mobilenetv3_large_075")
    with pytest.raises(NotImplementedError):
        E.AutoEncoderFactory("timm", "tf_mobilenetv3_large_100")


# ---------------------------------------------------------------------------------------------------- libeffocr_mnv3.so without a GPU
def _create(arch, img=224, prec=1):
    L = _lib.mnv3_lib()
    h = ctypes.c_void_p()
    rc = L.effocr_mnv3_create(arch.encode(), img, prec, ctypes.byref(h))
    return L, rc, h


def test_every_symbol_resolves():
    L = _lib.mnv3_lib()
    assert len(_lib.MNV3_EXPORTS) == 21 and all(n.startswith("effocr_mnv3_") for n in _lib.MNV3_EXPORTS)
    for name in _lib.MNV3_EXPORTS:
        assert getattr(L, name) is not None
    assert L.effocr_mnv3_abi_version() == _lib.MNV3_ABI_VERSION


@pytest.mark.parametrize("arch", ARCHS + ["mobilenetv3_small_050"])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_c_handle_tables_without_gpu(arch, prec):
    """The C side derives its block list from the name alone: its parameter names, order and sizes must be weights.param_shapes'."""
    L, rc, h = _create(arch, 224, _lib.PREC[prec])
    assert rc == 0, L.effocr_mnv3_last_error()
    try:
        assert L.effocr_mnv3_embed_dim(h) == W.embed_dim(arch)
        shapes = W.param_shapes(arch)
        n = L.effocr_mnv3_num_params(h)
        names = [L.effocr_mnv3_param_name(h, i).decode() for i in range(n)]
        assert names == list(shapes)
        for i, k in enumerate(names):
            assert L.effocr_mnv3_param_numel(h, i) == math.prod(shapes[k])
        assert L.effocr_mnv3_param_name(h, n) is None and L.effocr_mnv3_param_numel(h, -1) == -1
        es = 4 if prec == "fp32" else 2
        assert L.effocr_mnv3_weights_bytes(h) >= es * COUNTS[arch][0] * 0.99
        assert L.effocr_mnv3_workspace_bytes(h, 0) == 0
        ws1, ws16, ws4096 = (L.effocr_mnv3_workspace_bytes(h, b) for b in (1, 16, 4096))
        assert 0 < ws1 < ws16 <= ws4096 <= 512 << 20               # sub-batches keep the workspace under 512 MiB
        assert L.effocr_mnv3_set_chunk(h, 8) == 0
        assert L.effocr_mnv3_workspace_bytes(h, 4096) == L.effocr_mnv3_workspace_bytes(h, 8) < ws16
        t = torch.zeros(5)
        assert L.effocr_mnv3_set_param(h, b"bn1.weight", _lib.ptr(t), 5) == -1
        assert L.effocr_mnv3_set_param(h, b"classifier.weight", _lib.ptr(t), 5) == -1
        ws = ctypes.c_void_p(256)
        assert L.effocr_mnv3_forward(h, ws, 1, ws, 0, ws, 1 << 40, None) == -5     # forward before upload: refused on the host
    finally:
        L.effocr_mnv3_destroy(h)


@pytest.mark.parametrize("img", [0, 16, 48, 100, -32, 256])
def test_c_create_rejects_bad_img_size(img):
    L, rc, h = _create(LARGE, img)
    assert rc == -1 and b"img_size" in L.effocr_mnv3_last_error()


@pytest.mark.parametrize("img", [32, 64, 160, 224])
def test_c_create_accepts_multiples_of_32(img):
    L, rc, h = _create("mobilenetv3_small_100", img)
    assert rc == 0
    L.effocr_mnv3_destroy(h)


@pytest.mark.parametrize("prec", [-1, 3, 7])
def test_c_create_rejects_bad_precision(prec):
    L, rc, h = _create(LARGE, 224, prec)
    assert rc == -1 and b"precision" in L.effocr_mnv3_last_error()


def test_c_create_rejects_other_archs_and_product_library_unchanged():
    for a in ("mobilenetv3_large_075", "tf_mobilenetv3_large_100", "mobilenetv3_rw", "resnet50", ""):
        L, rc, h = _create(a)
        assert rc == -2, a
    lib = _lib.lib()
    h = ctypes.c_void_p()
    for a in ARCHS:
        assert lib.effocr_encoder_create(a.encode(), 224, 1, ctypes.byref(h)) == -2      # the product library goes on refusing them


# ---------------------------------------------------------------------------------------------------- the restatement's round_pw path, the signal checkpoint
@pytest.mark.parametrize("arch", ARCHS + ["mobilenetv3_small_050"])
def test_round_pw_path_against_plain(arch):
    """The restatement's round_pw path (the GPU tests' e_w) folds BN into the weights: with no rounding to speak of it gives the plain
    path's result, with bf16 it does not.  The plain path itself is untouched: mobilenetv3_small_050 through it is bit-identical to
    tests/mobilenetv3_ref.py, the same sequence of operations written out a second time."""
    sd = W.init_state_dict(arch, seed=11, img_size=64, scale="timm")
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)).double()
    a = mobilenetv3_family_forward(arch, sd, x)
    assert torch.equal(a, mobilenetv3_family_forward(arch, sd, x, round_pw=None))
    if arch == "mobilenetv3_small_050":
        assert torch.equal(a, mobilenetv3_forward(arch, sd, x))
    b = mobilenetv3_family_forward(arch, sd, x, round_pw=torch.float32)
    c = mobilenetv3_family_forward(arch, sd, x, round_pw=torch.bfloat16)
    rel = lambda u, v: ((u - v).abs().max() / v.abs().max()).item()
    assert rel(b, a) < 2e-6 and 1e-4 < rel(c, a) < 5e-2


@pytest.mark.parametrize("img", MR.SIGNAL_IMGS + (224,))
@pytest.mark.parametrize("arch", ARCHS + ["mobilenetv3_small_050"])
def test_signal_checkpoint_depends_on_the_crop(arch, img):
    """The premise of the GPU tests' crop-dependent parity, from the reference alone: all-zero crops and transposed crops each move the
    float64 embedding of the signal checkpoint by more than 0.1 of its norm, and a float32 run of the restatement stays within 3e-6 of
    float64 (the checkpoint does not amplify rounding, so the fp32 mode's 1e-5 stands).  224^2: the batch-invariance cases that use it."""
    if img == 224 and arch not in ("mobilenetv3_small_050", "mobilenetv3_small_100"):
        return
    B = 2 if img == 224 else MR.SIGNAL_B
    ref, d_zero, d_transposed = MR.signal_reference(arch, img, None, B)
    f32 = mobilenetv3_family_forward(arch, MR.signal_sd(arch, img), MR.signal_crops(img, B))
    e32 = ((f32 - ref).abs().max() / ref.abs().max()).item()
    print(f"{arch} {img}^2 gain {MR.SIGNAL_GAIN[arch]}: zero crops {d_zero:.2f}, transposed {d_transposed:.2f}, float32 vs float64 {e32:.1e}")
    assert d_zero > 0.1 and d_transposed > 0.1 and e32 < 3e-6
    unit = W.init_state_dict(arch, seed=7, img_size=img)
    assert all(torch.equal(v, unit[k]) for k, v in MR.signal_sd(arch, img).items() if v.dim() != 4 or ".se." in k)
