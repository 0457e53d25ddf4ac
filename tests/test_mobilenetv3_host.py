"""mobilenetv3_small_050 host side (-m "not gpu"): the parameter-table builder against timm's published counts, two independently
written restatements against each other in float64, the activations against their formulas, checkpoint I/O, key inference, seeded
init, and the C ABI's handle (creation, parameter table, workspace size) — none of it needs a GPU."""
import ctypes
import hashlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from effocr_amd import weights as W
from tests.mobilenetv3_ref import mobilenetv3_forward

ARCH = "mobilenetv3_small_050"


# ---------------------------------------------------------------------------------------------------- the builder
@pytest.mark.parametrize("arch,count", [("mobilenetv3_small_050", 1_593_224), ("mobilenetv3_small_075", 2_041_872),
                                        ("mobilenetv3_small_100", 2_542_856)])
def test_builder_counts_with_classifier(arch, count):
    # timm's published counts: 1.59 M, 2.04 M, 2.54 M (1000-class classifier on the 1024-d head)
    assert W.mobilenetv3_num_learnable(arch, num_classes=1000) == count


def test_param_table_050():
    shapes = W.param_shapes(ARCH)
    assert len(shapes) == 208
    assert W.embed_dim(ARCH) == 1024
    assert W.mobilenetv3_num_learnable(ARCH) == 568_224
    assert shapes["conv_stem.weight"] == (16, 3, 3, 3)
    assert shapes["blocks.0.0.se.conv_reduce.weight"] == (8, 16, 1, 1)
    assert shapes["blocks.0.0.conv_pw.weight"] == (8, 16, 1, 1)
    assert shapes["blocks.1.0.conv_pw.weight"] == (40, 8, 1, 1)
    assert shapes["blocks.1.1.conv_dw.weight"] == (56, 1, 3, 3)
    assert "blocks.1.1.se.conv_reduce.weight" not in shapes
    assert shapes["blocks.2.0.conv_dw.weight"] == (64, 1, 5, 5)
    assert shapes["blocks.2.0.se.conv_reduce.weight"] == (16, 64, 1, 1)
    assert shapes["blocks.2.2.se.conv_expand.weight"] == (144, 40, 1, 1)
    assert shapes["blocks.3.1.se.conv_reduce.weight"] == (24, 72, 1, 1)
    assert shapes["blocks.4.2.conv_pwl.weight"] == (48, 288, 1, 1)
    assert shapes["blocks.5.0.conv.weight"] == (288, 48, 1, 1)
    assert shapes["conv_head.weight"] == (1024, 288, 1, 1) and shapes["conv_head.bias"] == (1024,)
    assert "blocks.4.3.conv_pw.weight" not in shapes and "classifier.weight" not in shapes


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


def _module(sd):
    m = _MobileNetV3(ARCH).double().eval()
    full = dict(sd)
    for k in list(sd):
        if k.endswith(".running_var"):                  # a real checkpoint carries these; loading ignores their values
            full[k[: -len("running_var")] + "num_batches_tracked"] = torch.tensor(0)
    m.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in full.items()}, strict=True)
    return m


def test_module_parameter_count():
    assert sum(p.numel() for p in _MobileNetV3(ARCH).parameters()) == 568_224


@pytest.mark.parametrize("img,B", [(224, 2), (64, 3)])
@pytest.mark.parametrize("scale", ["unit", "timm"])
def test_restatements_agree(img, B, scale):
    sd = W.init_state_dict(ARCH, seed=5, img_size=img, scale=scale)
    x = torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(img), dtype=torch.float64)
    ref = mobilenetv3_forward(ARCH, sd, x)
    with torch.no_grad():
        mod = _module(sd)(x)
    assert ref.shape == (B, 1024) and ref.dtype == torch.float64
    rel = ((ref - mod).abs().max() / ref.abs().max()).item()
    print(f"functional vs nn.Module restatement at {img}^2 ({scale}): {rel:.2e}")
    assert rel <= 1e-12
    assert ref.abs().max() > 1e-3


def test_se_and_residuals_are_live():
    """Dropping blocks.0.0's SE or any residual changes the functional restatement's output: both restatements exercise them."""
    sd = W.init_state_dict(ARCH, seed=6, img_size=64)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    base = mobilenetv3_forward(ARCH, sd, x)
    sd2 = dict(sd)
    sd2["blocks.0.0.se.conv_expand.bias"] = sd["blocks.0.0.se.conv_expand.bias"] + 10.0   # gate saturates at 1
    assert not torch.allclose(mobilenetv3_forward(ARCH, sd2, x), base)
    m = _module(sd)
    with torch.no_grad():
        assert torch.allclose(m(x), base, rtol=1e-12, atol=0)
        for blk in m.blocks.modules():
            if isinstance(blk, _Block) and blk.res:
                blk.res = False
                assert not torch.allclose(m(x), base)
                blk.res = True


def test_activation_identities():
    x = torch.linspace(-8, 8, 4001, dtype=torch.float64)
    relu6 = lambda t: t.clamp(0, 6)                     # noqa: E731
    assert torch.allclose(F.hardswish(x), x * relu6(x + 3) / 6, rtol=0, atol=1e-15)
    assert torch.allclose(F.hardsigmoid(x), relu6(x + 3) / 6, rtol=0, atol=1e-15)


# ---------------------------------------------------------------------------------------------------- tables, I/O, init
def test_check_state_dict_and_infer_arch():
    sd = W.init_state_dict(ARCH, seed=0)
    W.check_state_dict(ARCH, sd)
    assert W.infer_arch(sd) == ARCH
    assert W.infer_arch({"net." + k: v for k, v in sd.items()}) == ARCH
    bad = dict(sd)
    bad["blocks.2.1.conv_pw.weight"] = torch.zeros(144, 23, 1, 1)
    with pytest.raises(ValueError, match="blocks.2.1.conv_pw.weight"):
        W.check_state_dict(ARCH, bad)
    missing = dict(sd)
    del missing["blocks.3.0.se.conv_reduce.bias"]
    with pytest.raises(ValueError, match="missing blocks.3.0.se.conv_reduce.bias"):
        W.check_state_dict(ARCH, missing)
    # a truncated checkpoint, and a different width, are not mobilenetv3_small_050
    with pytest.raises(ValueError):
        W.infer_arch({k: v for k, v in sd.items() if not k.startswith("blocks.4.2.")})
    assert W.infer_arch(W.init_state_dict("mobilenetv3_small_100", seed=0)) == "mobilenetv3_small_100"
    assert W.infer_arch(W.init_state_dict("mobilenetv3_small_075", seed=0)) == "mobilenetv3_small_075"


@pytest.mark.parametrize("suffix", [".pth", ".safetensors"])
def test_checkpoint_round_trip(tmp_path, suffix):
    sd = W.init_state_dict(ARCH, seed=2)
    path = tmp_path / ("enc_best" + suffix)
    W.save_checkpoint(sd, path)
    if suffix == ".pth":
        assert all(k.startswith("net.") for k in torch.load(path, weights_only=True))
    back = W.load_checkpoint(path)
    assert sorted(back) == sorted(sd)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    assert W.infer_arch(back) == ARCH


def test_factory_named_parameters(tmp_path):
    from effocr_amd.encoders import AutoEncoderFactory
    cls = AutoEncoderFactory("timm", ARCH)
    enc = cls()
    params = list(enc.named_parameters())
    assert all(k.startswith("net.") for k, _ in params)
    assert sum(p.numel() for _, p in params) == 568_224
    sd = W.init_state_dict(ARCH, seed=4)
    W.save_checkpoint(sd, tmp_path / "enc.pth")
    got = cls.load(str(tmp_path / "enc.pth")).state_dict()
    assert all(torch.equal(got["net." + k], v) for k, v in sd.items())


def test_seeded_init_is_deterministic_and_nontrivial():
    a = W.init_state_dict(ARCH, seed=9)
    b = W.init_state_dict(ARCH, seed=9)
    c = W.init_state_dict(ARCH, seed=10)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["conv_stem.weight"], c["conv_stem.weight"])
    for k in ("bn1.weight", "blocks.2.1.bn2.weight", "blocks.5.0.bn1.weight"):
        assert 0.5 <= a[k].min() and a[k].max() <= 1.5 and a[k].std() > 0.1, k
    assert a["blocks.1.0.bn1.running_var"].min() >= 0.5 and a["blocks.1.0.bn1.running_var"].std() > 0.1
    assert a["blocks.4.0.bn3.running_mean"].abs().max() > 0.05
    assert a["conv_head.bias"].abs().max() > 0.05
    assert abs(a["blocks.2.1.conv_dw.weight"].std().item() - 1 / 5) < 0.02          # fan-in 25
    t = W.init_state_dict(ARCH, seed=9, scale="timm")
    assert torch.all(t["bn1.weight"] == 1) and torch.all(t["blocks.2.0.bn3.running_var"] == 1)
    assert torch.all(t["blocks.2.0.se.conv_reduce.bias"] == 0) and torch.all(t["conv_head.bias"] == 0)
    assert abs(t["conv_head.weight"].std().item() - (2 / 1024) ** 0.5) < 0.003          # fan_out = 1024
    assert abs(t["blocks.4.1.conv_dw.weight"].std().item() - (2 / 25) ** 0.5) < 0.02     # depthwise: fan_out = k * k


# sha256 (first 32 hex digits) over (key, fp32 bytes) of init_state_dict(arch, seed=1, 224, scale), taken on the tree before
# MobileNetV3 was added (the hashes of the other architectures are pinned in test_convnext_host.py)
_FROZEN_CNX = {"unit": "145739ab4c744687a0fa7b55ea5cbb75", "timm": "40bc3448f2f1491649ece4271ea27ee4"}


@pytest.mark.parametrize("scale", sorted(_FROZEN_CNX))
def test_convnext_seeded_stream_unchanged(scale):
    h = hashlib.sha256()
    for k, v in W.init_state_dict("convnext_tiny", seed=1, img_size=224, scale=scale).items():
        h.update(k.encode())
        h.update(v.numpy().tobytes())
    assert h.hexdigest()[:32] == _FROZEN_CNX[scale]


# ---------------------------------------------------------------------------------------------------- the C ABI handle
def test_cabi_handle(hip_lib):
    h = ctypes.c_void_p()
    shapes = W.param_shapes(ARCH)
    for prec in (0, 1, 2):
        assert hip_lib.effocr_encoder_create(ARCH.encode(), 224, prec, ctypes.byref(h)) == 0
        try:
            assert hip_lib.effocr_encoder_embed_dim(h) == 1024
            n = hip_lib.effocr_encoder_num_params(h)
            names = [hip_lib.effocr_encoder_param_name(h, i).decode() for i in range(n)]
            assert names == list(shapes)
            for i, k in enumerate(names):
                numel = 1
                for d in shapes[k]:
                    numel *= d
                assert hip_lib.effocr_encoder_param_numel(h, i) == numel
            assert hip_lib.effocr_encoder_weights_bytes(h) > 0
            # default sub-batch: <= 512 crops, workspace <= 128 MiB; it grows with the chunk setting only
            ws1 = hip_lib.effocr_encoder_workspace_bytes(h, 1)
            ws = hip_lib.effocr_encoder_workspace_bytes(h, 1024)
            assert 0 < ws1 < ws <= (128 << 20)
            assert hip_lib.effocr_encoder_workspace_bytes(h, 512) == ws
            assert hip_lib.effocr_encoder_set_chunk(h, 5) == 0
            assert hip_lib.effocr_encoder_workspace_bytes(h, 1024) == hip_lib.effocr_encoder_workspace_bytes(h, 5) < ws
        finally:
            hip_lib.effocr_encoder_destroy(h)
    for bad in (0, 16, 48, 100, 256):
        assert hip_lib.effocr_encoder_create(ARCH.encode(), bad, 1, ctypes.byref(h)) == -1
    for ok in (32, 64, 160):
        assert hip_lib.effocr_encoder_create(ARCH.encode(), ok, 1, ctypes.byref(h)) == 0
        hip_lib.effocr_encoder_destroy(h)
