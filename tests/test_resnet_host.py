"""Host-side tests of the ResNet-34 / ResNet-50 encoders (no GPU): the parameter tables, the float64 restatement pinned to
transformers.ResNetModel, architecture inference and the C ABI of libeffocr_resnet.so up to the device."""
import ctypes
import math

import pytest
import torch

from effocr_amd import _lib
from effocr_amd import weights as W
from effocr_amd.encoders import AutoEncoderFactory
from tests.resnet_ref import hf_state_dict, resnet_forward

ARCHS = ["resnet34", "resnet50"]
COUNTS = {"resnet34": 21_284_672, "resnet50": 23_508_032}       # timm num_classes=0


def _learnable(arch):
    return sum(math.prod(s) for k, s in W.param_shapes(arch).items() if not k.endswith(("running_mean", "running_var")))


@pytest.mark.parametrize("arch", ARCHS)
def test_param_counts_and_embed_dim(arch):
    assert _learnable(arch) == COUNTS[arch]
    assert W.embed_dim(arch) == {"resnet34": 512, "resnet50": 2048}[arch]
    assert W.head_keys(arch) == ("fc.weight", "fc.bias")
    assert W.head_shapes(arch, 7)["fc.weight"] == (7, W.embed_dim(arch))


def _hf_model(arch):
    transformers = pytest.importorskip("transformers")
    bott = W.RESNET_CFG[arch][2] == "bottleneck"
    cfg = transformers.ResNetConfig(layer_type="bottleneck" if bott else "basic", depths=[3, 4, 6, 3],
                                    hidden_sizes=[256, 512, 1024, 2048] if bott else [64, 128, 256, 512], embedding_size=64,
                                    downsample_in_bottleneck=False)
    return transformers.ResNetModel(cfg).eval()


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("img", [224, 64])
def test_restatement_matches_transformers(arch, img):
    m = _hf_model(arch)
    assert sum(p.numel() for p in m.parameters()) == COUNTS[arch]
    sd = W.init_state_dict(arch, seed=5, img_size=img)
    hsd = hf_state_dict(sd)
    missing, unexpected = m.load_state_dict(hsd, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    x = torch.randn(2, 3, img, img, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = m(x).pooler_output.flatten(1)
        got = resnet_forward(arch, sd, x)
    rel = ((got - want).abs().max() / want.abs().max()).item()
    assert rel <= 1e-5, rel


@pytest.mark.parametrize("arch", ["resnet18"] + ARCHS)
def test_infer_arch(arch):
    sd = W.init_state_dict(arch, seed=0)
    sd["layer1.0.bn1.num_batches_tracked"] = torch.tensor(0)
    assert W.infer_arch(sd) == arch
    assert W.infer_arch({"net." + k: v for k, v in sd.items()}) == arch


def test_infer_arch_rejects_other_depths():
    sd = W.init_state_dict("resnet34", seed=0)
    sd = {k: v for k, v in sd.items() if not k.startswith("layer3.5.")}
    with pytest.raises(ValueError, match="unsupported ResNet"):
        W.infer_arch(sd)


@pytest.mark.parametrize("arch", ARCHS)
def test_check_state_dict(arch):
    sd = W.init_state_dict(arch, seed=0)
    W.check_state_dict(arch, sd)
    sd["layer2.0.conv2.weight"] = torch.zeros(1, 1, 3, 3)
    with pytest.raises(ValueError, match="layer2.0.conv2.weight"):
        W.check_state_dict(arch, sd)
    other = "resnet50" if arch == "resnet34" else "resnet34"
    with pytest.raises(ValueError):
        W.check_state_dict(other, W.init_state_dict(arch, seed=0))


@pytest.mark.parametrize("arch", ARCHS)
def test_init_is_seeded_and_resnet18_stream_unchanged(arch):
    a, b = W.init_state_dict(arch, seed=3), W.init_state_dict(arch, seed=3)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["conv1.weight"], W.init_state_dict(arch, seed=4)["conv1.weight"])
    t = W.init_state_dict(arch, seed=3, scale="timm")
    last = "bn3" if arch == "resnet50" else "bn2"
    assert torch.count_nonzero(t[f"layer1.0.{last}.weight"]) == 0           # timm's zero_init_last
    assert (a["bn1.running_var"] > 0).all()


@pytest.mark.parametrize("arch", ARCHS)
def test_factory_accepts_and_loads(arch, tmp_path):
    cls = AutoEncoderFactory("timm", arch)
    sd = W.init_state_dict(arch, seed=1)
    path = tmp_path / "enc_best.pth"
    W.save_checkpoint(sd, path)
    enc = cls.load(str(path))                                            # CPU only: the engine is built on first forward
    assert set(enc.state_dict()) == {"net." + k for k in sd}
    n = sum(p.numel() for _, p in enc.named_parameters())
    assert n == COUNTS[arch]


def _create(arch, img=224, prec=1):
    L = _lib.resnet_lib()
    h = ctypes.c_void_p()
    rc = L.effocr_resnet_create(arch.encode(), img, prec, ctypes.byref(h))
    return L, rc, h


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_c_handle_tables_without_gpu(arch, prec):
    L, rc, h = _create(arch, 224, _lib.PREC[prec])
    assert rc == 0, L.effocr_resnet_last_error()
    try:
        assert L.effocr_resnet_abi_version() == _lib.RESNET_ABI_VERSION
        assert L.effocr_resnet_embed_dim(h) == W.embed_dim(arch)
        shapes = W.param_shapes(arch)
        n = L.effocr_resnet_num_params(h)
        names = [L.effocr_resnet_param_name(h, i).decode() for i in range(n)]
        assert names == list(shapes)
        for i, k in enumerate(names):
            assert L.effocr_resnet_param_numel(h, i) == math.prod(shapes[k])
        assert L.effocr_resnet_param_name(h, n) is None and L.effocr_resnet_param_numel(h, -1) == -1
        es = 4 if prec == "fp32" else 2
        assert L.effocr_resnet_weights_bytes(h) >= es * COUNTS[arch] * 0.99
        assert L.effocr_resnet_workspace_bytes(h, 0) == 0
        ws1, ws64, ws4096 = (L.effocr_resnet_workspace_bytes(h, b) for b in (1, 64, 4096))
        assert 0 < ws1 < ws64 <= ws4096 < 1000 << 20                       # sub-batches keep the workspace under 1 GB
        assert L.effocr_resnet_set_chunk(h, 8) == 0
        assert L.effocr_resnet_workspace_bytes(h, 4096) == L.effocr_resnet_workspace_bytes(h, 8) < ws64
        t = torch.zeros(5)
        assert L.effocr_resnet_set_param(h, b"bn1.weight", _lib.ptr(t), 5) == -1
        assert L.effocr_resnet_set_param(h, b"fc.weight", _lib.ptr(t), 5) == -1
    finally:
        L.effocr_resnet_destroy(h)


@pytest.mark.parametrize("img", [0, 16, 48, 100, -32])
def test_c_create_rejects_bad_img_size(img):
    L, rc, h = _create("resnet50", img)
    assert rc == -1 and b"img_size" in L.effocr_resnet_last_error()


@pytest.mark.parametrize("prec", [-1, 3, 7])
def test_c_create_rejects_bad_precision(prec):
    L, rc, h = _create("resnet34", 224, prec)
    assert rc == -1 and b"precision" in L.effocr_resnet_last_error()


def test_c_create_rejects_other_archs():
    for a in ("resnet18", "resnet101", "resnet50d"):
        L, rc, h = _create(a)
        assert rc == -2, a
    lib = _lib.lib()
    h = ctypes.c_void_p()
    assert lib.effocr_encoder_create(b"resnet50", 224, 1, ctypes.byref(h)) == -2      # the product library is unchanged
