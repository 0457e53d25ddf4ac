"""convnext_tiny host side (-m "not gpu"): the CPU restatement against transformers' ConvNextModel, the parameter tables, checkpoint
I/O, seeded init, and the C ABI's handle (creation, parameter table, workspace size) — none of it needs a GPU."""
import ctypes
import hashlib

import pytest
import torch

from effocr_amd import weights as W
from tests.convnext_ref import convnext_forward, hf_state_dict

ARCH = "convnext_tiny"


def _hf_model():
    from transformers import ConvNextConfig, ConvNextModel
    # transformers' defaults ARE ConvNeXt-T (depths 3,3,9,3; widths 96..768; layer scale; erf GELU) except the final LayerNorm's
    # eps (1e-12); timm's head uses 1e-6
    return ConvNextModel(ConvNextConfig(layer_norm_eps=1e-6)).eval()


@pytest.mark.parametrize("img,B", [(224, 2), (64, 3)])
def test_restatement_matches_transformers(img, B):
    sd = W.init_state_dict(ARCH, seed=5, img_size=img)
    m = _hf_model()
    missing, unexpected = m.load_state_dict(hf_state_dict(sd), strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    x = torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(img))
    ref = convnext_forward(ARCH, sd, x)
    with torch.no_grad():
        hf = m(pixel_values=x).pooler_output
    assert ref.shape == (B, 768)
    rel = ((ref - hf).abs().max() / hf.abs().max()).item()
    print(f"restatement vs transformers at {img}^2: {rel:.2e}")
    assert rel <= 1e-5


def test_param_table_and_counts():
    shapes = W.param_shapes(ARCH)
    assert W.embed_dim(ARCH) == 768
    assert shapes["stem.0.weight"] == (96, 3, 4, 4)
    assert shapes["stages.1.downsample.0.weight"] == (96,)
    assert shapes["stages.3.downsample.1.weight"] == (768, 384, 2, 2)
    assert shapes["stages.2.blocks.8.conv_dw.weight"] == (384, 1, 7, 7)
    assert shapes["stages.3.blocks.2.mlp.fc1.weight"] == (3072, 768)
    assert shapes["head.norm.bias"] == (768,)
    assert "stages.0.downsample.0.weight" not in shapes and "stages.2.blocks.9.gamma" not in shapes
    n = 0
    for v in shapes.values():
        k = 1
        for d in v:
            k *= d
        n += k
    assert n == 27_820_128
    assert sum(p.numel() for p in _hf_model().parameters()) == 27_820_128


def test_check_state_dict_and_infer_arch():
    sd = W.init_state_dict(ARCH, seed=0)
    W.check_state_dict(ARCH, sd)
    pref = {"net." + k: v for k, v in sd.items()}
    assert W.infer_arch(pref) == ARCH
    assert W.infer_arch(sd) == ARCH
    bad = dict(sd)
    bad["stages.2.blocks.3.mlp.fc1.weight"] = torch.zeros(1536, 383)
    with pytest.raises(ValueError, match="stages.2.blocks.3.mlp.fc1.weight"):
        W.check_state_dict(ARCH, bad)
    missing = dict(sd)
    del missing["stages.1.blocks.0.gamma"]
    with pytest.raises(ValueError, match="missing stages.1.blocks.0.gamma"):
        W.check_state_dict(ARCH, missing)
    # a ConvNeXt with other depths is not convnext_tiny
    small = {k: v for k, v in sd.items() if not k.startswith("stages.2.blocks.8.")}
    with pytest.raises(ValueError):
        W.infer_arch(small)


@pytest.mark.parametrize("suffix", [".pth", ".safetensors"])
def test_checkpoint_round_trip(tmp_path, suffix):
    sd = W.init_state_dict(ARCH, seed=2)
    path = tmp_path / ("enc_best" + suffix)
    W.save_checkpoint(sd, path)
    raw = torch.load(path, weights_only=True) if suffix == ".pth" else None
    if raw is not None:
        assert all(k.startswith("net.") for k in raw)
    back = W.load_checkpoint(path)
    assert sorted(back) == sorted(sd)                # (safetensors stores its keys sorted)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    assert W.infer_arch(back) == ARCH


def test_factory_named_parameters(tmp_path):
    from effocr_amd.encoders import AutoEncoderFactory
    cls = AutoEncoderFactory("timm", ARCH)
    enc = cls()
    params = list(enc.named_parameters())
    assert all(k.startswith("net.") for k, _ in params)
    assert sum(p.numel() for _, p in params) == 27_820_128
    sd = W.init_state_dict(ARCH, seed=4)
    W.save_checkpoint(sd, tmp_path / "enc.pth")
    enc2 = cls.load(str(tmp_path / "enc.pth"))
    got = enc2.state_dict()
    assert all(torch.equal(got["net." + k], v) for k, v in sd.items())


def test_seeded_init_is_deterministic_and_nontrivial():
    a = W.init_state_dict(ARCH, seed=9)
    b = W.init_state_dict(ARCH, seed=9)
    c = W.init_state_dict(ARCH, seed=10)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["stem.0.weight"], c["stem.0.weight"])
    # every term non-trivial under scale="unit": LayerNorm gains that lack "norm" in their names, layer scale well away from 0
    for k in ("stem.1.weight", "stages.2.downsample.0.weight", "stages.0.blocks.0.norm.weight", "head.norm.weight"):
        assert 0.5 <= a[k].min() and a[k].max() <= 1.5 and a[k].std() > 0.1, k
    assert a["stages.1.blocks.2.gamma"].min() >= 0.2 and a["stages.1.blocks.2.gamma"].max() <= 1.0
    assert abs(a["stages.0.blocks.0.conv_dw.weight"].std().item() - 1 / 7) < 0.02     # fan-in 49
    t = W.init_state_dict(ARCH, seed=9, scale="timm")
    assert torch.all(t["stages.3.blocks.1.gamma"] == 1e-6)
    assert torch.all(t["stem.1.weight"] == 1) and torch.all(t["stages.1.downsample.0.bias"] == 0)
    assert abs(t["stages.2.blocks.0.mlp.fc1.weight"].std().item() - 0.02) < 0.003


# sha256 (first 32 hex digits) over (key, fp32 bytes) of init_state_dict(arch, seed=1, img_size, scale), taken on the tree BEFORE
# ConvNeXt was added: the existing architectures' seeded streams must not move (the golden files and the parity tests depend on them)
_FROZEN = {
    ("resnet18", 224, "unit"): "65c069a5030bca285c1c8a05b99a857f",
    ("resnet18", 224, "timm"): "3f451b5d2e0dc73671fd532f0ca45051",
    ("vit_small_patch16_224", 224, "unit"): "3d7830440844c11879cb142b58f55669",
    ("vit_small_patch16_224", 224, "timm"): "01bde60951da8f3801b5c3e455f720d1",
    ("vit_base_patch16_224", 224, "unit"): "7210b5eb9441854371ab801b37b3f8e8",
    ("vit_base_patch16_224", 224, "timm"): "9053ffcc1bc28fc9813fdf76421a0fb6",
    ("vit_tiny_test", 64, "unit"): "fa139b9704d9fc61cdd94a109066a75b",
    ("vit_tiny_test", 64, "timm"): "f73e9aa9055729dee20f709b3dd6b25b",
}


@pytest.mark.parametrize("key", sorted(_FROZEN))
def test_existing_seeded_streams_unchanged(key):
    arch, img, scale = key
    h = hashlib.sha256()
    for k, v in W.init_state_dict(arch, seed=1, img_size=img, scale=scale).items():
        h.update(k.encode())
        h.update(v.numpy().tobytes())
    assert h.hexdigest()[:32] == _FROZEN[key]


def test_cabi_handle(hip_lib):
    h = ctypes.c_void_p()
    for prec in (0, 1, 2):
        assert hip_lib.effocr_encoder_create(ARCH.encode(), 224, prec, ctypes.byref(h)) == 0
        try:
            assert hip_lib.effocr_encoder_embed_dim(h) == 768
            shapes = W.param_shapes(ARCH)
            n = hip_lib.effocr_encoder_num_params(h)
            names = [hip_lib.effocr_encoder_param_name(h, i).decode() for i in range(n)]
            assert set(names) == set(shapes) and len(names) == len(shapes)
            for i, k in enumerate(names):
                numel = 1
                for d in shapes[k]:
                    numel *= d
                assert hip_lib.effocr_encoder_param_numel(h, i) == numel
            assert hip_lib.effocr_encoder_weights_bytes(h) > 0
            # sub-batches keep the workspace of any call under 1 GiB by default; it grows with the chunk setting only
            ws1 = hip_lib.effocr_encoder_workspace_bytes(h, 1)
            ws = hip_lib.effocr_encoder_workspace_bytes(h, 1024)
            assert 0 < ws1 < ws < (1 << 30)
            assert hip_lib.effocr_encoder_workspace_bytes(h, 192) == ws
            assert hip_lib.effocr_encoder_set_chunk(h, 5) == 0
            assert hip_lib.effocr_encoder_workspace_bytes(h, 1024) == hip_lib.effocr_encoder_workspace_bytes(h, 5) < ws
        finally:
            hip_lib.effocr_encoder_destroy(h)
    for bad in (0, 48, 100, 16):
        assert hip_lib.effocr_encoder_create(ARCH.encode(), bad, 1, ctypes.byref(h)) == -1
    assert hip_lib.effocr_encoder_create(ARCH.encode(), 64, 1, ctypes.byref(h)) == 0
    hip_lib.effocr_encoder_destroy(h)
