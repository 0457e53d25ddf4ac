"""swin_tiny_patch4_window7_224 host side (-m "not gpu"): the CPU restatement against transformers' SwinModel, the parameter tables, both
timm checkpoint layouts, checkpoint I/O, seeded init, and libeffocr_swin.so's C ABI (exports, version, refusals) — none of it needs a GPU."""
import ctypes
import hashlib
import os
import re

import pytest
import torch

from effocr_amd import _lib
from effocr_amd import weights as W
from tests.swin_ref import hf_state_dict, swin_forward

ARCH = "swin_tiny_patch4_window7_224"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PARAMS = 27_519_354


def _hf_model():
    from transformers import SwinConfig, SwinModel
    return SwinModel(SwinConfig(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7)).eval().double()


@pytest.mark.parametrize("B", [1, 3])
def test_restatement_matches_transformers(B):
    # scale="unit": random LayerNorm gains and biases, bias tables N(0, 1) — a wrong relative index, mask, roll or merge order moves
    # the output by O(1)
    sd = W.init_state_dict(ARCH, seed=5)
    m = _hf_model()
    missing, unexpected = m.load_state_dict(hf_state_dict(sd), strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B), dtype=torch.float64)
    # glyph-like structure near window borders: bright corners of the crop
    x[:, :, :12, :12] += 4.0
    x[:, :, -12:, -12:] -= 4.0
    ref = swin_forward(ARCH, sd, x)
    with torch.no_grad():
        hf = m(pixel_values=x).pooler_output
    assert ref.shape == (B, 768)
    rel = ((ref - hf).abs().max() / hf.abs().max()).item()
    print(f"restatement vs transformers, B={B}: {rel:.2e}")
    assert rel <= 1e-10


def test_restatement_depends_on_mask_and_bias():
    """The restatement is sensitive to the shift mask: dropping it moves the output far beyond any tolerance of the GPU tests (the
    crops of those tests exercise it on every shifted block)."""
    import tests.swin_ref as R
    sd = W.init_state_dict(ARCH, seed=6)
    x = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    ref = swin_forward(ARCH, sd, x)
    saved = R.region_mask
    try:
        R.region_mask = lambda H, W_, ws, shift, dtype: torch.zeros(1, dtype=dtype)
        nomask = swin_forward(ARCH, sd, x)
    finally:
        R.region_mask = saved
    assert ((nomask - ref).norm() / ref.norm()).item() > 1e-2


def test_param_table_and_counts():
    shapes = W.param_shapes(ARCH)
    assert W.embed_dim(ARCH) == 768
    assert shapes["patch_embed.proj.weight"] == (96, 3, 4, 4)
    assert shapes["layers.1.downsample.norm.weight"] == (384,)
    assert shapes["layers.3.downsample.reduction.weight"] == (768, 1536)
    assert shapes["layers.2.blocks.5.attn.relative_position_bias_table"] == (169, 12)
    assert shapes["layers.3.blocks.1.attn.qkv.weight"] == (2304, 768)
    assert "layers.0.downsample.norm.weight" not in shapes and "layers.2.blocks.6.norm1.weight" not in shapes
    n = sum(torch.Size(v).numel() for v in shapes.values())
    assert n == N_PARAMS
    hf = _hf_model()
    assert sum(p.numel() for p in hf.parameters()) == N_PARAMS
    hf_shapes = {k: tuple(v.shape) for k, v in hf.state_dict().items()}
    mapped = {k: tuple(v.shape) for k, v in hf_state_dict({k: torch.empty(s) for k, s in shapes.items()}).items()}
    assert mapped == hf_shapes
    with_head = W.param_shapes(ARCH, num_classes=10)
    assert sum(torch.Size(v).numel() for v in with_head.values()) == N_PARAMS + 7_690
    assert list(with_head)[-2:] == ["head.fc.weight", "head.fc.bias"]


def _old_layout(sd):
    """timm < 0.9: patch merging at the end of stages 0-2, classifier `head`, derived buffers in the checkpoint."""
    out = {}
    for k, v in sd.items():
        m = re.match(r"layers\.(\d+)\.downsample\.(.*)", k)
        if m:
            k = f"layers.{int(m.group(1)) - 1}.downsample.{m.group(2)}"
        elif k.startswith("head.fc."):
            k = "head." + k[len("head.fc."):]
        out[k] = v
    out["layers.0.blocks.1.attn_mask"] = torch.zeros(64, 49, 49)
    out["layers.1.blocks.0.attn.relative_position_index"] = torch.zeros(49, 49, dtype=torch.long)
    return out


def test_infer_arch_both_layouts_and_check_state_dict():
    sd = W.init_state_dict(ARCH, seed=0, num_classes=10)
    old = _old_layout(sd)
    assert "layers.0.downsample.reduction.weight" in old and "head.weight" in old
    for variant in (sd, old):
        for pref in ("", "net."):
            d = {pref + k: v for k, v in variant.items()}
            assert W.infer_arch(d) == ARCH
            canon = W.strip_prefix(d)
            assert sorted(canon) == sorted(sd)
            assert all(torch.equal(canon[k], sd[k]) for k in sd)
            assert W.infer_num_classes(d) == 10
    W.check_state_dict(ARCH, sd)
    W.check_state_dict(ARCH, sd, num_classes=10)
    bad = dict(sd)
    bad["layers.2.blocks.3.attn.qkv.weight"] = torch.zeros(1152, 383)
    with pytest.raises(ValueError, match="layers.2.blocks.3.attn.qkv.weight"):
        W.check_state_dict(ARCH, bad)
    bad = dict(sd)
    bad["layers.1.blocks.0.attn.relative_position_bias_table"] = torch.zeros(169, 5)
    with pytest.raises(ValueError, match="relative_position_bias_table"):
        W.check_state_dict(ARCH, bad)
    missing = dict(sd)
    del missing["layers.3.downsample.norm.bias"]
    with pytest.raises(ValueError, match="missing layers.3.downsample.norm.bias"):
        W.check_state_dict(ARCH, missing)


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
    # a timm < 0.9 checkpoint loads into the same tensors
    W.save_checkpoint(_old_layout(sd), tmp_path / ("old" + suffix))
    back = W.load_checkpoint(tmp_path / ("old" + suffix))
    assert sorted(back) == sorted(sd) and all(torch.equal(back[k], sd[k]) for k in sd)


def test_factories_accept_swin(tmp_path):
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.encoders import AutoEncoderFactory
    enc = AutoEncoderFactory("timm", ARCH)()
    assert sum(p.numel() for _, p in enc.named_parameters()) == N_PARAMS
    sd = W.init_state_dict(ARCH, seed=4, num_classes=7)
    W.save_checkpoint(_old_layout(sd), tmp_path / "clf.pth")
    clf = AutoClassifierFactory("timm", ARCH, n_classes=7).load(str(tmp_path / "clf.pth"))
    got = clf.state_dict()
    assert sorted(got) == sorted("net." + k for k in sd) and all(torch.equal(got["net." + k], v) for k, v in sd.items())
    # names that raise today still raise
    for name in ("xcit_small_12_p8_224", "swin_small_patch4_window7_224"):
        with pytest.raises(NotImplementedError):
            AutoEncoderFactory("timm", name)
    with pytest.raises(NotImplementedError):
        AutoEncoderFactory("hf", ARCH)


def test_seeded_init_is_deterministic_and_nontrivial():
    a = W.init_state_dict(ARCH, seed=9)
    b = W.init_state_dict(ARCH, seed=9)
    c = W.init_state_dict(ARCH, seed=10)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["patch_embed.proj.weight"], c["patch_embed.proj.weight"])
    for k in ("patch_embed.norm.weight", "layers.2.downsample.norm.weight", "layers.0.blocks.1.norm1.weight", "norm.weight"):
        assert 0.5 <= a[k].min() and a[k].max() <= 1.5 and a[k].std() > 0.1, k
    assert abs(a["layers.1.blocks.0.attn.relative_position_bias_table"].std().item() - 1.0) < 0.1
    assert abs(a["layers.3.blocks.0.mlp.fc2.weight"].std().item() - 1 / 3072 ** 0.5) < 2e-3
    t = W.init_state_dict(ARCH, seed=9, scale="timm")
    assert torch.all(t["norm.weight"] == 1) and torch.all(t["layers.1.downsample.norm.bias"] == 0)
    assert abs(t["layers.2.blocks.0.mlp.fc1.weight"].std().item() - 0.02) < 0.003
    h = W.init_state_dict(ARCH, seed=9, num_classes=5)
    assert all(torch.equal(h[k], a[k]) for k in a) and h["head.fc.weight"].shape == (5, 768)


# sha256 (first 32 hex digits) over (key, fp32 bytes) of init_state_dict(arch, seed=1, img_size, scale), taken on the tree BEFORE
# Swin was added: the other architectures' seeded streams must not move
_FROZEN = {
    ("resnet18", 224, "unit"): "65c069a5030bca285c1c8a05b99a857f",
    ("vit_small_patch16_224", 224, "unit"): "3d7830440844c11879cb142b58f55669",
    ("vit_base_patch16_224", 224, "timm"): "9053ffcc1bc28fc9813fdf76421a0fb6",
    ("vit_tiny_test", 64, "unit"): "fa139b9704d9fc61cdd94a109066a75b",
    ("convnext_tiny", 224, "unit"): "145739ab4c744687a0fa7b55ea5cbb75",
    ("convnext_tiny", 224, "timm"): "40bc3448f2f1491649ece4271ea27ee4",
    ("mobilenetv3_small_050", 224, "unit"): "0818591024e206f52c23ac4a7b6c9bcc",
    ("mobilenetv3_small_050", 224, "timm"): "4fea2eb4c3ea8b8953a50d28d4884e47",
}


def _digest(arch, img, scale):
    h = hashlib.sha256()
    for k, v in W.init_state_dict(arch, seed=1, img_size=img, scale=scale).items():
        h.update(k.encode())
        h.update(v.numpy().tobytes())
    return h.hexdigest()[:32]


@pytest.mark.parametrize("key", sorted(_FROZEN))
def test_other_seeded_streams_unchanged(key):
    assert _digest(*key) == _FROZEN[key]


# -- libeffocr_swin.so ------------------------------------------------------------------------------------------------------------
def test_swin_library_exports_its_header_and_versions_agree():
    src = open(os.path.join(ROOT, "include", "effocr_swin.h")).read()
    declared = sorted(set(re.findall(r"\b(effocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert len(declared) == 15
    raw = ctypes.CDLL(_lib.SWIN_SO_PATH)
    for n in declared:
        assert hasattr(raw, n), f"{n} declared in effocr_swin.h but not exported"
    assert sorted(_lib.SWIN_EXPORTS) == declared
    v = int(re.search(r"#define\s+EFFOCR_SWIN_ABI_VERSION\s+(\d+)", src).group(1))
    assert _lib.swin_lib().effocr_swin_abi_version() == v == _lib.SWIN_ABI_VERSION
    # the GEMMs compiled into it stay hidden, and the product library neither gains nor loses anything
    for hidden in ("_ZN6effocr7gemm_ntEiiRKNS_8GemmArgsEP12ihipStream_t", "effocr_abi_version", "effocr_encoder_create"):
        assert not hasattr(raw, hidden), hidden
    _lib.lib()
    assert not set(declared) & set(_lib.EXPORTS)
    assert not hasattr(ctypes.CDLL(_lib.SO_PATH), "effocr_swin_create")


def test_product_library_still_refuses_swin(hip_lib):
    h = ctypes.c_void_p()
    assert hip_lib.effocr_encoder_create(ARCH.encode(), 224, 1, ctypes.byref(h)) == -2


def test_swin_handle_and_refusals():
    L = _lib.swin_lib()
    h = ctypes.c_void_p()
    shapes = W.param_shapes(ARCH)
    for prec in (0, 1, 2):
        assert L.effocr_swin_create(ARCH.encode(), 224, prec, ctypes.byref(h)) == 0
        try:
            assert L.effocr_swin_embed_dim(h) == 768
            n = L.effocr_swin_num_params(h)
            names = [L.effocr_swin_param_name(h, i).decode() for i in range(n)]
            assert names == list(shapes)
            for i, k in enumerate(names):
                assert L.effocr_swin_param_numel(h, i) == torch.Size(shapes[k]).numel()
            assert L.effocr_swin_param_name(h, n) is None and L.effocr_swin_param_numel(h, -1) == -1
            assert L.effocr_swin_weights_bytes(h) > 0
            ws1 = L.effocr_swin_workspace_bytes(h, 1)
            ws = L.effocr_swin_workspace_bytes(h, 1024)
            assert 0 < ws1 < ws < 1000 * (1 << 20)                    # sub-batches keep the workspace under 1 GB
            assert L.effocr_swin_workspace_bytes(h, 0) == 0
            assert L.effocr_swin_set_chunk(h, 5) == 0
            assert L.effocr_swin_workspace_bytes(h, 1024) == L.effocr_swin_workspace_bytes(h, 5) < ws
            assert L.effocr_swin_set_chunk(h, -1) == -1
            one = torch.zeros(1)
            assert L.effocr_swin_set_param(h, b"norm.weight", _lib.ptr(one), 1) == -1
            assert b"expects 768" in L.effocr_swin_last_error()
            assert L.effocr_swin_set_param(h, b"head.fc.weight", _lib.ptr(one), 1) == -1
            assert L.effocr_swin_set_param(h, None, _lib.ptr(one), 1) == -1
            # upload before every parameter is set, forward before upload
            p = ctypes.c_void_p(4096)                                  # never dereferenced: these calls are refused first
            assert L.effocr_swin_upload(h, p, L.effocr_swin_weights_bytes(h)) == -5
            assert L.effocr_swin_upload(h, p, 1) == -3
            assert L.effocr_swin_upload(h, None, 1 << 30) == -1
            assert L.effocr_swin_forward(h, p, 2, p, 0, p, 1 << 40, None) == -5
            assert L.effocr_swin_forward(h, p, -1, p, 0, p, 1 << 40, None) == -1
            assert L.effocr_swin_forward(h, None, 2, p, 0, p, 1 << 40, None) == -1
            assert L.effocr_swin_forward(h, p, 0, p, 0, p, 0, None) == 0
            assert L.effocr_swin_check_status(h, None, None) == -1
        finally:
            L.effocr_swin_destroy(h)
    for size in (0, 192, 256, 448):
        assert L.effocr_swin_create(ARCH.encode(), size, 1, ctypes.byref(h)) == -2
        assert b"224" in L.effocr_swin_last_error()
    for prec in (-1, 3):
        assert L.effocr_swin_create(ARCH.encode(), 224, prec, ctypes.byref(h)) == -1
    assert L.effocr_swin_create(b"swin_small_patch4_window7_224", 224, 1, ctypes.byref(h)) == -2
    assert L.effocr_swin_create(None, 224, 1, ctypes.byref(h)) == -1
    assert L.effocr_swin_create(ARCH.encode(), 224, 1, None) == -1
    assert L.effocr_swin_forward(None, None, 1, None, 0, None, 0, None) == -1
    assert L.effocr_swin_embed_dim(None) == 0 and L.effocr_swin_num_params(None) == 0
