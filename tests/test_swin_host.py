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
    assert len(declared) == 21
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


def test_swin_op_entry_points_check_their_arguments():
    """Every effocr_swin_op_* call below is refused on the host, before any launch: NULL pointers, non-positive sizes, unknown precision
    or epilogue -> -1; what the launcher cannot do -> -2; each with a message."""
    L = _lib.swin_lib()
    p, s = ctypes.c_void_p(4096), None                                            # (never dereferenced)

    def refused(rc, code):
        assert rc == code, (rc, L.effocr_swin_last_error())
        assert L.effocr_swin_last_error()

    stem = lambda x=p, B=1, S=8, w=p, b=p, g=p, be=p, C0=96, o=p: L.effocr_swin_op_stem(x, B, S, w, b, g, be, C0, o, s)
    for kw in (dict(x=None), dict(w=None), dict(b=None), dict(g=None), dict(be=None), dict(o=None), dict(B=0), dict(S=0), dict(C0=0), dict(S=-4)):
        refused(stem(**kw), -1)
    for kw in (dict(S=10), dict(C0=132), dict(C0=94)):                            # S % 4; beyond the 128 channels; C0 % 4
        refused(stem(**kw), -2)

    ln = lambda pr=2, x=p, M=4, C=96, Cp=128, g=p, b=p, o=p: L.effocr_swin_op_layernorm(pr, x, M, C, Cp, g, b, o, s)
    for kw in (dict(x=None), dict(g=None), dict(b=None), dict(o=None), dict(M=0), dict(C=0), dict(Cp=-128), dict(pr=3), dict(pr=-1)):
        refused(ln(**kw), -1)
    for kw in (dict(Cp=192, C=96), dict(Cp=1152, C=1152), dict(C=256, Cp=128), dict(C=94)):   # Cp % 128; > 1024; C > Cp; C % 4
        refused(ln(**kw), -2)

    mg = lambda pr=2, x=p, B=1, H=4, C=96, Cp=128, g=p, b=p, o=p: L.effocr_swin_op_merge(pr, x, B, H, C, Cp, g, b, o, s)
    for kw in (dict(x=None), dict(g=None), dict(b=None), dict(o=None), dict(B=0), dict(H=0), dict(C=0), dict(Cp=0), dict(pr=3)):
        refused(mg(**kw), -1)
    for kw in (dict(C=48), dict(H=5), dict(C=416, Cp=512), dict(C=256, Cp=128), dict(Cp=130)):   # C % 32; odd H; C > 384; C > Cp; Cp % 4
        refused(mg(**kw), -2)

    wa = lambda pr=2, q=p, B=1, H=14, C=96, Cp=128, sh=3, t=p, o=p: L.effocr_swin_op_window_attention(pr, q, B, H, C, Cp, sh, t, o, s)
    for kw in (dict(q=None), dict(t=None), dict(o=None), dict(B=0), dict(H=0), dict(C=0), dict(Cp=0), dict(pr=3)):
        refused(wa(**kw), -1)
    for kw in (dict(H=12), dict(C=48), dict(sh=7), dict(sh=-1), dict(H=7, sh=3), dict(C=256, Cp=128), dict(Cp=132)):
        refused(wa(**kw), -2)                                                     # H % 7; C % 32; shift >= 7; < 0; with one window; ...

    hd = lambda x=p, B=1, T=4, C=128, Cp=256, g=p, b=p, l2=1, e=p, st=p: L.effocr_swin_op_head(x, B, T, C, Cp, g, b, l2, e, st, s)
    for kw in (dict(x=None), dict(g=None), dict(b=None), dict(e=None), dict(st=None), dict(B=0), dict(T=0), dict(C=0), dict(Cp=0)):
        refused(hd(**kw), -1)
    for kw in (dict(C=96, Cp=128), dict(C=1152, Cp=1152), dict(C=256, Cp=128), dict(Cp=258)):
        refused(hd(**kw), -2)

    li = lambda pr=2, epi=0, x=p, w=p, b=p, r=None, o=p, M=4, N=128, K=128: L.effocr_swin_op_linear(pr, epi, x, w, b, r, o, M, N, K, s)
    for kw in (dict(x=None), dict(w=None), dict(b=None), dict(o=None), dict(M=0), dict(N=0), dict(K=0), dict(pr=3), dict(epi=3), dict(epi=4),
               dict(epi=6), dict(epi=-1), dict(epi=2)):                            # (EPI_BIAS_RESID without a residual)
        refused(li(**kw), -1)
    for kw in (dict(N=192), dict(K=48), dict(pr=0, K=96), dict(M=1 << 24, N=128, K=128), dict(M=1 << 20, K=3072, N=128)):
        refused(li(**kw), -2)
    assert b"32-bit" in L.effocr_swin_last_error()
