"""vit_small_patch8_224 / vit_base_patch8_224 host side (-m "not gpu"): the CPU restatement against transformers' ViTModel(patch_size=8),
the attention references, the parameter tables, the checkpoint loader, the factories and libeffocr_vit8.so's C ABI (exports, version,
refusals) — none of it needs a GPU."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from effocr_amd import _lib
from effocr_amd import weights as W
from tests.vit8_ref import attention_emulated, attention_ref, hf_config, hf_state_dict, vit8_forward

SMALL, BASE, TINY = "vit_small_patch8_224", "vit_base_patch8_224", "vit8_tiny_test"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# by hand: patch conv 192 D + D, cls D, pos 785 D, 12 blocks of 12 D^2 + 13 D, final norm 2 D
N_PARAMS = {SMALL: 21_670_272, BASE: 85_807_872}


def _hf_model(arch, img):
    from transformers import ViTModel
    D, depth, heads, _ = W.VIT8_CFG[arch]
    return ViTModel(hf_config(D, depth, heads, img), add_pooling_layer=False).eval()


def _x(B, img, seed, dtype):
    x = torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(seed), dtype=dtype)
    x[:, :, :6, :6] += 3.0                                 # glyph-like structure: the crops (and their patch tokens) differ
    x[1:, :, -6:, -6:] -= 3.0
    return x


@pytest.mark.parametrize("arch,img,B", [(TINY, 8, 3), (TINY, 48, 3), (TINY, 224, 2), (SMALL, 224, 1)])
def test_restatement_matches_transformers(arch, img, B):
    """fp32 on both sides, bound 1e-5 (max norm relative to max|hf|)."""
    sd = W.init_state_dict(arch, seed=5, img_size=img)
    m = _hf_model(arch, img)
    missing, unexpected = m.load_state_dict(hf_state_dict(sd, list(m.state_dict())), strict=True)
    assert not missing and not unexpected
    x = _x(B, img, B, torch.float32)
    ref = vit8_forward(sd, x)
    with torch.no_grad():
        hf = m(pixel_values=x).last_hidden_state[:, 0]
    assert ref.shape == (B, W.embed_dim(arch))
    rel = ((ref - hf).abs().max() / hf.abs().max()).item()
    print(f"restatement vs transformers, {arch} img {img} B={B}: {rel:.2e}")
    assert rel <= 1e-5
    if B > 1:                                              # the restatement tells crops apart
        assert ((ref[0] - ref[1]).abs().max() / ref.abs().max()).item() > 1e-2


def test_param_table_and_counts():
    for arch in (SMALL, BASE):
        D = W.VIT8_CFG[arch][0]
        shapes = W.param_shapes(arch)
        n = sum(torch.Size(v).numel() for v in shapes.values())
        hf = _hf_model(arch, 224)
        assert n == sum(p.numel() for p in hf.parameters()) == N_PARAMS[arch]
        hf_shapes = {k: tuple(v.shape) for k, v in hf.state_dict().items()}
        mapped = {k: tuple(v.shape) for k, v in hf_state_dict({k: torch.empty(s) for k, s in shapes.items()}, list(hf_shapes)).items()}
        assert mapped == hf_shapes
        assert W.embed_dim(arch) == D and W.is_vit8(arch) and not W.is_vit(arch) and W._family(arch) == "vit8"
        assert shapes["patch_embed.proj.weight"] == (D, 3, 8, 8) and shapes["pos_embed"] == (1, 785, D)
        assert shapes["blocks.11.attn.qkv.bias"] == (3 * D,)
        with_head = W.param_shapes(arch, num_classes=10)
        assert sum(torch.Size(v).numel() for v in with_head.values()) == n + 10 * D + 10
        assert list(with_head)[-2:] == ["head.weight", "head.bias"] == list(W.head_keys(arch))
    assert W.param_shapes(TINY, 64)["pos_embed"] == (1, 65, 128) and not W.is_vit(TINY)
    for img in (0, 4, 12, 100, 232):
        with pytest.raises(ValueError):
            W.param_shapes(SMALL, img)


def test_infer_arch_and_img_size():
    for arch in (SMALL, BASE, TINY):
        for img in (224, 64):
            sd = W.init_state_dict(arch, seed=1, img_size=img, scale="timm", num_classes=3)
            for pref in ("", "net."):
                d = {pref + k: v for k, v in sd.items()}
                assert W.infer_arch(d) == arch
                assert W.vit8_img_size(d) == img
                assert W.infer_num_classes(d) == 3
            W.check_state_dict(arch, sd, img, num_classes=3)
    # the patch-16 ViTs and the other token models get the answers they got before
    assert W.infer_arch(W.init_state_dict("vit_small_patch16_224", scale="timm")) == "vit_small_patch16_224"
    assert W.infer_arch({"net." + k: v for k, v in W.init_state_dict("vit_base_patch16_224", scale="timm").items()}) == "vit_base_patch16_224"
    assert W.infer_arch(W.init_state_dict("vit_tiny_test", img_size=64)) == "vit_tiny_test"
    assert W.infer_arch(W.init_state_dict("beit_tiny_test", img_size=64)) == "beit_tiny_test"
    assert W.infer_arch(W.init_state_dict("swin_tiny_patch4_window7_224", scale="timm")) == "swin_tiny_patch4_window7_224"
    # a patch-8 model of another width, a pos_embed that is no grid
    sd = W.init_state_dict(TINY, img_size=16)
    odd = {k: (torch.zeros(1, 5, 256) if k == "pos_embed" else v) for k, v in sd.items()}
    with pytest.raises(ValueError, match="unsupported patch-8 ViT"):
        W.infer_arch(odd)
    with pytest.raises(ValueError, match="7 rows"):
        W.vit8_img_size({"pos_embed": torch.zeros(1, 7, 128)})


def test_check_state_dict_names_what_is_wrong():
    sd = W.init_state_dict(SMALL, seed=0, scale="timm")
    bad = dict(sd)
    bad["patch_embed.proj.weight"] = torch.zeros(384, 3, 16, 16)
    with pytest.raises(ValueError, match=r"patch_embed\.proj\.weight: shape \(384, 3, 16, 16\)"):
        W.check_state_dict(SMALL, bad)
    missing = dict(sd)
    del missing["pos_embed"]
    with pytest.raises(ValueError, match="missing pos_embed"):
        W.check_state_dict(SMALL, missing)
    with pytest.raises(ValueError, match="pos_embed"):     # a 224^2 checkpoint asked to run at 64^2
        W.check_state_dict(SMALL, sd, 64)


def test_seeded_init_is_deterministic_and_nontrivial():
    a, b, c = (W.init_state_dict(TINY, seed=s, img_size=64) for s in (9, 9, 10))
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["patch_embed.proj.weight"], c["patch_embed.proj.weight"])
    for k in ("blocks.0.attn.qkv.bias", "blocks.1.attn.proj.bias", "blocks.1.mlp.fc1.bias", "patch_embed.proj.bias", "norm.bias"):
        assert a[k].abs().max() > 0, k
    assert 0.5 <= a["norm.weight"].min() and a["norm.weight"].max() <= 1.5
    t = W.init_state_dict(TINY, seed=9, img_size=64, scale="timm")
    assert torch.all(t["norm.weight"] == 1) and torch.all(t["blocks.1.norm1.bias"] == 0) and t["pos_embed"].abs().max() <= 0.04
    tr = W.init_state_dict(TINY, seed=9, img_size=64, scale="trained")
    assert tr["blocks.0.mlp.fc2.weight"].std() < 0.5 * a["blocks.0.mlp.fc2.weight"].std()
    with pytest.raises(ValueError):
        W.init_state_dict(TINY, scale="huge")
    h = W.init_state_dict(TINY, seed=9, img_size=64, num_classes=5)
    assert all(torch.equal(h[k], a[k]) for k in a) and h["head.weight"].shape == (5, 128)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_attention_emulation_is_the_reference_up_to_rounding(dtype):
    """attention_emulated walks tiles with a running softmax: with no rounding (float64 as the 'type') it equals attention_ref to 1e-14,
    whatever the tile size; with a 16-bit type its distance is a few units of that type's half-ulp — nonzero, so a bound made of it is
    a real bound."""
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(2, 2, 197, 64, generator=g).to(dtype) for _ in range(3))
    ref = attention_ref(q, k, v)
    for tile in (64, 16, 1000):
        exact = attention_emulated(q, k, v, torch.float64, key_tile=tile)
        assert ((exact - ref).abs().max() / ref.abs().max()).item() < 1e-13
    e = ((attention_emulated(q, k, v, dtype) - ref).abs().max() / ref.abs().max()).item()
    half_ulp = 2.0 ** -12 if dtype == torch.float16 else 2.0 ** -9
    assert 0.1 * half_ulp < e < 8 * half_ulp, e
    # a wrong mean is far outside: q = k = 0 makes every row the mean of the T value rows; T - 1 of them is off by ~1/T
    z = torch.zeros_like(q)
    mean = attention_ref(z, z, v)
    assert torch.allclose(mean, v.double().mean(-2, keepdim=True).expand_as(mean), atol=1e-14)
    short = v[..., :-1, :].double().mean(-2, keepdim=True).expand_as(mean)
    assert ((short - mean).abs().max() / mean.abs().max()).item() > 20 * e


# -- libeffocr_vit8.so ------------------------------------------------------------------------------------------------------------
def test_vit8_library_exports_its_header_and_versions_agree():
    src = open(os.path.join(ROOT, "include", "effocr_vit8.h")).read()
    declared = sorted(set(re.findall(r"\b(effocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert len(declared) == 18
    raw = ctypes.CDLL(_lib.VIT8_SO_PATH)
    for n in declared:
        assert hasattr(raw, n), f"{n} declared in effocr_vit8.h but not exported"
    assert sorted(_lib.VIT8_EXPORTS) == declared
    v = int(re.search(r"#define\s+EFFOCR_VIT8_ABI_VERSION\s+(\d+)", src).group(1))
    assert _lib.vit8_lib().effocr_vit8_abi_version() == v == _lib.VIT8_ABI_VERSION == 1
    # it exports effocr_vit8_* only: the dynamic symbol table holds no other defined symbol
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.VIT8_SO_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    defined = sorted(line.split()[-1] for line in nm.splitlines())
    assert defined == declared, defined
    for hidden in ("_ZN6effocr7gemm_ntEiiRKNS_8GemmArgsEP12ihipStream_t", "effocr_abi_version", "effocr_encoder_create", "effocr_beit_create"):
        assert not hasattr(raw, hidden), hidden
    _lib.lib()
    assert not set(declared) & set(_lib.EXPORTS)
    assert not hasattr(ctypes.CDLL(_lib.SO_PATH), "effocr_vit8_create")


def test_product_library_still_refuses_patch8(hip_lib):
    h = ctypes.c_void_p()
    for name in (SMALL, BASE, TINY):
        assert hip_lib.effocr_encoder_create(name.encode(), 224, 1, ctypes.byref(h)) == -2


def test_vit8_handle_and_refusals():
    L = _lib.vit8_lib()
    h = ctypes.c_void_p()
    for arch, img, D in ((SMALL, 224, 384), (BASE, 224, 768), (TINY, 64, 128), (TINY, 8, 128)):
        shapes = W.param_shapes(arch, img)
        for prec in (0, 1, 2):
            assert L.effocr_vit8_create(arch.encode(), img, prec, ctypes.byref(h)) == 0
            try:
                assert L.effocr_vit8_embed_dim(h) == D
                n = L.effocr_vit8_num_params(h)
                names = [L.effocr_vit8_param_name(h, i).decode() for i in range(n)]
                assert names == list(shapes)
                for i, k in enumerate(names):
                    assert L.effocr_vit8_param_numel(h, i) == torch.Size(shapes[k]).numel()
                assert L.effocr_vit8_param_name(h, n) is None and L.effocr_vit8_param_numel(h, -1) == -1
                assert L.effocr_vit8_weights_bytes(h) > 0
                ws1 = L.effocr_vit8_workspace_bytes(h, 1)
                ws = L.effocr_vit8_workspace_bytes(h, 4096)
                assert 0 < ws1 < ws < 1000 * (1 << 20)                    # sub-batches keep the workspace under 1 GB
                assert L.effocr_vit8_workspace_bytes(h, 0) == 0
                assert L.effocr_vit8_set_chunk(h, 5) == 0
                assert L.effocr_vit8_workspace_bytes(h, 4096) == L.effocr_vit8_workspace_bytes(h, 5) < ws
                assert L.effocr_vit8_set_chunk(h, -1) == -1
                one = torch.zeros(1)
                assert L.effocr_vit8_set_param(h, b"norm.weight", _lib.ptr(one), 1) == -1
                assert f"expects {D}".encode() in L.effocr_vit8_last_error()
                for absent in (b"head.weight", b"fc_norm.weight", b"blocks.0.gamma_1"):
                    assert L.effocr_vit8_set_param(h, absent, _lib.ptr(one), 1) == -1
                assert L.effocr_vit8_set_param(h, None, _lib.ptr(one), 1) == -1
                # upload before every parameter is set, forward before upload
                p = ctypes.c_void_p(4096)                                  # never dereferenced: these calls are refused first
                assert L.effocr_vit8_upload(h, p, L.effocr_vit8_weights_bytes(h)) == -5
                assert L.effocr_vit8_upload(h, p, 1) == -3
                assert L.effocr_vit8_upload(h, None, 1 << 30) == -1
                assert L.effocr_vit8_forward(h, p, 2, p, 0, p, 1 << 40, None) == -5
                assert L.effocr_vit8_forward(h, p, -1, p, 0, p, 1 << 40, None) == -1
                assert L.effocr_vit8_forward(h, None, 2, p, 0, p, 1 << 40, None) == -1
                assert L.effocr_vit8_forward(h, p, 0, p, 0, p, 0, None) == 0
                assert L.effocr_vit8_check_status(h, None, None) == -1
                assert L.effocr_vit8_reset_status(h, None, None) == -1
            finally:
                L.effocr_vit8_destroy(h)
    for size in (0, 4, 12, 100, 232, 384, -8):
        assert L.effocr_vit8_create(SMALL.encode(), size, 1, ctypes.byref(h)) == -1
        assert b"multiple of 8" in L.effocr_vit8_last_error()
    for prec in (-1, 3):
        assert L.effocr_vit8_create(SMALL.encode(), 224, prec, ctypes.byref(h)) == -1
    for name in (b"vit_small_patch16_224", b"xcit_small_12_p8_224", b"vit_base_patch16_384", b"vit_small_patch32_224"):
        assert L.effocr_vit8_create(name, 224, 1, ctypes.byref(h)) == -2
    assert L.effocr_vit8_create(None, 224, 1, ctypes.byref(h)) == -1
    assert L.effocr_vit8_create(SMALL.encode(), 224, 1, None) == -1
    assert L.effocr_vit8_forward(None, None, 1, None, 0, None, 0, None) == -1
    assert L.effocr_vit8_embed_dim(None) == 0 and L.effocr_vit8_num_params(None) == 0
    p = ctypes.c_void_p(4096)
    assert L.effocr_vit8_op_attn(None, 1, 5, 2, 1, p, None) == -1
    assert L.effocr_vit8_op_attn(p, 0, 5, 2, 1, p, None) == -1
    for tokens in (0, 1025):
        assert L.effocr_vit8_op_attn(p, 1, tokens, 2, 1, p, None) == -2           # refused before any launch
    assert L.effocr_vit8_op_patch_embed(p, 1, 16, 128, 1, p, p, p, p, p, None, None) == -1
    assert L.effocr_vit8_op_patch_embed(p, 1, 16, 100, 1, p, p, p, p, p, p, None) == -1
    assert L.effocr_vit8_op_patch_embed(p, 1, 12, 128, 1, p, p, p, p, p, p, None) == -1   # img 12: refused before any launch


def test_factories_accept_patch8(tmp_path):
    from effocr_amd import EffOCRHipError
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.encoders import AutoEncoderFactory, Vit8Encoder, make_encoder
    for arch in (SMALL, BASE):
        enc = AutoEncoderFactory("timm", arch)()           # NotImplementedError before libeffocr_vit8.so existed
        assert enc.arch == arch
        assert sum(p.numel() for _, p in enc.named_parameters()) == N_PARAMS[arch]
    sd = W.init_state_dict(TINY, seed=4, img_size=64, num_classes=7)
    W.save_checkpoint(sd, tmp_path / "clf.pth")
    clf = AutoClassifierFactory("timm", TINY, n_classes=7, img_size=64).load(str(tmp_path / "clf.pth"))
    got = clf.state_dict()
    assert sorted(got) == sorted("net." + k for k in sd) and all(torch.equal(got["net." + k], v) for k, v in sd.items())
    enc = AutoEncoderFactory("timm", TINY, img_size=64).load(str(tmp_path / "clf.pth"))
    if not torch.cuda.is_available():                      # no GPU: a loud failure, never NotImplementedError or a fallback
        from effocr_amd.recognizer_engine import EffRecognizer
        with pytest.raises(EffOCRHipError):
            enc.to("cuda")(torch.zeros(1, 3, 64, 64))
        with pytest.raises(EffOCRHipError):
            clf.to("cuda")(torch.zeros(1, 3, 64, 64))
        with pytest.raises(EffOCRHipError):
            make_encoder(TINY, sd, img_size=64)
        with pytest.raises(EffOCRHipError):
            Vit8Encoder(SMALL, W.init_state_dict(SMALL, scale="timm"))
        with pytest.raises(EffOCRHipError):
            EffRecognizer(str(tmp_path / "clf.pth"))
    # names that raise today still raise
    for name in ("vit_small_patch16_384", "vit_base_patch32_224", "vit_large_patch8_224", "xcit_small_12_p8_224"):
        with pytest.raises(NotImplementedError):
            AutoEncoderFactory("timm", name)
    with pytest.raises(NotImplementedError):
        AutoEncoderFactory("hf", "facebook/dino-vits8")
