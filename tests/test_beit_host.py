"""beit_base_patch16_224 / beitv2_base_patch16_224 host side (-m "not gpu"): the CPU restatement against transformers' BeitModel, what
that parity check can and cannot see, the relative-position index, the parameter tables, the factories, the checkpoint loader and
libeffocr_beit.so's C ABI (exports, version, refusals) — none of it needs a GPU."""
import ctypes
import os
import re

import pytest
import torch

from effocr_amd import _lib
from effocr_amd import weights as W
from tests.beit_ref import beit_forward, hf_config, hf_state_dict

ARCH, ARCH2, TINY = "beit_base_patch16_224", "beitv2_base_patch16_224", "beit_tiny_test"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PARAMS = 85_761_984                                      # 12 x 7 097 424 + 590 592 + 768 + 1 536


def _hf_model(arch, img):
    from transformers import BeitModel
    return BeitModel(hf_config(arch, img)).eval().double()


def _x(B, img, seed):
    x = torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    x[:, :, :12, :12] += 3.0                               # glyph-like structure: the crops (and their patch tokens) differ
    x[1:, :, -12:, -12:] -= 3.0
    return x


@pytest.mark.parametrize("arch,img,B", [(TINY, 64, 3), (TINY, 32, 3), (ARCH, 224, 2)])
def test_restatement_matches_transformers(arch, img, B):
    # scale="unit": random LayerNorm gains, biases N(0, 0.1), bias tables N(0, 1), layer scale 0.1.  Bound 1e-5, the other families'
    # host bound; transformers keeps a float32 step in its bias path, so the difference is ~1e-7 and not 1e-14.
    sd = W.init_state_dict(arch, seed=5, img_size=img)
    m = _hf_model(arch, img)
    missing, unexpected = m.load_state_dict(hf_state_dict(sd), strict=False)
    assert not unexpected and all(k.endswith("relative_position_index") for k in missing), (missing, unexpected)
    x = _x(B, img, B)
    ref = beit_forward(arch, sd, x)
    with torch.no_grad():
        hf = m(pixel_values=x).pooler_output
    assert ref.shape == (B, W.embed_dim(arch))
    rel = ((ref - hf).abs().max() / hf.abs().max()).item()
    print(f"restatement vs transformers, {arch} img {img} B={B}: {rel:.2e}")
    assert rel <= 1e-5


@pytest.mark.parametrize("mistake", ["swap_ij", "swap_cls", "q_bias_on_k", "mean_with_cls", "no_fc_norm"])
def test_parity_sees_each_planted_mistake(mistake):
    """Each of these, alone, moves the restatement's output by more than 1e-2 (relative L2): a GPU parity test against it pins them.
    q_bias_on_k is q's bias landing in k's slot of the packed bias vector, [0 | q_bias | v_bias]."""
    sd = W.init_state_dict(TINY, seed=6, img_size=64)
    x = _x(3, 64, 0)
    ref = beit_forward(TINY, sd, x)
    bad = beit_forward(TINY, sd, x, **{mistake: True})
    moved = ((bad - ref).norm() / ref.norm()).item()
    print(f"{mistake}: moves the output by {moved:.2e}")
    assert moved > 1e-2


def test_a_bias_added_to_k_alone_is_invisible():
    """k given q_bias ON TOP of q keeping its own, [q_bias | q_bias | v_bias], adds q_i . b to every score of row i: softmax cancels it.
    No parity test can see that variant (it is why BEiT has no k bias); the visible form of the mistake is q_bias_on_k above."""
    sd = W.init_state_dict(TINY, seed=6, img_size=64)
    x = _x(3, 64, 0)
    ref = beit_forward(TINY, sd, x)
    same = beit_forward(TINY, sd, x, k_bias_added=True)
    assert ((same - ref).norm() / ref.norm()).item() < 1e-12


@pytest.mark.parametrize("Wn", [1, 2, 4, 8, 14])
def test_relative_position_index_is_the_linear_code_form(Wn):
    idx = W.beit_relative_position_index(Wn)
    T, n = Wn * Wn + 1, (2 * Wn - 1) ** 2
    assert idx.shape == (T, T) and idx.dtype == torch.long
    p = torch.arange(Wn * Wn)
    code = (p // Wn) * (2 * Wn - 1) + p % Wn
    assert torch.equal(idx[1:, 1:], code[:, None] - code[None, :] + 2 * Wn * (Wn - 1))
    assert torch.all(idx[0, 1:] == n) and torch.all(idx[1:, 0] == n + 1) and idx[0, 0] == n + 2
    assert idx[1:, 1:].min() == 0 and idx[1:, 1:].max() == n - 1
    # transformers builds the same array (a buffer of its relative-position-bias module)
    from transformers import BeitModel
    m = BeitModel(hf_config(TINY, 16 * Wn))
    hf = [b for k, b in m.named_buffers() if k.endswith("relative_position_index")]
    if hf:
        assert torch.equal(hf[0].view(T, T), idx)


def test_param_table_and_counts():
    for arch in (ARCH, ARCH2):
        shapes = W.param_shapes(arch)
        assert W.embed_dim(arch) == 768 and W.is_beit(arch) and W._family(arch) == "beit"
        assert sum(torch.Size(v).numel() for v in shapes.values()) == N_PARAMS
        assert "pos_embed" not in shapes and "blocks.0.attn.qkv.bias" not in shapes and "norm.weight" not in shapes
        assert shapes["blocks.11.attn.relative_position_bias_table"] == (732, 12)
        assert shapes["blocks.3.attn.qkv.weight"] == (2304, 768) and shapes["blocks.3.gamma_2"] == (768,)
    assert list(W.param_shapes(ARCH)) == list(W.param_shapes(ARCH2))
    hf = _hf_model(ARCH, 224)
    assert sum(p.numel() for p in hf.parameters()) == N_PARAMS
    hf_shapes = {k: tuple(v.shape) for k, v in hf.state_dict().items() if not k.endswith("relative_position_index")}
    mapped = {k: tuple(v.shape) for k, v in hf_state_dict({k: torch.empty(s) for k, s in W.param_shapes(ARCH).items()}).items()}
    assert mapped == hf_shapes
    assert W.param_shapes(TINY, 64)["blocks.1.attn.relative_position_bias_table"] == (52, 2)
    with_head = W.param_shapes(ARCH, num_classes=10)
    assert sum(torch.Size(v).numel() for v in with_head.values()) == N_PARAMS + 7_690
    assert list(with_head)[-2:] == ["head.weight", "head.bias"] == list(W.head_keys(ARCH))
    for img in (0, 8, 100, 240):
        with pytest.raises(ValueError):
            W.param_shapes(ARCH, img)


def _old_layout(sd, img=224):
    """Older timm checkpoints carry the derived buffers as well."""
    out = dict(sd)
    T = (img // 16) ** 2 + 1
    for i in (0, 1):
        out[f"blocks.{i}.attn.relative_position_index"] = torch.zeros(T, T, dtype=torch.long)
        out[f"blocks.{i}.attn.k_bias"] = torch.zeros(sd["blocks.0.attn.q_bias"].shape)
    return out


def test_factories_accept_beit(tmp_path):
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.encoders import AutoEncoderFactory, BeitEncoder, make_encoder  # noqa: F401
    for arch in (ARCH, ARCH2):
        enc = AutoEncoderFactory("timm", arch)()           # NotImplementedError before libeffocr_beit.so existed
        assert enc.arch == arch
        assert sum(p.numel() for _, p in enc.named_parameters()) == N_PARAMS
    sd = W.init_state_dict(ARCH, seed=4, num_classes=7)
    W.save_checkpoint(_old_layout(sd), tmp_path / "clf.pth")
    clf = AutoClassifierFactory("timm", ARCH, n_classes=7).load(str(tmp_path / "clf.pth"))
    got = clf.state_dict()
    assert sorted(got) == sorted("net." + k for k in sd) and all(torch.equal(got["net." + k], v) for k, v in sd.items())
    assert sum(p.numel() for _, p in clf.named_parameters()) == N_PARAMS + 7 * 768 + 7
    # names that raise today still raise
    for name in ("beit_large_patch16_224", "beit_base_patch16_384", "xcit_small_12_p8_224"):
        with pytest.raises(NotImplementedError):
            AutoEncoderFactory("timm", name)
    with pytest.raises(NotImplementedError):
        AutoEncoderFactory("hf", ARCH)


def test_loader_and_infer_arch():
    sd = W.init_state_dict(ARCH, seed=0, num_classes=10)
    for variant in (sd, _old_layout(sd)):
        for pref in ("", "net."):
            d = {pref + k: v for k, v in variant.items()}
            assert W.infer_arch(d) == ARCH                 # beitv2 has the same keys and shapes: the answer is the first name
            canon = W.strip_prefix(d)
            assert sorted(canon) == sorted(sd) and all(torch.equal(canon[k], sd[k]) for k in sd)
            assert W.infer_num_classes(d) == 10
            assert W.beit_img_size(d) == 224
    W.check_state_dict(ARCH, sd)
    W.check_state_dict(ARCH2, sd, num_classes=10)
    # img_size comes from the table length
    for img in (16, 64, 128):
        t = W.init_state_dict(TINY, seed=1, img_size=img)
        assert W.infer_arch(t) == TINY and W.beit_img_size(t) == img
    # BEiT, ViT and Swin checkpoints are told apart
    assert W.infer_arch(W.init_state_dict("vit_base_patch16_224", scale="timm")) == "vit_base_patch16_224"
    assert W.infer_arch(W.init_state_dict("vit_tiny_test", img_size=64)) == "vit_tiny_test"
    assert W.infer_arch(W.init_state_dict("swin_tiny_patch4_window7_224", scale="timm")) == "swin_tiny_patch4_window7_224"
    # a wrong table length, in every block or in one
    bad = dict(sd)
    for i in range(12):
        bad[f"blocks.{i}.attn.relative_position_bias_table"] = torch.zeros(731, 12)
    with pytest.raises(ValueError, match="731 rows"):
        W.infer_arch(bad)
    bad = dict(sd)
    bad["blocks.7.attn.relative_position_bias_table"] = torch.zeros(628, 12)
    with pytest.raises(ValueError, match="blocks.7.attn.relative_position_bias_table"):
        W.infer_arch(bad)
    with pytest.raises(ValueError, match="blocks.7.attn.relative_position_bias_table"):
        W.check_state_dict(ARCH, bad)
    missing = dict(sd)
    del missing["blocks.2.attn.v_bias"]
    with pytest.raises(ValueError, match="missing blocks.2.attn.v_bias"):
        W.check_state_dict(ARCH, missing)
    wide = {k: v for k, v in W.init_state_dict(TINY, seed=1, img_size=64).items() if not k.startswith("blocks.1.")}
    with pytest.raises(ValueError, match="unsupported BEiT"):
        W.infer_arch(wide)


def test_seeded_init_is_deterministic_and_nontrivial():
    a, b, c = (W.init_state_dict(ARCH, seed=s) for s in (9, 9, 10))
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["patch_embed.proj.weight"], c["patch_embed.proj.weight"])
    t = W.init_state_dict(ARCH, seed=9, scale="timm")
    for sd in (a, t):
        assert torch.all(sd["blocks.4.gamma_1"] == 0.1) and torch.all(sd["blocks.4.gamma_2"] == 0.1)
        assert sd["blocks.0.attn.relative_position_bias_table"].abs().min() > 0
        for k in ("blocks.0.attn.q_bias", "blocks.0.attn.v_bias", "blocks.5.attn.proj.bias", "blocks.5.mlp.fc1.bias", "patch_embed.proj.bias"):
            assert sd[k].abs().max() > 0, k
    assert abs(a["blocks.1.attn.relative_position_bias_table"].std().item() - 1.0) < 0.05
    assert 0.5 <= a["fc_norm.weight"].min() and a["fc_norm.weight"].max() <= 1.5 and a["blocks.3.norm2.weight"].std() > 0.1
    assert torch.all(t["fc_norm.weight"] == 1) and torch.all(t["blocks.3.norm1.bias"] == 0)
    assert abs(t["blocks.2.mlp.fc1.weight"].std().item() - 0.02) < 0.003
    h = W.init_state_dict(ARCH, seed=9, num_classes=5)
    assert all(torch.equal(h[k], a[k]) for k in a) and h["head.weight"].shape == (5, 768)


# -- libeffocr_beit.so ------------------------------------------------------------------------------------------------------------
def test_beit_library_exports_its_header_and_versions_agree():
    src = open(os.path.join(ROOT, "include", "effocr_beit.h")).read()
    declared = sorted(set(re.findall(r"\b(effocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert len(declared) == 17
    raw = ctypes.CDLL(_lib.BEIT_SO_PATH)
    for n in declared:
        assert hasattr(raw, n), f"{n} declared in effocr_beit.h but not exported"
    assert sorted(_lib.BEIT_EXPORTS) == declared
    v = int(re.search(r"#define\s+EFFOCR_BEIT_ABI_VERSION\s+(\d+)", src).group(1))
    assert _lib.beit_lib().effocr_beit_abi_version() == v == _lib.BEIT_ABI_VERSION == 1
    # it exports effocr_beit_* only: the dynamic symbol table holds no other defined function
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.BEIT_SO_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    defined = sorted(line.split()[-1] for line in nm.splitlines())
    assert defined == declared, defined
    for hidden in ("_ZN6effocr7gemm_ntEiiRKNS_8GemmArgsEP12ihipStream_t", "effocr_abi_version", "effocr_encoder_create", "effocr_swin_create"):
        assert not hasattr(raw, hidden), hidden
    _lib.lib()
    assert not set(declared) & set(_lib.EXPORTS)
    assert not hasattr(ctypes.CDLL(_lib.SO_PATH), "effocr_beit_create")


def test_product_library_still_refuses_beit(hip_lib):
    h = ctypes.c_void_p()
    for name in (ARCH, ARCH2):
        assert hip_lib.effocr_encoder_create(name.encode(), 224, 1, ctypes.byref(h)) == -2


def test_beit_handle_and_refusals():
    L = _lib.beit_lib()
    h = ctypes.c_void_p()
    for arch, img, D in ((ARCH, 224, 768), (ARCH2, 224, 768), (TINY, 64, 128), (TINY, 16, 128)):
        shapes = W.param_shapes(arch, img)
        for prec in (0, 1, 2):
            assert L.effocr_beit_create(arch.encode(), img, prec, ctypes.byref(h)) == 0
            try:
                assert L.effocr_beit_embed_dim(h) == D
                n = L.effocr_beit_num_params(h)
                names = [L.effocr_beit_param_name(h, i).decode() for i in range(n)]
                assert names == list(shapes)
                for i, k in enumerate(names):
                    assert L.effocr_beit_param_numel(h, i) == torch.Size(shapes[k]).numel()
                assert L.effocr_beit_param_name(h, n) is None and L.effocr_beit_param_numel(h, -1) == -1
                assert L.effocr_beit_weights_bytes(h) > 0
                ws1 = L.effocr_beit_workspace_bytes(h, 1)
                ws = L.effocr_beit_workspace_bytes(h, 4096)
                assert 0 < ws1 < ws < 1000 * (1 << 20)                    # sub-batches keep the workspace under 1 GB
                assert L.effocr_beit_workspace_bytes(h, 0) == 0
                assert L.effocr_beit_set_chunk(h, 5) == 0
                assert L.effocr_beit_workspace_bytes(h, 4096) == L.effocr_beit_workspace_bytes(h, 5) < ws
                assert L.effocr_beit_set_chunk(h, -1) == -1
                one = torch.zeros(1)
                assert L.effocr_beit_set_param(h, b"fc_norm.weight", _lib.ptr(one), 1) == -1
                assert f"expects {D}".encode() in L.effocr_beit_last_error()
                for absent in (b"head.weight", b"pos_embed", b"blocks.0.attn.qkv.bias", b"blocks.0.attn.k_bias"):
                    assert L.effocr_beit_set_param(h, absent, _lib.ptr(one), 1) == -1
                assert L.effocr_beit_set_param(h, None, _lib.ptr(one), 1) == -1
                # upload before every parameter is set, forward before upload
                p = ctypes.c_void_p(4096)                                  # never dereferenced: these calls are refused first
                assert L.effocr_beit_upload(h, p, L.effocr_beit_weights_bytes(h)) == -5
                assert L.effocr_beit_upload(h, p, 1) == -3
                assert L.effocr_beit_upload(h, None, 1 << 30) == -1
                assert L.effocr_beit_forward(h, p, 2, p, 0, p, 1 << 40, None) == -5
                assert L.effocr_beit_forward(h, p, -1, p, 0, p, 1 << 40, None) == -1
                assert L.effocr_beit_forward(h, None, 2, p, 0, p, 1 << 40, None) == -1
                assert L.effocr_beit_forward(h, p, 0, p, 0, p, 0, None) == 0
                assert L.effocr_beit_check_status(h, None, None) == -1
                assert L.effocr_beit_reset_status(h, None, None) == -1
            finally:
                L.effocr_beit_destroy(h)
    for size in (0, 8, 100, 240, 384, -16):
        assert L.effocr_beit_create(ARCH.encode(), size, 1, ctypes.byref(h)) == -1
        assert b"multiple of 16" in L.effocr_beit_last_error()
    for prec in (-1, 3):
        assert L.effocr_beit_create(ARCH.encode(), 224, prec, ctypes.byref(h)) == -1
    for name in (b"beit_large_patch16_224", b"beit_base_patch16_384", b"vit_base_patch16_224"):
        assert L.effocr_beit_create(name, 224, 1, ctypes.byref(h)) == -2
    assert L.effocr_beit_create(None, 224, 1, ctypes.byref(h)) == -1
    assert L.effocr_beit_create(ARCH.encode(), 224, 1, None) == -1
    assert L.effocr_beit_forward(None, None, 1, None, 0, None, 0, None) == -1
    assert L.effocr_beit_embed_dim(None) == 0 and L.effocr_beit_num_params(None) == 0
    p = ctypes.c_void_p(4096)
    assert L.effocr_beit_op_attn(None, p, 1, 2, 2, 1, p, None) == -1
    assert L.effocr_beit_op_attn(p, p, 0, 2, 2, 1, p, None) == -1
    for side in (0, 15):
        assert L.effocr_beit_op_attn(p, p, 1, side, 2, 1, p, None) == -2          # refused before any launch
