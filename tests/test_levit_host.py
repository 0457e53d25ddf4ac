"""LeViT without a GPU: the parameter tables against timm's published counts, the CPU restatement (tests/levit_ref.py) against an independent
implementation (transformers.LevitModel), the attention references, the checkpoint loader, the two-head classifier fold, the factories and
libeffocr_levit.so's C ABI (exports, version, handle, messages, refusals)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from effocr_amd import _lib
from effocr_amd import weights as W
from tests.levit_ref import (KEY_TILE, attention_emulated, attention_ref, bias_index, header_grids, hf_config, hf_state_dict, levit_forward,
                             levit_logits, sub)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY, TINY32 = "levit_tiny_test", "levit_tiny32_test"
# sum(p.numel()) of transformers.LevitModel built with these configs (learnable parameters, no running statistics) / the same plus timm's two
# 1000-class BatchNorm1d + Linear heads: timm's published 7.8 / 9.2 / 10.9 / 18.9 / 39.1 M
N_PARAMS = {"levit_128s": (7005522, 7777058), "levit_128": (8442400, 9213936), "levit_192": (10175533, 10947069),
            "levit_256": (17865828, 18893876), "levit_384": (37587764, 39128836)}
EMBED = {"levit_128s": 384, "levit_128": 384, "levit_192": 384, "levit_256": 512, "levit_384": 768, TINY: 128, TINY32: 256}


def test_parameter_counts_match_timm():
    assert tuple(N_PARAMS) == W.LEVIT_SUPPORTED
    for arch, (bare, headed) in N_PARAMS.items():
        assert W.levit_num_learnable(arch) == bare
        assert W.levit_num_learnable(arch, num_classes=1000) == headed
        assert round(headed / 1e6, 1) == {"levit_128s": 7.8, "levit_128": 9.2, "levit_192": 10.9, "levit_256": 18.9, "levit_384": 39.1}[arch]
        assert W.embed_dim(arch) == EMBED[arch] and W.is_levit(arch) and not W.is_vit(arch) and W._family(arch) == "levit"


def test_parameter_count_matches_transformers():
    from transformers import LevitModel
    for arch in ("levit_128s", "levit_192"):
        m = LevitModel(hf_config(arch, 224))
        assert sum(p.numel() for p in m.parameters()) == N_PARAMS[arch][0]


@pytest.mark.parametrize("arch,img", [(TINY, 32), (TINY, 48), (TINY, 64), (TINY32, 48), (TINY32, 64), (TINY, 224), ("levit_128s", 224)])
def test_reference_matches_transformers(arch, img):
    """levit_ref against transformers.LevitModel.pooler_output on the same seeded weights, fp32, bound 1e-5 (relative L2 per row).  The
    token grids are 2 -> 1 -> 1, 3 -> 2 -> 1, 4 -> 2 -> 1 and 14 -> 7 -> 4.  LevitModel runs in float32 only (in float64 its cached biases
    stay float32) and caches the gathered biases at its first eval-mode forward: the weights are loaded before that."""
    from transformers import LevitModel
    sd = W.init_state_dict(arch, seed=11, img_size=img)
    m = LevitModel(hf_config(arch, img))
    res = m.load_state_dict(hf_state_dict(arch, sd), strict=False)
    assert not res.unexpected_keys and all(k.endswith("num_batches_tracked") for k in res.missing_keys)
    m.eval()
    x = torch.randn(3, 3, img, img, generator=torch.Generator().manual_seed(img))
    with torch.no_grad():
        want = m(x).pooler_output
    got = levit_forward(arch, sd, x)
    assert got.shape == (3, EMBED[arch]) and got.dtype == torch.float32
    rel = ((got - want).norm(dim=1) / want.norm(dim=1)).max().item()
    assert rel <= 1e-5, rel
    # and float32 against float64 of the same restatement
    ref64 = levit_forward(arch, sd, x.double())
    assert ((got.double() - ref64).norm(dim=1) / ref64.norm(dim=1)).max().item() <= 1e-5
    assert (ref64[0] - ref64[1]).norm() / ref64[0].norm() > 0.01                   # the embedding depends on the crop


def test_bias_index_is_timm_s_enumeration():
    """timm enumerates the offsets (|dy|, |dx|) in the order the pairs (query (0, 0), key in row-major order) first produce them: index
    |dy| R + |dx|; the strided form measures from the query's position on the key grid."""
    import itertools
    for R, stride in ((1, 1), (3, 1), (4, 1), (14, 1), (2, 2), (3, 2), (7, 2), (14, 2)):
        Rq = sub(R) if stride == 2 else R
        pts, qpts = list(itertools.product(range(R), range(R))), list(itertools.product(range(Rq), range(Rq)))
        offsets, idxs = {}, []
        for p1 in qpts:
            for p2 in pts:
                off = (abs(p1[0] * stride - p2[0]), abs(p1[1] * stride - p2[1]))
                offsets.setdefault(off, len(offsets))
                idxs.append(offsets[off])
        assert len(offsets) == R * R
        assert torch.equal(torch.tensor(idxs).view(Rq * Rq, R * R), bias_index(R, stride))
    assert [sub(r) for r in (14, 7, 4, 3, 2, 1)] == [7, 4, 2, 2, 1, 1]


def test_operator_test_grids_surround_the_tile_sizes():
    """The grids tests/test_gpu_levit_ops.py walks (LEVIT_TEST_GRIDS of csrc/levit.hpp) give key counts one below, at and above the 32-key
    MFMA tile and the 4-key tail, and every down-sampling a supported crop size produces."""
    grids, ktile, ktail = header_grids()
    keys = [r * r for r in grids]
    assert keys == [1, 4, 9, 16, 36, 49, 64, 196] and (ktile, ktail) == (32, 4) and ktile == KEY_TILE
    assert any(k < ktile for k in keys) and any(ktile < k < 2 * ktile for k in keys) and 2 * ktile in keys       # 16 | 36, 49 | 64
    assert ktail in keys and ktail - 3 in keys and any(k % ktile == ktail for k in keys if k > ktile)           # 4 | 1 | 36, 196
    assert {(14, 7), (7, 4), (3, 2), (2, 1)} <= {(r, sub(r)) for r in grids}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_attention_emulation_is_the_reference_up_to_rounding(dtype):
    g = torch.Generator().manual_seed(3)
    R = 14
    q, k = (torch.randn(2, 2, 49, 16, generator=g).to(dtype).double(), torch.randn(2, 2, 196, 16, generator=g).to(dtype).double())
    v, tb = torch.randn(2, 2, 196, 64, generator=g).to(dtype).double(), torch.randn(2, 196, generator=g)
    ref = attention_ref(q, k, v, tb.double(), R, 2)
    exact = attention_emulated(q, k, v, tb, R, 2, dtype=torch.float64)
    assert ((exact - ref).abs().max() / ref.abs().max()).item() < 1e-13
    e = ((attention_emulated(q, k, v, tb, R, 2, dtype=dtype) - ref).abs().max() / ref.abs().max()).item()
    half_ulp = 2.0 ** -12 if dtype == torch.float16 else 2.0 ** -9
    assert 0.1 * half_ulp < e < 8 * half_ulp, e


def test_infer_arch_img_size_and_round_trip(tmp_path):
    for arch, img in ((TINY, 32), (TINY32, 64), ("levit_128s", 224), ("levit_128", 160), ("levit_192", 224), ("levit_256", 96)):
        sd = W.init_state_dict(arch, seed=1, img_size=img, scale="timm")
        assert list(sd) == list(W.param_shapes(arch, img))
        assert W.infer_arch(sd) == arch and W.levit_img_size(sd) == img
        W.check_state_dict(arch, sd, img)
    sd = W.init_state_dict(TINY, seed=2, img_size=48)
    path = tmp_path / "enc_best.pth"
    W.save_checkpoint(sd, path)
    raw = torch.load(path, map_location="cpu", weights_only=True)
    assert all(k.startswith("net.") for k in raw)
    # the derived buffers and BatchNorm counters a real timm checkpoint carries are ignored
    raw["net.stages.0.blocks.0.attn.attention_bias_idxs"] = torch.zeros(9, 9, dtype=torch.long)
    raw["net.stem.conv1.bn.num_batches_tracked"] = torch.tensor(5)
    torch.save(raw, path)
    back = W.load_checkpoint(path)
    assert W.infer_arch(back) == TINY and W.levit_img_size(back) == 48
    W.check_state_dict(TINY, back, 48)
    assert all(torch.equal(back[k], v) for k, v in sd.items())
    with pytest.raises(ValueError, match="attention_biases"):      # a 48^2 checkpoint asked to run at 64^2
        W.check_state_dict(TINY, sd, 64)
    with pytest.raises(ValueError, match="multiple of 16"):
        W.param_shapes(TINY, 40)
    with pytest.raises(ValueError, match="multiple of 16"):
        W.param_shapes(TINY, 16)


def test_unsupported_levits_are_refused_by_name_and_by_checkpoint():
    from effocr_amd.encoders import AutoEncoderFactory
    for name in ("levit_conv_128s", "levit_conv_256", "levit_384_s8", "levit_512", "levit_512d", "levit_conv_512_s8"):
        for call in (W.embed_dim, W.param_shapes, W._family, lambda n: AutoEncoderFactory("timm", n)):
            with pytest.raises(NotImplementedError, match="levit_128s, levit_128, levit_192, levit_256, levit_384"):
                call(name)
    sd = W.init_state_dict(TINY, seed=0, img_size=32, scale="timm")
    conv = dict(sd)
    conv["stages.0.blocks.0.attn.qkv.linear.weight"] = sd["stages.0.blocks.0.attn.qkv.linear.weight"][:, :, None, None]
    with pytest.raises(ValueError, match="levit_conv.*levit_128s, levit_128"):
        W.infer_arch(conv)
    with pytest.raises(ValueError, match="timm < 0.9.*levit_128s"):
        W.infer_arch({"patch_embed.0.c.weight": torch.zeros(16, 3, 3, 3), "blocks.0.m.qkv.c.weight": torch.zeros(256, 128)})
    wide = {k: (torch.zeros(512, 256, 3, 3) if k == "stem.conv4.linear.weight" else v) for k, v in sd.items()}
    with pytest.raises(ValueError, match="stem width 512.*supported"):
        W.infer_arch(wide)
    with pytest.raises(ValueError, match="R\\^2"):
        W.levit_img_size({"stages.0.blocks.0.attn.attention_biases": torch.zeros(4, 12)})


def test_seeded_init_is_deterministic_and_switches_nothing_off():
    a, b, c = (W.init_state_dict(TINY, seed=s, img_size=64) for s in (9, 9, 10))
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["stem.conv1.linear.weight"], c["stem.conv1.linear.weight"])
    for k, v in a.items():
        if k.endswith("attention_biases"):
            assert v.abs().max() > 0 and (v.numel() < 32 or 0.5 < v.std() < 1.5), k
        elif k.endswith(("bn.weight", "running_var")):
            assert v.min() >= 0.2 and v.max() <= 1.5, k
        elif k.endswith(("bn.bias", "running_mean")):
            assert v.abs().max() > 0, k
    t = W.init_state_dict(TINY, seed=9, img_size=64, scale="timm")
    assert torch.all(t["stages.0.blocks.0.attn.attention_biases"] == 0) and torch.all(t["stages.1.blocks.0.mlp.ln2.bn.weight"] == 0)
    assert torch.all(t["stages.1.blocks.0.attn.proj.ln.bn.weight"] == 0) and torch.all(t["stages.1.downsample.attn_downsample.proj.ln.bn.weight"] == 1)
    with pytest.raises(ValueError):
        W.init_state_dict(TINY, scale="huge")
    h = W.init_state_dict(TINY, seed=9, img_size=64, num_classes=5)
    assert all(torch.equal(h[k], a[k]) for k in a) and h["head_dist.linear.weight"].shape == (5, 128)
    assert W.infer_num_classes(h) == 5 and W.infer_num_classes(a) == 0


def test_two_head_fold_equals_the_unfolded_heads():
    """timm's Levit classifier averages two BatchNorm1d + Linear heads: folded on the host in float64 into one [N, D] weight and [N] bias."""
    sd = W.init_state_dict(TINY32, seed=4, img_size=32, num_classes=7)
    assert [k for k in sd if k.startswith("head")] == [f"{h}.{k}" for h in ("head", "head_dist") for k in
                                                       ("bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "linear.weight", "linear.bias")]
    w, b = W.levit_fold_heads(sd)
    assert w.shape == (7, 256) and b.shape == (7,) and w.dtype == b.dtype == torch.float32
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(1)).double()
    emb = levit_forward(TINY32, sd, x)
    want = levit_logits(TINY32, sd, x)
    got = emb @ w.double().T + b.double()
    assert ((got - want).abs().max() / want.abs().max()).item() < 1e-6          # the fold is float64; w and b are rounded to float32 once
    one = torch.nn.functional.linear(emb, sd["head.linear.weight"].double(), sd["head.linear.bias"].double())
    assert ((one - want).abs().max() / want.abs().max()).item() > 0.05          # neither head alone, nor a head without its BatchNorm


# -- libeffocr_levit.so -------------------------------------------------------------------------------------------------------------
def test_levit_library_exports_its_header_and_versions_agree():
    src = open(os.path.join(ROOT, "include", "effocr_levit.h")).read()
    declared = sorted(set(re.findall(r"\b(effocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert len(declared) == 18
    raw = ctypes.CDLL(_lib.LEVIT_SO_PATH)
    for n in declared:
        assert hasattr(raw, n), f"{n} declared in effocr_levit.h but not exported"
    assert sorted(_lib.LEVIT_EXPORTS) == declared
    v = int(re.search(r"#define\s+EFFOCR_LEVIT_ABI_VERSION\s+(\d+)", src).group(1))
    assert _lib.levit_lib().effocr_levit_abi_version() == v == _lib.LEVIT_ABI_VERSION == 1
    # it exports effocr_levit_* only: the dynamic symbol table holds no other defined symbol
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LEVIT_SO_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    defined = sorted(line.split()[-1] for line in nm.splitlines())
    assert defined == declared, defined
    for hidden in ("_ZN6effocr7gemm_ntEiiRKNS_8GemmArgsEP12ihipStream_t", "effocr_abi_version", "effocr_encoder_create", "effocr_vit8_create"):
        assert not hasattr(raw, hidden), hidden
    _lib.lib()
    assert not set(declared) & set(_lib.EXPORTS)
    assert not hasattr(ctypes.CDLL(_lib.SO_PATH), "effocr_levit_create")


def test_product_library_still_refuses_levit(hip_lib):
    h = ctypes.c_void_p()
    for name in ("levit_128s", "levit_384", TINY):
        assert hip_lib.effocr_encoder_create(name.encode(), 224, 1, ctypes.byref(h)) == -2


def test_levit_handle_messages_and_refusals():
    L = _lib.levit_lib()
    h = ctypes.c_void_p()
    for arch, img in (("levit_128s", 224), ("levit_128", 224), ("levit_192", 224), ("levit_256", 224), ("levit_384", 224), (TINY, 32),
                      (TINY32, 48), ("levit_192", 112)):
        shapes = W.param_shapes(arch, img)
        for prec in (0, 1, 2):
            assert L.effocr_levit_create(arch.encode(), img, prec, ctypes.byref(h)) == 0
            try:
                assert L.effocr_levit_embed_dim(h) == EMBED[arch]
                n = L.effocr_levit_num_params(h)
                names = [L.effocr_levit_param_name(h, i).decode() for i in range(n)]
                assert names == list(shapes)
                for i, k in enumerate(names):
                    assert L.effocr_levit_param_numel(h, i) == torch.Size(shapes[k]).numel()
                assert L.effocr_levit_param_name(h, n) is None and L.effocr_levit_param_numel(h, -1) == -1
                assert L.effocr_levit_weights_bytes(h) > 0
                ws1 = L.effocr_levit_workspace_bytes(h, 1)
                ws = L.effocr_levit_workspace_bytes(h, 4096)
                assert 0 < ws1 < ws < 1000 * (1 << 20)                    # sub-batches keep the workspace under 1 GB
                assert L.effocr_levit_workspace_bytes(h, 0) == 0
                assert L.effocr_levit_set_chunk(h, 5) == 0
                assert L.effocr_levit_workspace_bytes(h, 4096) == L.effocr_levit_workspace_bytes(h, 5) < ws
                assert L.effocr_levit_set_chunk(h, -1) == -1
                assert L.effocr_levit_last_error() == b"levit_set_chunk: bad argument"
                one = torch.zeros(1)
                assert L.effocr_levit_set_param(h, b"stem.conv1.bn.weight", _lib.ptr(one), 1) == -1
                assert f"levit_set_param: 'stem.conv1.bn.weight' expects {shapes['stem.conv1.bn.weight'][0]} elements, got 1".encode() == L.effocr_levit_last_error()
                for absent in (b"head.linear.weight", b"head_dist.bn.weight", b"stages.0.blocks.0.attn.attention_bias_idxs", b"stages.0.downsample.mlp.ln1.linear.weight"):
                    assert L.effocr_levit_set_param(h, absent, _lib.ptr(one), 1) == -1
                    assert L.effocr_levit_last_error() == b"levit_set_param: unknown parameter '" + absent + b"'"
                assert L.effocr_levit_set_param(h, None, _lib.ptr(one), 1) == -1
                # upload before every parameter is set, forward before upload
                p = ctypes.c_void_p(4096)                                  # never dereferenced: these calls are refused first
                assert L.effocr_levit_upload(h, p, L.effocr_levit_weights_bytes(h)) == -5
                assert L.effocr_levit_last_error() == b"levit_upload: parameter 'stem.conv1.linear.weight' was never set"
                assert L.effocr_levit_upload(h, p, 1) == -3
                assert L.effocr_levit_upload(h, None, 1 << 30) == -1
                assert L.effocr_levit_forward(h, p, 2, p, 0, p, 1 << 40, None) == -5
                assert L.effocr_levit_last_error() == b"levit_forward: weights were not uploaded"
                assert L.effocr_levit_forward(h, p, -1, p, 0, p, 1 << 40, None) == -1
                assert L.effocr_levit_forward(h, None, 2, p, 0, p, 1 << 40, None) == -1
                assert L.effocr_levit_forward(h, p, 0, p, 0, p, 0, None) == 0
                assert L.effocr_levit_check_status(h, None, None) == -1
                assert L.effocr_levit_reset_status(h, None, None) == -1
            finally:
                L.effocr_levit_destroy(h)
    for size in (0, 16, 40, 100, 240, 384, -16):
        assert L.effocr_levit_create(b"levit_128s", size, 1, ctypes.byref(h)) == -1
        assert L.effocr_levit_last_error() == b"levit_create: img_size must be a multiple of 16 from 32 to 224"
    for prec in (-1, 3):
        assert L.effocr_levit_create(b"levit_128s", 224, prec, ctypes.byref(h)) == -1
    for name in (b"levit_conv_128s", b"levit_384_s8", b"levit_512", b"vit_small_patch16_224", b"nope"):
        assert L.effocr_levit_create(name, 224, 1, ctypes.byref(h)) == -2
        assert L.effocr_levit_last_error() == (b"levit_create: unsupported architecture '" + name +
                                               b"' (supported: levit_128s, levit_128, levit_192, levit_256, levit_384)")
    assert L.effocr_levit_create(None, 224, 1, ctypes.byref(h)) == -1
    assert L.effocr_levit_create(b"levit_128s", 224, 1, None) == -1
    assert L.effocr_levit_forward(None, None, 1, None, 0, None, 0, None) == -1
    assert L.effocr_levit_embed_dim(None) == 0 and L.effocr_levit_num_params(None) == 0
    p = ctypes.c_void_p(4096)
    assert L.effocr_levit_op_attention(None, 64, 64, 0, p, 64, 64, 16, 32, p, 1, 2, 1, 1, 16, 32, 0, 1, p, None) == -1
    assert L.effocr_levit_op_attention(p, 64, 64, 0, p, 64, 64, 16, 32, p, 0, 2, 1, 1, 16, 32, 0, 1, p, None) == -1
    assert L.effocr_levit_op_attention(p, 64, 64, 0, p, 64, 64, 16, 32, p, 1, 15, 1, 1, 16, 32, 0, 1, p, None) == -2     # refused before any launch
    assert L.effocr_levit_op_stem_conv(p, 1, 1, 8, 3, p, p, 16, 1, 1, None, 16, 0, None) == -1
    assert L.effocr_levit_op_stem_conv(p, 1, 1, 300, 3, p, p, 16, 1, 1, p, 16, 0, None) == -1


def test_factories_accept_levit(tmp_path):
    from effocr_amd import EffOCRHipError
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.encoders import AutoEncoderFactory, LevitEncoder, make_encoder
    for arch in ("levit_128s", "levit_192"):
        enc = AutoEncoderFactory("timm", arch)()           # NotImplementedError before libeffocr_levit.so existed
        assert enc.arch == arch
        assert sum(p.numel() for _, p in enc.named_parameters()) == N_PARAMS[arch][0]
    sd = W.init_state_dict(TINY, seed=4, img_size=64, num_classes=7)
    W.save_checkpoint(sd, tmp_path / "clf.pth")
    clf = AutoClassifierFactory("timm", TINY, n_classes=7, img_size=64).load(str(tmp_path / "clf.pth"))
    got = clf.state_dict()
    assert sorted(got) == sorted("net." + k for k in sd) and all(torch.equal(got["net." + k], v) for k, v in sd.items())
    assert sum(p.numel() for p in clf.parameters()) == W.levit_num_learnable(TINY, 64, 7)
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
            LevitEncoder("levit_128s", W.init_state_dict("levit_128s", scale="timm"))
        with pytest.raises(EffOCRHipError):
            EffRecognizer(str(tmp_path / "clf.pth"))
