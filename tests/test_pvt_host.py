"""PVTv2 (pvt_v2_b0 ... pvt_v2_b5) without a GPU: the restatement tests/pvt_ref.py against transformers.PvtV2Model, the parameter table and
its counts, architecture inference and its refusals, checkpoint I/O, the classifier's head keys, and the C ABI of libeffocr_pvt.so."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from effocr_amd import _lib
from effocr_amd import weights as W
from tests import pvt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pvt_v2_b0", "pvt_v2_b1", "pvt_v2_b2", "pvt_v2_b3", "pvt_v2_b4", "pvt_v2_b5")
MINI32, MINI64 = "pvt_v2_mini32_test", "pvt_v2_mini64_test"
# learnable parameters without the head: b0 ... b3 and the miniatures as the issue states them (b0 ... b3 + 1000-class head = timm's
# published 3.67 / 14.01 / 25.36 / 45.24 M), b4 and b5 as transformers.PvtV2Model counts them (recorded here, re-checked below)
N_PARAMS = {"pvt_v2_b0": 3409760, "pvt_v2_b1": 13496000, "pvt_v2_b2": 24849856, "pvt_v2_b3": 44725696, "pvt_v2_b4": 62043072,
            "pvt_v2_b5": 81443008, MINI32: 789920, MINI64: 3704128}
EMBED = {"pvt_v2_b0": 256, MINI32: 128, MINI64: 256}


@pytest.mark.parametrize("arch", NAMES + (MINI32, MINI64))
def test_param_counts_against_table_and_transformers(arch):
    from transformers import PvtV2Model
    shapes = W.param_shapes(arch)
    n = sum(torch.Size(s).numel() for s in shapes.values())
    assert n == N_PARAMS[arch] == W.pvt_num_learnable(arch)
    with torch.device("meta"):
        m = PvtV2Model(R.hf_config(arch, 224))
    assert sum(p.numel() for p in m.parameters()) == n
    assert W.embed_dim(arch) == EMBED.get(arch, 512)
    assert W.pvt_num_learnable(arch, 1000) == n + 1000 * W.embed_dim(arch) + 1000
    # the restatement's own table agrees with the package's
    assert R.CFG[arch] == W.PVT_CFG[arch]


CASES = [(a, 32) for a in NAMES] + [(a, s) for a in ("pvt_v2_b0", MINI32, MINI64) for s in (64, 96)]


@pytest.mark.parametrize("arch,img", CASES)
def test_restatement_matches_transformers(arch, img):
    sd = W.init_state_dict(arch, seed=1, scale="trained")
    x = R.crops(2, img, seed=5)
    want = R.hf_forward(arch, sd, x)
    got = R.pvt_forward(arch, sd, x, dtype=torch.float32)
    assert got.shape == (2, W.embed_dim(arch))
    err = ((got - want).abs().max() / want.abs().max()).item()
    assert err < 1e-5, err
    if img == 64:
        assert img // 32 == 2                                # the last stage is (img / 32)^2 tokens: 1 at 32^2, 49 at 224^2
        for m in R.MISTAKES:                                 # every deliberately wrong network is a different function
            bad = R.pvt_forward(arch, sd, x, mistake=m, dtype=torch.float32)
            assert ((bad - want).abs().max() / want.abs().max()).item() > 1e-3, m


def test_key_list_and_dwconv_spelling():
    s = W.param_shapes("pvt_v2_b0")
    keys = list(s)
    assert keys[:4] == ["patch_embed.proj.weight", "patch_embed.proj.bias", "patch_embed.norm.weight", "patch_embed.norm.bias"]
    assert s["patch_embed.proj.weight"] == (32, 3, 7, 7) and s["stages.1.downsample.proj.weight"] == (64, 32, 3, 3)
    blk = [k[len("stages.0.blocks.0."):] for k in keys if k.startswith("stages.0.blocks.0.")]
    assert blk == [f"{m}.{leaf}" for m in ("norm1", "attn.q", "attn.kv", "attn.proj", "attn.sr", "attn.norm", "norm2", "mlp.fc1", "mlp.dwconv", "mlp.fc2")
                   for leaf in ("weight", "bias")]
    assert s["stages.0.blocks.0.attn.sr.weight"] == (32, 32, 8, 8) and s["stages.2.blocks.1.attn.sr.weight"] == (160, 160, 2, 2)
    assert s["stages.0.blocks.0.attn.kv.weight"] == (64, 32) and s["stages.0.blocks.0.mlp.dwconv.weight"] == (256, 1, 3, 3)
    assert not any(k.startswith("stages.3.blocks.0.attn.sr") or k.startswith("stages.3.blocks.0.attn.norm") for k in keys)
    assert "stages.0.downsample.proj.weight" not in s and keys[-2:] == ["stages.3.norm.weight", "stages.3.norm.bias"]
    assert W.head_keys("pvt_v2_b0") == ("head.weight", "head.bias")
    assert list(W.param_shapes("pvt_v2_b0", 224, 9))[-2:] == ["head.weight", "head.bias"]
    assert W.param_shapes("pvt_v2_b0", 224, 9)["head.weight"] == (9, 256)
    assert W.param_shapes("pvt_v2_b1", 64) == W.param_shapes("pvt_v2_b1", 224)       # a checkpoint does not fix the crop size
    # the original repository's spelling of the depthwise convolution is accepted
    sd = W.init_state_dict(MINI32, seed=2)
    old = {("net." + k).replace(".mlp.dwconv.", ".mlp.dwconv.dwconv."): v for k, v in sd.items()}
    back = W.strip_prefix(old)
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    assert W.infer_arch(old) == MINI32


@pytest.mark.parametrize("arch", NAMES + (MINI32, MINI64))
def test_infer_arch(arch):
    sd = W.init_state_dict(arch, seed=0, scale="timm")
    assert W.infer_arch(sd) == arch
    assert W.infer_arch({"net." + k: v for k, v in sd.items()}) == arch
    W.check_state_dict(arch, sd, 96)
    assert W.is_pvt(arch) and not W.is_vit(arch) and not W.is_levit(arch)


def test_refusals_list_the_supported_names():
    listed = ", ".join(NAMES)
    from effocr_amd.encoders import AutoEncoderFactory
    for name in ("pvt_v2_b2_li", "pvt_tiny", "pvt_v2_b6"):
        with pytest.raises(NotImplementedError, match="pvt_v2_b0, pvt_v2_b1") as ei:
            AutoEncoderFactory("timm", name)
        assert listed in str(ei.value)
    with pytest.raises(NotImplementedError):
        AutoEncoderFactory("timm", "xcit_small_12_p8_224")   # raised before this family existed, and still must
    with pytest.raises(NotImplementedError):
        AutoEncoderFactory("hf", "pvt_v2_b0")
    sd = W.init_state_dict("pvt_v2_b1", seed=0, scale="timm")

    def refused(mod, pattern):
        bad = dict(sd)
        mod(bad)
        with pytest.raises(ValueError, match=pattern) as ei:
            W.infer_arch(bad)
        assert listed in str(ei.value)
    refused(lambda d: d.update({"pos_embed": torch.zeros(1, 3136, 64)}), "position embeddings")              # PVT v1
    refused(lambda d: d.update({"stages.0.blocks.0.attn.pool.weight": torch.zeros(1)}), "pooled linear")   # pvt_v2_b2_li
    refused(lambda d: [d.pop(k) for k in list(d) if ".attn.sr." in k and k.startswith("stages.0.")], "no stage-0 spatial reduction")
    refused(lambda d: [d.pop(k) for k in list(d) if k.startswith("stages.2.blocks.1.")], "depths")          # a wrong depth
    refused(lambda d: d.update({"stages.1.blocks.0.attn.q.weight": torch.zeros(96, 96)}), "does not fit")   # a wrong width
    refused(lambda d: d.update({"patch_embed.proj.weight": torch.zeros(48, 3, 7, 7)}), "stem width 48")
    with pytest.raises(ValueError, match="missing stages.0.norm.weight"):
        W.check_state_dict("pvt_v2_b0", {k: v for k, v in W.init_state_dict("pvt_v2_b0").items() if k != "stages.0.norm.weight"})


def test_seeded_init_and_checkpoint_round_trip(tmp_path):
    a, b = W.init_state_dict(MINI64, seed=3), W.init_state_dict(MINI64, seed=3)
    assert list(a) == list(W.param_shapes(MINI64)) and all(torch.equal(a[k], b[k]) for k in a)
    c = W.init_state_dict(MINI64, seed=4)
    assert not torch.equal(a["stages.0.blocks.0.attn.q.weight"], c["stages.0.blocks.0.attn.q.weight"])
    assert all(v.abs().max() > 0 for v in a.values())       # "unit": no term is switched off
    t = W.init_state_dict(MINI64, seed=3, scale="timm")
    assert torch.equal(t["stages.1.norm.weight"], torch.ones(128)) and t["stages.1.blocks.0.mlp.fc1.bias"].abs().max() == 0
    tr = W.init_state_dict(MINI64, seed=3, scale="trained")
    assert tr["stages.0.blocks.0.mlp.fc2.weight"].std() < 0.5 * a["stages.0.blocks.0.mlp.fc2.weight"].std()
    with pytest.raises(ValueError):
        W.init_state_dict(MINI64, scale="big")
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.encoders import AutoEncoderFactory
    sd = W.init_state_dict(MINI32, seed=4, num_classes=7)
    assert sd["head.weight"].shape == (7, 128) and sd["head.bias"].shape == (7,)
    W.save_checkpoint(sd, tmp_path / "clf.pth")
    assert all(k.startswith("net.") for k in torch.load(tmp_path / "clf.pth", weights_only=True))
    clf = AutoClassifierFactory("timm", MINI32, n_classes=7, img_size=64).load(str(tmp_path / "clf.pth"))
    got = clf.state_dict()
    assert sorted(got) == sorted("net." + k for k in sd) and all(torch.equal(got["net." + k], v) for k, v in sd.items())
    enc = AutoEncoderFactory("timm", MINI32, img_size=64).load(str(tmp_path / "clf.pth"))
    assert sum(p.numel() for _, p in enc.named_parameters()) == N_PARAMS[MINI32]
    for arch in NAMES[:2]:
        e = AutoEncoderFactory("timm", arch)()              # NotImplementedError before libeffocr_pvt.so existed
        assert e.arch == arch and sum(p.numel() for _, p in e.named_parameters()) == N_PARAMS[arch]
    if not torch.cuda.is_available():                        # no GPU: a loud failure, never NotImplementedError or a fallback
        from effocr_amd import EffOCRHipError
        from effocr_amd.encoders import PvtEncoder, make_encoder
        from effocr_amd.recognizer_engine import EffRecognizer
        with pytest.raises(EffOCRHipError):
            enc.to("cuda")(torch.zeros(1, 3, 64, 64))
        with pytest.raises(EffOCRHipError):
            make_encoder(MINI32, sd, img_size=64)
        with pytest.raises(EffOCRHipError):
            PvtEncoder(MINI32, sd, img_size=64)
        with pytest.raises(EffOCRHipError):
            EffRecognizer(str(tmp_path / "clf.pth"), img_size=64)


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_attention_emulation_is_the_reference_up_to_rounding(prec):
    g = torch.Generator().manual_seed(7)
    B, N, M, heads, hd = 2, 50, 9, 2, 32
    q = R.rnd(torch.randn(B * N, heads * hd, generator=g), prec).double()
    kv = R.rnd(torch.randn(B * M, 2 * heads * hd, generator=g), prec).double()
    ref = R.attention_ref(q, kv, B, N, M, heads, hd)
    emu = R.attention_emulated(q, kv, B, N, M, heads, hd, prec)
    e = ((emu - ref).abs().max() / ref.abs().max()).item()
    ulp = 2.0 ** -8 if prec == "bf16" else 2.0 ** -11
    assert 0 < e < 4 * ulp, e
    # by hand for one (crop, head, query)
    s = (q[N + 3, 32:64] @ kv[M:2 * M, 32:64].T) / 32 ** 0.5
    want = s.softmax(0) @ kv[M:2 * M, 64 + 32:64 + 64]
    assert torch.allclose(ref[N + 3, 32:64], want, rtol=1e-12, atol=1e-12)


# -- libeffocr_pvt.so ---------------------------------------------------------------------------------------------------------------
def test_pvt_library_exports_its_header_and_versions_agree():
    src = open(os.path.join(ROOT, "include", "effocr_pvt.h")).read()
    declared = sorted(set(re.findall(r"\b(effocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert len(declared) == 20
    raw = ctypes.CDLL(_lib.PVT_SO_PATH)
    for n in declared:
        assert hasattr(raw, n), f"{n} declared in effocr_pvt.h but not exported"
    assert sorted(_lib.PVT_EXPORTS) == declared
    v = int(re.search(r"#define\s+EFFOCR_PVT_ABI_VERSION\s+(\d+)", src).group(1))
    assert _lib.pvt_lib().effocr_pvt_abi_version() == v == _lib.PVT_ABI_VERSION == 1
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.PVT_SO_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in nm.splitlines()) == declared
    _lib.lib()
    assert not set(declared) & set(_lib.EXPORTS)
    assert not hasattr(ctypes.CDLL(_lib.SO_PATH), "effocr_pvt_create")
    # the query tile the GPU tests walk around is stated in the kernel header
    hpp = open(os.path.join(ROOT, "effocr_amd", "csrc", "pvt.hpp")).read()
    assert int(re.search(r"constexpr int PVT_QBLK = (\d+);", hpp).group(1)) >= 1
    assert int(re.search(r"constexpr int PVT_MAX_KEYS = (\d+);", hpp).group(1)) == 49


def test_pvt_handle_and_refusals(hip_lib):
    L = _lib.pvt_lib()
    h = ctypes.c_void_p()
    for arch, img in tuple((a, 224) for a in NAMES) + ((MINI32, 32), (MINI64, 96)):
        shapes = W.param_shapes(arch, img)
        for prec in (0, 1, 2):
            assert L.effocr_pvt_create(arch.encode(), img, prec, ctypes.byref(h)) == 0
            try:
                assert L.effocr_pvt_embed_dim(h) == W.embed_dim(arch)
                n = L.effocr_pvt_num_params(h)
                names = [L.effocr_pvt_param_name(h, i).decode() for i in range(n)]
                assert names == list(shapes)
                for i, k in enumerate(names):
                    assert L.effocr_pvt_param_numel(h, i) == torch.Size(shapes[k]).numel()
                assert L.effocr_pvt_param_name(h, n) is None and L.effocr_pvt_param_numel(h, -1) == -1
                assert L.effocr_pvt_weights_bytes(h) > 0
                ws1 = L.effocr_pvt_workspace_bytes(h, 1)
                ws = L.effocr_pvt_workspace_bytes(h, 4096)
                assert 0 < ws1 < ws < 1000 * (1 << 20)                     # sub-batches keep the workspace under 1 GB
                assert L.effocr_pvt_workspace_bytes(h, 0) == 0
                assert L.effocr_pvt_set_chunk(h, 5) == 0
                assert L.effocr_pvt_workspace_bytes(h, 4096) == L.effocr_pvt_workspace_bytes(h, 5) < ws
                assert L.effocr_pvt_set_chunk(h, -1) == -1
                one = torch.zeros(1)
                assert L.effocr_pvt_set_param(h, b"stages.3.norm.weight", _lib.ptr(one), 1) == -1
                assert f"expects {W.embed_dim(arch)}".encode() in L.effocr_pvt_last_error()
                for absent in (b"head.weight", b"pos_embed", b"stages.3.blocks.0.attn.sr.weight", b"stages.0.blocks.0.attn.pool.weight"):
                    assert L.effocr_pvt_set_param(h, absent, _lib.ptr(one), 1) == -1
                p = ctypes.c_void_p(4096)                                   # never dereferenced: these calls are refused first
                assert L.effocr_pvt_upload(h, p, L.effocr_pvt_weights_bytes(h)) == -5
                assert L.effocr_pvt_upload(h, p, 1) == -3
                assert L.effocr_pvt_forward(h, p, 2, p, 0, p, 1 << 40, None) == -5
                assert L.effocr_pvt_forward(h, p, -1, p, 0, p, 1 << 40, None) == -1
                assert L.effocr_pvt_forward(h, p, 0, p, 0, p, 0, None) == 0
                assert L.effocr_pvt_check_status(h, None, None) == -1
                assert L.effocr_pvt_reset_status(h, None, None) == -1
            finally:
                L.effocr_pvt_destroy(h)
    for size in (0, 16, 48, 256, -32, 100):
        assert L.effocr_pvt_create(b"pvt_v2_b0", size, 1, ctypes.byref(h)) == -1
        assert b"multiple of 32" in L.effocr_pvt_last_error()
    for prec in (-1, 3):
        assert L.effocr_pvt_create(b"pvt_v2_b0", 224, prec, ctypes.byref(h)) == -1
    for name in (b"pvt_v2_b2_li", b"pvt_tiny", b"xcit_small_12_p8_224", b"levit_128", b"pvt_v2_b6"):
        assert L.effocr_pvt_create(name, 224, 1, ctypes.byref(h)) == -2
        assert b"pvt_v2_b0, pvt_v2_b1, pvt_v2_b2, pvt_v2_b3, pvt_v2_b4, pvt_v2_b5" in L.effocr_pvt_last_error()
    assert L.effocr_pvt_create(None, 224, 1, ctypes.byref(h)) == -1
    assert L.effocr_pvt_create(b"pvt_v2_b0", 224, 1, None) == -1
    assert L.effocr_pvt_embed_dim(None) == 0 and L.effocr_pvt_num_params(None) == 0
    # the op entry points refuse bad shapes before any launch
    p = ctypes.c_void_p(4096)
    assert L.effocr_pvt_op_attention(None, p, 1, 4, 4, 1, 32, 1, p, None) == -1
    assert L.effocr_pvt_op_attention(p, p, 0, 4, 4, 1, 32, 1, p, None) == -1
    for m, hd in ((0, 32), (50, 32), (4, 16), (4, 48)):
        assert L.effocr_pvt_op_attention(p, p, 1, 4, m, 1, hd, 1, p, None) == -2
    assert L.effocr_pvt_op_dwconv_gelu(p, 1, 2, 2, 6, p, p, 1, p, None) == -2
    assert L.effocr_pvt_op_stem(p, 1, 30, 32, p, p, p, p, 1, p, None) == -2
    assert L.effocr_pvt_op_conv_ln(p, 1, 8, 12, 32, 3, 2, 1, p, p, p, p, 1, p, None) == -2
    assert L.effocr_pvt_op_conv_ln(p, 1, 8, 32, 48, 3, 2, 1, p, p, p, p, 1, p, None) == -2
    # the product library still refuses the family
    for name in NAMES:
        assert hip_lib.effocr_encoder_create(name.encode(), 224, 1, ctypes.byref(h)) == -2
