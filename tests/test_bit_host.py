"""BiT ResNetV2 (resnetv2_50x1_bitm / resnetv2_101x1_bitm) without a GPU: the restatement of tests/bit_ref.py against transformers.BitModel,
the parameter table, checkpoint handling and the factories, the refusals, libeffocr_bit.so's C ABI without a device, and the operator
bounds of tests/bit_ref.py (they accept the kernels' contract emulated on the CPU and reject every mutant)."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

from effocr_amd import _lib
from effocr_amd import weights as W
from tests import bit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCHS = ["resnetv2_50x1_bitm", "resnetv2_101x1_bitm"]
ALIAS = {"resnetv2_50x1_bitm": "resnetv2_50x1_bit", "resnetv2_101x1_bitm": "resnetv2_101x1_bit"}
COUNTS = {"resnetv2_50x1_bitm": 23500352, "resnetv2_101x1_bitm": 42492480}
COUNTS_1000 = {"resnetv2_50x1_bitm": 25549352, "resnetv2_101x1_bitm": 44541480}       # timm's published 25.55 M / 44.54 M


def _hf(arch):
    from transformers import BitConfig, BitModel
    cfg = BitConfig(num_channels=3, embedding_size=64, hidden_sizes=[256, 512, 1024, 2048], depths=list(W.BIT_CFG[arch]),
                    layer_type="preactivation", hidden_act="relu", global_padding=None, num_groups=32, drop_path_rate=0.0,
                    embedding_dynamic_padding=False, output_stride=32, width_factor=1)
    return BitModel(cfg).eval()


@pytest.mark.parametrize("arch", ARCHS)
def test_restatement_equals_transformers_bitmodel(arch):
    m = _hf(arch)
    sd = W.init_state_dict(arch, seed=3)
    hf_sd = m.state_dict()
    mapped = {R.hf_key(k): v for k, v in sd.items()}
    assert sorted(mapped) == sorted(hf_sd)                                   # a bijection on the parameters
    assert all(tuple(mapped[k].shape) == tuple(hf_sd[k].shape) for k in mapped)
    assert sum(p.numel() for p in m.parameters()) == COUNTS[arch]
    m.load_state_dict(mapped)
    x = R.crops(2, 5, 64)
    with torch.no_grad():
        want = m(x).pooler_output.flatten(1)
    got = R.bit_forward(arch, sd, x)                                         # float32, as the module
    err = ((got - want).abs().max() / want.abs().max()).item()
    print(f"{arch}: restatement vs transformers.BitModel in float32: {err:.2e}")
    assert err <= 1e-5
    err64 = ((R.bit_forward(arch, sd, x.double()).float() - want).abs().max() / want.abs().max()).item()
    assert err64 <= 1e-5


@pytest.mark.parametrize("arch", ARCHS)
def test_parameter_table_and_counts(arch):
    shapes = W.param_shapes(arch)
    assert sum(math.prod(s) for s in shapes.values()) == COUNTS[arch]
    assert sum(math.prod(s) for s in W.param_shapes(arch, num_classes=1000).values()) == COUNTS_1000[arch]
    assert W.param_shapes(ALIAS[arch]) == shapes
    for name in (arch, ALIAS[arch]):
        assert W.embed_dim(name) == 2048 and W.is_bit(name) and W._family(name) == "bit"
        assert W.head_keys(name) == ("head.fc.weight", "head.fc.bias")
    assert W.head_shapes(arch, 7) == {"head.fc.weight": (7, 2048, 1, 1), "head.fc.bias": (7,)}
    assert list(shapes)[:4] == ["stem.conv.weight", "stages.0.blocks.0.downsample.conv.weight", "stages.0.blocks.0.norm1.weight",
                                "stages.0.blocks.0.norm1.bias"]
    assert not any("running" in k or k.endswith("conv.bias") for k in shapes)
    assert not W.is_bit("resnet50") and not W.is_resnet_lib(arch)


def test_infer_arch_and_check_state_dict():
    for arch in ARCHS:
        sd = W.init_state_dict(arch, seed=1, num_classes=9)
        for d in (sd, {"net." + k: v for k, v in sd.items()}):
            assert W.infer_arch(d) == arch                                   # (the _bit names share keys and shapes: the _bitm name answers)
            assert W.infer_num_classes(d) == 9
        assert sorted(W.strip_prefix({"net." + k: v for k, v in sd.items()})) == sorted(sd)   # nothing but the prefix is dropped
        W.check_state_dict(arch, sd)
        W.check_state_dict(ALIAS[arch], sd, num_classes=9)
        flat = dict(sd)
        flat["head.fc.weight"] = sd["head.fc.weight"].reshape(9, 2048)       # the head as a matrix is accepted too
        W.check_state_dict(arch, flat, num_classes=9)
        assert W.infer_num_classes(flat) == 9
    sd = W.init_state_dict("resnetv2_50x1_bitm", seed=1)
    with pytest.raises(ValueError, match="stages.2.blocks.6"):
        W.check_state_dict("resnetv2_101x1_bitm", sd)
    missing = dict(sd)
    del missing["stages.1.blocks.0.downsample.conv.weight"]
    with pytest.raises(ValueError, match="missing stages.1.blocks.0.downsample.conv.weight"):
        W.check_state_dict("resnetv2_50x1_bitm", missing)
    # another depth (resnetv2_152: (3, 8, 36, 3) is not built here; two blocks fewer is as foreign) and another width (x3)
    short = {k: v for k, v in sd.items() if not k.startswith(("stages.2.blocks.5.", "stages.2.blocks.4."))}
    with pytest.raises(ValueError, match=r"unsupported BiT.*resnetv2_50x1_bitm.*resnetv2_101x1_bitm"):
        W.infer_arch(short)
    wide = {k: (v.repeat_interleave(3, 0) if v.dim() >= 1 else v) for k, v in sd.items()}
    with pytest.raises(ValueError, match="width factor 3"):
        W.infer_arch(wide)
    # the other families are still told apart
    assert W.infer_arch(W.init_state_dict("resnet50", seed=0)) == "resnet50"
    assert W.infer_arch(W.init_state_dict("convnext_tiny", seed=0)) == "convnext_tiny"


def test_seeded_init():
    arch = ARCHS[0]
    a, b, c = (W.init_state_dict(arch, seed=s) for s in (9, 9, 10))
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["stem.conv.weight"], c["stem.conv.weight"])
    assert 0.5 <= a["norm.weight"].min() and a["norm.weight"].max() <= 1.5
    assert a["stages.1.blocks.2.norm3.weight"].max() <= 0.375 and a["stages.1.blocks.2.norm3.weight"].min() >= 0.125
    t = W.init_state_dict(arch, seed=9, scale="timm")
    assert torch.count_nonzero(t["stages.0.blocks.1.norm3.weight"]) == 0 and torch.all(t["stages.0.blocks.1.norm1.weight"] == 1)
    h = W.init_state_dict(arch, seed=9, num_classes=5)
    assert all(torch.equal(h[k], a[k]) for k in a) and h["head.fc.weight"].shape == (5, 2048, 1, 1)


@pytest.mark.parametrize("arch", ARCHS)
def test_checkpoint_and_factories_round_trip(arch, tmp_path):
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.encoders import AutoEncoderFactory, BitEncoder, make_encoder  # noqa: F401
    sd = W.init_state_dict(arch, seed=2, num_classes=6)
    path = tmp_path / "enc_best.pth"
    W.save_checkpoint(sd, path)
    raw = torch.load(path, weights_only=True)
    assert all(k.startswith("net.") for k in raw)
    back = W.load_checkpoint(path)
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    assert W.infer_arch(back) == arch
    enc = AutoEncoderFactory("timm", arch).load(str(path))                   # CPU only: the engine is built on first forward
    assert sum(p.numel() for _, p in enc.named_parameters()) == COUNTS[arch]
    enc2 = AutoEncoderFactory("timm", ALIAS[arch])()
    enc2.load_state_dict(enc.state_dict())
    assert all(torch.equal(v, sd[k[4:]]) for k, v in enc2.state_dict().items())
    clf = AutoClassifierFactory("timm", arch, n_classes=6).load(str(path))
    st = clf.state_dict()
    assert st["net.head.fc.weight"].shape == (6, 2048, 1, 1)
    assert sum(p.numel() for _, p in clf.named_parameters()) == COUNTS[arch] + 6 * 2048 + 6
    clf2 = AutoClassifierFactory("timm", arch, n_classes=6)()
    clf2.load_state_dict(st)
    assert all(torch.equal(v, sd[k[4:]]) for k, v in clf2.state_dict().items())
    with pytest.raises(ValueError):
        AutoClassifierFactory("timm", arch, n_classes=5)().load_state_dict(st)


def test_refusals():
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.encoders import AutoEncoderFactory
    for name in ("resnetv2_50", "resnetv2_50x3_bitm", "resnetv2_152x2_bitm"):
        with pytest.raises(NotImplementedError):
            AutoEncoderFactory("timm", name)
        with pytest.raises(NotImplementedError):
            AutoClassifierFactory("timm", name, 5)
        with pytest.raises(NotImplementedError):
            W.param_shapes(name)
    with pytest.raises(NotImplementedError):
        AutoEncoderFactory("hf", "google/bit-50")
    with pytest.raises(NotImplementedError):
        AutoClassifierFactory("hf", "google/bit-50", 5)


# -- libeffocr_bit.so -----------------------------------------------------------------------------------------------------------------
def test_library_exports_its_header_and_versions_agree():
    src = open(os.path.join(ROOT, "include", "effocr_bit.h")).read()
    declared = sorted(set(re.findall(r"\b(effocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert len(declared) == 19
    raw = ctypes.CDLL(_lib.BIT_SO_PATH)
    for n in declared:
        assert hasattr(raw, n), f"{n} declared in effocr_bit.h but not exported"
    assert sorted(_lib.BIT_EXPORTS) == declared
    v = int(re.search(r"#define\s+EFFOCR_BIT_ABI_VERSION\s+(\d+)", src).group(1))
    assert _lib.bit_lib().effocr_bit_abi_version() == v == _lib.BIT_ABI_VERSION == 1
    # it exports effocr_bit_* and no other project function (weak C++ library instances aside, as libeffocr_resnet.so)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.BIT_SO_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    ours = sorted(s for s in (line.split()[-1] for line in nm.splitlines()) if "effocr" in s)
    assert ours == declared, ours
    for hidden in ("effocr_abi_version", "effocr_encoder_create", "effocr_resnet_create"):
        assert not hasattr(raw, hidden), hidden
    ldd = subprocess.run(["ldd", _lib.BIT_SO_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libeffocr" not in ldd                                            # it links no other library of the project
    _lib.lib()
    assert not set(declared) & set(_lib.EXPORTS)


@pytest.mark.parametrize("arch", ARCHS + list(ALIAS.values()))
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_c_handle_tables_without_gpu(arch, prec):
    L = _lib.bit_lib()
    h = ctypes.c_void_p()
    assert L.effocr_bit_create(arch.encode(), 224, _lib.PREC[prec], ctypes.byref(h)) == 0, L.effocr_bit_last_error()
    try:
        assert L.effocr_bit_embed_dim(h) == 2048
        shapes = W.param_shapes(arch)
        n = L.effocr_bit_num_params(h)
        names = [L.effocr_bit_param_name(h, i).decode() for i in range(n)]
        assert names == list(shapes)
        for i, k in enumerate(names):
            assert L.effocr_bit_param_numel(h, i) == math.prod(shapes[k])
        assert L.effocr_bit_param_name(h, n) is None and L.effocr_bit_param_numel(h, -1) == -1
        es = 4 if prec == "fp32" else 2
        count = sum(math.prod(s) for s in shapes.values())
        assert es * count <= L.effocr_bit_weights_bytes(h) <= 4 * count * 1.01
        assert L.effocr_bit_workspace_bytes(h, 0) == 0
        ws = [L.effocr_bit_workspace_bytes(h, b) for b in (1, 2, 3, 8, 64, 4096)]
        assert 0 < ws[0] and all(a <= b for a, b in zip(ws, ws[1:])) and ws[0] < ws[1] < ws[3] and ws[-1] < 1000 << 20
        assert L.effocr_bit_set_chunk(h, 8) == 0
        assert L.effocr_bit_workspace_bytes(h, 4096) == ws[3]
        assert L.effocr_bit_set_chunk(h, -1) == -1
        t = torch.zeros(5)
        assert L.effocr_bit_set_param(h, b"norm.weight", _lib.ptr(t), 5) == -1
        assert b"expects 2048" in L.effocr_bit_last_error()
        for absent in (b"head.fc.weight", b"stem.conv.bias", b"stages.0.blocks.1.downsample.conv.weight", b"stages.0.blocks.0.norm1.running_mean"):
            assert L.effocr_bit_set_param(h, absent, _lib.ptr(t), 5) == -1
        assert L.effocr_bit_set_param(h, None, _lib.ptr(t), 5) == -1
        p = ctypes.c_void_p(4096)                                            # never dereferenced: these calls are refused first
        assert L.effocr_bit_upload(h, p, L.effocr_bit_weights_bytes(h)) == -5
        assert L.effocr_bit_upload(h, p, 1) == -3
        assert L.effocr_bit_forward(h, p, 2, p, 0, p, 1 << 40, None) == -5
        assert L.effocr_bit_forward(h, p, -1, p, 0, p, 1 << 40, None) == -1
        assert L.effocr_bit_forward(h, p, 0, p, 0, p, 0, None) == 0
        assert L.effocr_bit_check_status(h, None, None) == -1
        assert L.effocr_bit_reset_status(h, None, None) == -1
    finally:
        L.effocr_bit_destroy(h)


def test_c_create_refusals():
    L = _lib.bit_lib()
    h = ctypes.c_void_p()
    for img in (0, 16, 48, 100, -32):
        assert L.effocr_bit_create(b"resnetv2_50x1_bitm", img, 1, ctypes.byref(h)) == -1
        assert b"img_size must be a positive multiple of 32" in L.effocr_bit_last_error()
    for img in (32, 96, 448):
        assert L.effocr_bit_create(b"resnetv2_50x1_bitm", img, 1, ctypes.byref(h)) == 0
        L.effocr_bit_destroy(h)
    for prec in (-1, 3):
        assert L.effocr_bit_create(b"resnetv2_50x1_bitm", 224, prec, ctypes.byref(h)) == -1
        assert b"precision" in L.effocr_bit_last_error()
    for name in (b"resnetv2_50", b"resnetv2_50x3_bitm", b"resnetv2_152x2_bitm", b"resnet50"):
        assert L.effocr_bit_create(name, 224, 1, ctypes.byref(h)) == -2
        assert b"unsupported architecture" in L.effocr_bit_last_error()
    assert L.effocr_bit_create(None, 224, 1, ctypes.byref(h)) == -1
    assert L.effocr_bit_create(b"resnetv2_50x1_bitm", 224, 1, None) == -1
    assert L.effocr_bit_forward(None, None, 1, None, 0, None, 0, None) == -1
    assert L.effocr_bit_embed_dim(None) == 0 and L.effocr_bit_num_params(None) == 0
    p = ctypes.c_void_p(4096)
    assert L.effocr_bit_op_groupnorm_relu(1, None, 1, 4, 64, p, p, p, p, 1 << 20, None) == -1
    assert L.effocr_bit_op_groupnorm_relu(1, p, 1, 4, 96, p, p, p, p, 1 << 20, None) == -2      # channels: a power of two
    assert L.effocr_bit_op_groupnorm_relu(1, p, 1, 4, 64, p, p, p, p, 16, None) == -3           # scratch too small
    assert L.effocr_bit_op_groupnorm_relu(5, p, 1, 4, 64, p, p, p, p, 1 << 20, None) == -1
    assert L.effocr_bit_op_stem_pool(1, p, 1, 8, 8, 12, p, None) == -2
    assert L.effocr_bit_op_stem_pool(1, None, 1, 8, 8, 64, p, None) == -1
    assert L.effocr_bit_op_head(1, p, 1, 4, 100, p, p, 0, p, None, None) == -2
    assert L.effocr_bit_op_head(1, p, 1, 0, 2048, p, p, 0, p, None, None) == -1
    lib = _lib.lib()
    for name in (b"resnetv2_50x1_bitm", b"resnetv2_101x1_bitm"):
        assert lib.effocr_encoder_create(name, 224, 1, ctypes.byref(h)) == -2                   # the product library still refuses them


# -- operator bounds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.GN_CASES))
def test_groupnorm_bound_accepts_the_contract_and_rejects_mutants(name):
    for prec in R.GN_CASES[name][5]:
        x, gamma, beta = R.gn_case(name, prec)
        ref, bound = R.gn_relu_ref(x, gamma, beta), R.gn_bound(x, gamma, beta, prec)
        w = R.worst(R.gn_relu_emul(x, gamma, beta, prec), ref, bound)
        assert w <= 1, (name, prec, w)
        muts = R.gn_mutants(x, gamma, beta)
        if name == "mean = 20 sigma":
            muts["E[x^2] - mean^2 in float32"] = R.gn_mutant_ex2(x, gamma, beta)
        for m, out in muts.items():
            wm = R.worst(out, ref, bound)
            # what a case can tell apart at all: eps matters only where the variance is of its size, and an n / (n - 1) variance only
            # where n is small or the type fine enough
            if m == "eps omitted" and name != "scaled by 3e-3":
                continue
            if m == "unbiased variance" and not (prec == "fp32" or name == "head width, one pixel"):
                continue
            assert wm > 1, (name, prec, m, wm)


@pytest.mark.parametrize("name", list(R.POOL_CASES))
def test_stem_pool_mutant_differs(name):
    x = R.pool_case(name, "fp16")
    ref = R.stem_pool_ref(x)
    assert ref.shape == (x.shape[0], x.shape[1] // 2, x.shape[2] // 2, x.shape[3])
    assert (ref[:, 0] == 0).any() and (ref >= 0)[:, 0].all()                 # the zero padding wins on the negative border
    assert not torch.equal(R.stem_pool_mutant(x), ref)


@pytest.mark.parametrize("name", list(R.HEAD_CASES))
@pytest.mark.parametrize("l2", [False, True])
def test_head_bound_accepts_float32_and_rejects_mutants(name, l2):
    for prec in ("fp32", "fp16", "bf16"):
        x, gamma, beta = R.head_case(name, prec)
        ref, bound = R.head_ref(x, gamma, beta, l2), R.head_bound(x, gamma, beta, l2)
        emul = R.gn_relu_emul(x, gamma, beta, "fp32").float().mean(dim=1)
        if l2:
            emul = torch.nn.functional.normalize(emul, dim=1)
        w = R.worst(emul.double(), ref, bound)
        assert w <= 1, (name, prec, w)
        for m, out in R.head_mutants(x, gamma, beta, l2).items():
            if m == "mean before ReLU" and name == "HW 1":
                continue                                                     # one pixel: the mean is the value
            assert R.worst(out, ref, bound) > 1, (name, prec, m)
