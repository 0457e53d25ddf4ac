"""RegNetX / RegNetY without a GPU: the width generator and the parameter tables against timm's published counts, the CPU restatement
(tests/regnet_ref.py) against an independent implementation (transformers.RegNetModel), the checkpoint loader, the factories and
libeffocr_regnet.so's C ABI (exports, version, handle, messages, refusals)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from effocr_amd import _lib
from effocr_amd import weights as W
from tests.regnet_ref import ARCHS, MISTAKES, TEN, gconv_emulated, gconv_ref, header_constants, hf_config, hf_state_dict, regnet_forward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI8, MINI16, MINI24 = "regnetx_mini8_test", "regnetx_mini16_test", "regnety_mini24_test"
NAMES = "regnetx_002, regnetx_004, regnetx_006, regnetx_008, regnetx_016, regnety_002, regnety_004, regnety_006, regnety_008, regnety_016"
# timm's published parameter counts: with the 1000-class head / headless
N_PARAMS = {"regnetx_002": (2684792, 2315792), "regnetx_004": (5157512, 4772512), "regnetx_006": (6196040, 5667040),
            "regnetx_008": (7259656, 6586656), "regnetx_016": (9190136, 8277136), "regnety_002": (3162996, 2793996),
            "regnety_004": (4344144, 3903144), "regnety_006": (6055160, 5446160), "regnety_008": (6263168, 5494168),
            "regnety_016": (11202430, 10313430)}
UNSUPPORTED = ("regnetx_032", "regnety_032", "regnetx_040", "regnety_320", "regnetz_b16", "regnetv_040")


def test_generator_reproduces_the_table():
    assert tuple(N_PARAMS) == TEN == W.REGNET_SUPPORTED
    for arch in TEN:
        widths, depths, gw, se = ARCHS[arch]
        w0, wa, wm, d, g, s = W.REGNET_CFG[arch]
        assert W.regnet_widths(w0, wa, wm, d, g) == (widths, depths)
        assert W.regnet_arch(arch) == (widths, depths, gw, se) and sum(depths) == d
        assert W.embed_dim(arch) == widths[-1] and W.is_regnet(arch) and W._family(arch) == "regnet"
        assert W.head_keys(arch) == ("head.fc.weight", "head.fc.bias")
    for arch in (MINI8, MINI16, MINI24):
        assert W.regnet_arch(arch) == ARCHS[arch] and W.embed_dim(arch) == ARCHS[arch][0][-1]


def test_parameter_counts_match_timm():
    for arch, (headed, bare) in N_PARAMS.items():
        assert W.regnet_num_learnable(arch) == bare
        assert W.regnet_num_learnable(arch, num_classes=1000) == headed
        assert headed - bare == 1000 * (ARCHS[arch][0][-1] + 1)


def test_parameter_count_matches_transformers():
    from transformers import RegNetModel
    for arch in ("regnetx_002", "regnety_004"):
        assert sum(p.numel() for p in RegNetModel(hf_config(arch)).parameters()) == N_PARAMS[arch][1]


@pytest.mark.parametrize("arch,img", [("regnetx_006", 64), ("regnety_004", 64), (MINI8, 32), (MINI24, 32)])
def test_reference_matches_transformers(arch, img):
    """regnet_ref against transformers.RegNetModel.pooler_output on the same seeded weights (non-trivial BatchNorm statistics), fp32 on the
    CPU, bound 1e-5 in the max norm relative to max|ref|."""
    from transformers import RegNetModel
    sd = W.init_state_dict(arch, seed=11)
    m = RegNetModel(hf_config(arch))
    res = m.load_state_dict(hf_state_dict(arch, sd), strict=False)
    assert not res.unexpected_keys and all(k.endswith("num_batches_tracked") for k in res.missing_keys)
    m.eval()
    x = torch.randn(3, 3, img, img, generator=torch.Generator().manual_seed(img))
    with torch.no_grad():
        want = m(x).pooler_output.flatten(1)
    got = regnet_forward(arch, sd, x)
    assert got.shape == (3, ARCHS[arch][0][-1]) and got.dtype == torch.float32
    rel = ((got - want).abs().max() / want.abs().max()).item()
    assert rel <= 1e-5, rel
    ref64 = regnet_forward(arch, sd, x.double())
    assert ((got.double() - ref64).abs().max() / ref64.abs().max()).item() <= 1e-5
    assert (ref64[0] - ref64[1]).norm() / ref64[0].norm() > 0.01                   # the embedding depends on the crop
    # the folded-BN form of the emulation without any 16-bit rounding is the same network
    fold = regnet_forward(arch, sd, x.double(), prec="fp32")
    assert ((fold - ref64).abs().max() / ref64.abs().max()).item() <= 1e-6
    for mistake in MISTAKES:                                                       # every wrong network is a different network
        if mistake == "no_gate" and not ARCHS[arch][3]:
            continue
        bad = regnet_forward(arch, sd, x.double(), mistake=mistake)
        assert ((bad - ref64).norm(dim=1) / ref64.norm(dim=1)).min().item() > 1e-3, mistake


def test_gconv_emulation_is_the_reference_up_to_the_roundings():
    g = torch.Generator().manual_seed(5)
    for gw, groups, stride in ((8, 3, 1), (16, 2, 2), (24, 3, 1)):
        C = gw * groups
        x, w, b = torch.randn(2, C, 7, 7, generator=g), torch.randn(C, gw, 3, 3, generator=g) / (3 * gw ** 0.5), torch.randn(C, generator=g) * 0.1
        ref = gconv_ref(x.double(), w.double(), b.double(), stride, gw)
        assert ((gconv_emulated(x, w, b, stride, gw, "fp32").double() - ref).abs().max() / ref.abs().max()).item() <= 1e-6
        for prec, lim in (("fp16", 2e-6), ("bf16", 1e-4)):                         # on weights already rounded: hi + lo loses 2^-22 / 2^-16
            wr = w.to(torch.float16 if prec == "fp16" else torch.bfloat16).float()
            ref = gconv_ref(x.double(), wr.double(), b.double(), stride, gw)
            assert ((gconv_emulated(x, w, b, stride, gw, prec).double() - ref).abs().max() / ref.abs().max()).item() <= lim


def test_infer_arch_answers_every_name_with_and_without_prefix(tmp_path):
    for arch in TEN + (MINI8, MINI16, MINI24):
        sd = W.init_state_dict(arch, seed=1, scale="timm", num_classes=5 if arch == "regnety_002" else 0)
        assert W.infer_arch(sd) == arch
        assert W.infer_arch({"net." + k: v for k, v in sd.items()}) == arch
        W.check_state_dict(arch, sd, 224)
    sd = W.init_state_dict("regnety_002", seed=1, num_classes=5)
    assert W.infer_num_classes(sd) == 5
    W.save_checkpoint(sd, tmp_path / "enc.pth")
    back = W.load_checkpoint(tmp_path / "enc.pth")
    assert W.infer_arch(back) == "regnety_002" and all(torch.equal(back[k], v) for k, v in sd.items())


def test_wrong_checkpoints_are_refused_with_the_list_of_names():
    x = W.init_state_dict("regnetx_002", scale="timm")
    y = W.init_state_dict("regnety_002", scale="timm")
    with_se = dict(x)
    with_se.update({k: v for k, v in y.items() if ".se." in k and not k.startswith("s1.b1.")})  # (with ALL of them it is regnety_002)
    without_se = {k: v for k, v in y.items() if ".se." not in k or k.startswith("s1.b1.")}     # Y by its first block, the rest stripped
    depth = {k: v for k, v in x.items() if not k.startswith("s4.b7.")}
    deeper = dict(x)
    deeper.update({k.replace("s4.b7.", "s4.b8."): v for k, v in x.items() if k.startswith("s4.b7.")})
    group = {k: (v[:, :4].contiguous() if k.endswith("conv2.conv.weight") else v) for k, v in x.items()}
    only_x_keys = {k: v for k, v in y.items() if ".se." not in k}
    assert W.infer_arch(only_x_keys) == "regnetx_002"                              # (Y without any se key IS the X of the same shapes)
    for bad in (with_se, without_se, depth, deeper, group):
        with pytest.raises(ValueError, match=NAMES):
            W.infer_arch(bad)
    wide = W.init_state_dict("regnetx_002", scale="timm")
    wide["s1.b1.conv1.conv.weight"] = torch.zeros(96, 32, 1, 1)
    with pytest.raises(ValueError, match=NAMES):
        W.infer_arch(wide)


def test_unsupported_regnets_are_refused_by_name():
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.encoders import AutoEncoderFactory
    for name in UNSUPPORTED:
        for call in (lambda: W.embed_dim(name), lambda: AutoEncoderFactory("timm", name), lambda: AutoClassifierFactory("timm", name, 10),
                     lambda: W.param_shapes(name), lambda: W.head_keys(name)):
            with pytest.raises(NotImplementedError, match=NAMES):
                call()
        assert not W.is_regnet(name)


def test_factories_accept_regnet(tmp_path):
    from effocr_amd import EffOCRHipError
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.encoders import AutoEncoderFactory, RegNetEncoder, make_encoder
    for arch in ("regnetx_002", "regnety_016"):
        enc = AutoEncoderFactory("timm", arch)()           # NotImplementedError before libeffocr_regnet.so existed
        assert enc.arch == arch
        assert sum(p.numel() for _, p in enc.named_parameters()) == N_PARAMS[arch][1]
        clf = AutoClassifierFactory("timm", arch, n_classes=1000)()
        assert sum(p.numel() for p in clf.parameters()) == N_PARAMS[arch][0]
    sd = W.init_state_dict(MINI24, seed=4, num_classes=7)
    W.save_checkpoint(sd, tmp_path / "clf.pth")
    clf = AutoClassifierFactory("timm", MINI24, n_classes=7, img_size=64).load(str(tmp_path / "clf.pth"))
    got = clf.state_dict()
    assert sorted(got) == sorted("net." + k for k in sd) and all(torch.equal(got["net." + k], v) for k, v in sd.items())
    assert sum(p.numel() for p in clf.parameters()) == W.regnet_num_learnable(MINI24, 7)
    enc = AutoEncoderFactory("timm", MINI24, img_size=64).load(str(tmp_path / "clf.pth"))
    back = enc.state_dict()
    assert all(torch.equal(back["net." + k], v) for k, v in sd.items())
    if not torch.cuda.is_available():                      # no GPU: a loud failure, never NotImplementedError or a fallback
        from effocr_amd.recognizer_engine import EffRecognizer
        with pytest.raises(EffOCRHipError):
            enc.to("cuda")(torch.zeros(1, 3, 64, 64))
        with pytest.raises(EffOCRHipError):
            clf.to("cuda")(torch.zeros(1, 3, 64, 64))
        with pytest.raises(EffOCRHipError):
            make_encoder(MINI24, sd, img_size=64)
        with pytest.raises(EffOCRHipError):
            RegNetEncoder("regnetx_002", W.init_state_dict("regnetx_002", scale="timm"))
        with pytest.raises(EffOCRHipError):
            EffRecognizer(str(tmp_path / "clf.pth"), img_size=64)


# -- libeffocr_regnet.so ------------------------------------------------------------------------------------------------------------
def test_regnet_library_exports_its_header_and_versions_agree():
    src = open(os.path.join(ROOT, "include", "effocr_regnet.h")).read()
    declared = sorted(set(re.findall(r"\b(effocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert len(declared) == 24
    raw = ctypes.CDLL(_lib.REGNET_SO_PATH)
    for n in declared:
        assert hasattr(raw, n), f"{n} declared in effocr_regnet.h but not exported"
    assert sorted(_lib.REGNET_EXPORTS) == declared
    v = int(re.search(r"#define\s+EFFOCR_REGNET_ABI_VERSION\s+(\d+)", src).group(1))
    assert _lib.regnet_lib().effocr_regnet_abi_version() == v == _lib.REGNET_ABI_VERSION == 1
    # it exports effocr_regnet_* only: the dynamic symbol table holds no other defined symbol
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.REGNET_SO_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    defined = sorted(line.split()[-1] for line in nm.splitlines())
    assert defined == declared, defined
    for hidden in ("effocr_abi_version", "effocr_encoder_create", "effocr_mnv3_create", "effocr_effnet_create"):
        assert not hasattr(raw, hidden), hidden
    _lib.lib()
    assert not set(declared) & set(_lib.EXPORTS)
    assert not hasattr(ctypes.CDLL(_lib.SO_PATH), "effocr_regnet_create")


def test_product_library_still_refuses_regnet(hip_lib):
    h = ctypes.c_void_p()
    for name in ("regnetx_002", "regnety_016", MINI8):
        assert hip_lib.effocr_encoder_create(name.encode(), 224, 1, ctypes.byref(h)) == -2


def test_regnet_handle_messages_and_refusals():
    L = _lib.regnet_lib()
    h = ctypes.c_void_p()
    for arch, img in [(a, 224) for a in TEN] + [(MINI8, 32), (MINI16, 64), (MINI24, 96), ("regnety_008", 320)]:
        shapes = W.param_shapes(arch)
        for prec in (0, 1, 2):
            assert L.effocr_regnet_create(arch.encode(), img, prec, ctypes.byref(h)) == 0
            try:
                assert L.effocr_regnet_embed_dim(h) == ARCHS[arch][0][-1]
                n = L.effocr_regnet_num_params(h)
                names = [L.effocr_regnet_param_name(h, i).decode() for i in range(n)]
                assert names == list(shapes)                                       # timm's state-dict order
                for i, k in enumerate(names):
                    assert L.effocr_regnet_param_numel(h, i) == torch.Size(shapes[k]).numel()
                assert L.effocr_regnet_param_name(h, n) is None and L.effocr_regnet_param_numel(h, -1) == -1
                assert L.effocr_regnet_weights_bytes(h) > 0
                ws1 = L.effocr_regnet_workspace_bytes(h, 1)
                ws = L.effocr_regnet_workspace_bytes(h, 4096)
                assert 0 < ws1 <= ws < (1 << 30)                                   # sub-batches keep the workspace under 1 GB
                assert L.effocr_regnet_workspace_bytes(h, 0) == 0
                assert L.effocr_regnet_set_chunk(h, 5) == 0
                assert L.effocr_regnet_workspace_bytes(h, 4096) == L.effocr_regnet_workspace_bytes(h, 5) <= ws
                assert L.effocr_regnet_set_chunk(h, -1) == -1
                assert L.effocr_regnet_last_error() == b"regnet_set_chunk: bad argument"
                assert L.effocr_regnet_set_chunk(h, 65536) == -1
                one = torch.zeros(1)
                assert L.effocr_regnet_set_param(h, b"stem.bn.weight", _lib.ptr(one), 1) == -1
                assert L.effocr_regnet_last_error() == b"regnet_set_param: 'stem.bn.weight' expects 32 elements, got 1"
                for absent in (b"head.fc.weight", b"stem.bn.num_batches_tracked", b"s1.b2.downsample.conv.weight" if ARCHS[arch][1][0] > 1 else b"s1.b9.conv1.conv.weight"):
                    assert L.effocr_regnet_set_param(h, absent, _lib.ptr(one), 1) == -1
                    assert L.effocr_regnet_last_error() == b"regnet_set_param: unknown parameter '" + absent + b"'"
                assert L.effocr_regnet_set_param(h, None, _lib.ptr(one), 1) == -1
                p = ctypes.c_void_p(4096)                                          # never dereferenced: every check below fails first
                assert L.effocr_regnet_upload(h, p, L.effocr_regnet_weights_bytes(h)) == -5
                assert L.effocr_regnet_last_error() == b"regnet_upload: parameter 'stem.conv.weight' was never set"
                assert L.effocr_regnet_upload(h, p, 1) == -3
                assert L.effocr_regnet_upload(h, None, 1 << 30) == -1
                assert L.effocr_regnet_forward(h, p, 2, p, 0, p, 1 << 40, None) == -5
                assert L.effocr_regnet_last_error() == b"regnet_forward: weights were not uploaded"
                assert L.effocr_regnet_forward(h, p, -1, p, 0, p, 1 << 40, None) == -1
                assert L.effocr_regnet_forward(h, None, 2, p, 0, p, 1 << 40, None) == -1
                assert L.effocr_regnet_forward(h, p, 0, p, 0, p, 0, None) == 0
                assert L.effocr_regnet_check_status(h, None, None) == -1
                assert L.effocr_regnet_reset_status(h, None, None) == -1
            finally:
                L.effocr_regnet_destroy(h)
    for size in (0, 16, 48, 100, -32):
        assert L.effocr_regnet_create(b"regnetx_002", size, 1, ctypes.byref(h)) == -1
        assert L.effocr_regnet_last_error() == b"regnet_create: img_size must be a positive multiple of 32 (at most 4096)"
    for prec in (-1, 3):
        assert L.effocr_regnet_create(b"regnetx_002", 224, prec, ctypes.byref(h)) == -1
    for name in tuple(n.encode() for n in UNSUPPORTED) + (b"resnet50", b"nope"):
        assert L.effocr_regnet_create(name, 224, 1, ctypes.byref(h)) == -2
        assert L.effocr_regnet_last_error() == b"regnet_create: unsupported architecture '" + name + b"' (supported: " + NAMES.encode() + b")"
    assert L.effocr_regnet_create(None, 224, 1, ctypes.byref(h)) == -1
    assert L.effocr_regnet_create(b"regnetx_002", 224, 1, None) == -1
    assert L.effocr_regnet_forward(None, None, 1, None, 0, None, 0, None) == -1
    assert L.effocr_regnet_embed_dim(None) == 0 and L.effocr_regnet_num_params(None) == 0
    p = ctypes.c_void_p(4096)
    assert L.effocr_regnet_op_gconv(1, None, 1, 8, 16, 1, 16, p, p, p, None, None) == -1
    assert L.effocr_regnet_op_gconv(1, p, 1, 8, 20, 1, 16, p, p, p, None, None) == -1          # channels no multiple of the group width
    assert L.effocr_regnet_op_gconv(1, p, 1, 8, 32, 1, 32, p, p, p, None, None) == -1          # group width 32
    assert L.effocr_regnet_op_gconv(1, p, 1, 8, 16, 3, 16, p, p, p, None, None) == -1
    assert L.effocr_regnet_op_gconv(1, p, 70000, 8, 16, 1, 16, p, p, p, None, None) == -2      # refused before any launch
    assert L.effocr_regnet_op_se_gate(None, 1, 1, 1, 8, 2, p, p, p, p, p, None) == -1
    assert L.effocr_regnet_op_se_gate(p, 1, 1, 1, 2048, 2, p, p, p, p, p, None) == -2
    assert L.effocr_regnet_op_stem(p, 1, 32, p, p, None, None) == -1
    assert L.effocr_regnet_op_stem(p, 1, 33, p, p, p, None) == -2
    assert L.effocr_regnet_op_gather2(p, 1, 4, 6, p, None) == -2
    assert L.effocr_regnet_op_gather2(None, 1, 4, 8, p, None) == -1
    assert L.effocr_regnet_op_relu(p, 6, None) == -2 and L.effocr_regnet_op_relu(None, 8, None) == -1
    assert L.effocr_regnet_op_pack_gconv(1, 16, 16, None, p) == -1
    assert L.effocr_regnet_op_gconv_weight_bytes(1, 20, 16) == 0 and L.effocr_regnet_op_tiles(0) == 0


def test_packed_grouped_weight_layout():
    """The host packing the kernels read: fp32 [9][C][gw]; 16-bit [C/16 tiles][9][input tiles][16][16], rounded once, zero between groups;
    the wasted fraction DESIGN.md states (0 for width 16, 1/2 for width 8, 5/14 for width 24 on whole periods of three tiles)."""
    L = _lib.regnet_lib()
    g = torch.Generator().manual_seed(2)
    for gw, groups, waste in ((16, 3, 0.0), (8, 4, 0.5), (8, 3, None), (24, 2, 5 / 14), (24, 3, None)):
        C = gw * groups
        w = torch.randn(C, gw, 3, 3, generator=g)
        n32 = L.effocr_regnet_op_gconv_weight_bytes(2, C, gw)
        assert n32 == 9 * C * gw * 4
        out = torch.zeros(n32 // 4)
        assert L.effocr_regnet_op_pack_gconv(2, C, gw, _lib.ptr(w), _lib.ptr(out)) == 0
        assert torch.equal(out.view(9, C, gw), w.reshape(C, gw, 9).permute(2, 0, 1))
        nkt = 3 if gw == 24 else 1
        n16 = L.effocr_regnet_op_gconv_weight_bytes(1, C, gw)
        tiles = (C + 15) // 16
        assert n16 == tiles * 9 * nkt * 256 * 2
        p16 = torch.full((n16 // 2,), 7.0, dtype=torch.float16)
        assert L.effocr_regnet_op_pack_gconv(1, C, gw, _lib.ptr(w), _lib.ptr(p16)) == 0
        p16 = p16.view(tiles, 9, nkt, 16, 16)
        dense = torch.zeros(9, C, C)                                               # the convolution as a dense [tap][out][in] matrix
        for o in range(C):
            dense[:, o, o // gw * gw:o // gw * gw + gw] = w[o].reshape(gw, 9).t()
        dense = dense.to(torch.float16)
        rebuilt = torch.zeros(9, tiles * 16, (tiles + 3) * 16, dtype=torch.float16)
        used = 0
        for ct in range(tiles):
            lo = ct * 16 // gw * gw
            hi = min(C, ((ct * 16 + 15) // gw + 1) * gw)
            kt0, n = lo // 16, (hi + 15) // 16 - lo // 16
            assert 1 <= n <= nkt and not p16[ct, :, n:].any()
            used += n
            for j in range(n):
                rebuilt[:, ct * 16:ct * 16 + 16, (kt0 + j) * 16:(kt0 + j) * 16 + 16] = p16[ct, :, j]
        assert torch.equal(rebuilt[:, :C, :C], dense) and not rebuilt[:, C:].any() and not rebuilt[:, :, C:].any()
        if waste is not None:
            assert abs(1 - C * gw / (used * 256) - waste) < 1e-9


def test_gpu_test_shapes_surround_the_kernel_tiles():
    """The shapes tests/test_gpu_regnet_ops.py walks lie below, at and above the tile sizes csrc/regnet.hpp declares: output maps of fewer
    than, exactly and more than RG_PIX_TILE pixels (one partial workgroup, one full, several with a partial last), channel counts of
    less than one, exactly one and several RG_CH_TILE tiles with a partial last one, for every group width."""
    from tests.test_gpu_regnet_ops import GROUP_COUNTS, GROUP_WIDTHS, SIZES, SE_SHAPES
    c = header_constants(os.path.join(ROOT, "effocr_amd", "csrc", "regnet.hpp"))
    assert c["RG_PIX_TILE"] == 64 and c["RG_CH_TILE"] == 16 and c["RG_STEM_C"] == 32
    outs = sorted({((h - 1) // s + 1) ** 2 for s, hs in SIZES.items() for h in hs})
    assert outs[0] == 1 and c["RG_PIX_TILE"] in outs and any(o < c["RG_PIX_TILE"] for o in outs)
    assert any(o > c["RG_PIX_TILE"] and o % c["RG_PIX_TILE"] for o in outs) and any(o > 2 * c["RG_PIX_TILE"] for o in outs)
    assert SIZES == {1: (1, 2, 3, 7, 8, 14), 2: (2, 4, 8, 14, 16)} and GROUP_WIDTHS == (8, 16, 24) and GROUP_COUNTS == (1, 2, 3, 7)
    chans = sorted({gw * n for gw in GROUP_WIDTHS for n in GROUP_COUNTS})
    assert chans[0] < c["RG_CH_TILE"] and c["RG_CH_TILE"] in chans and any(ch > c["RG_CH_TILE"] and ch % c["RG_CH_TILE"] for ch in chans)
    assert max(C for C, _ in SE_SHAPES) <= c["RG_SE_MAXC"] and max(R for _, R in SE_SHAPES) <= c["RG_SE_MAXR"]
    assert max(ARCHS[a][0][-1] for a in TEN) <= c["RG_SE_MAXC"] and max(ARCHS[a][0][-1] for a in TEN) // 4 <= c["RG_SE_MAXR"]
