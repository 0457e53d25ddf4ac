"""Host side of the YOLO11 n / s / m / l / x localizers (no GPU): the parameter tables against the module tree of tests/yolo11_ref.py and
the parameter counts ultralytics publishes, scale inference from a checkpoint and its refusals, the functional restatement against the
module tree, the size of the attention logits the seeded weights give, the mutation check of the CPU reference, and
libeffocr_yolo11.so's handle tables, sizes, refusals and exports."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from effocr_amd import _lib
from effocr_amd.localizer_engine import (YOLO11_DFL_KEY, YOLO11_SCALES, init_yolo11_state_dict, init_yolov5_state_dict, init_yolov8_state_dict,
                                         yolo11_param_shapes, yolo11_scale, yolov5_scale, yolov8_scale)
from tests.yolo11_ref import (BOX_REL, MISTAKES, NET_CASES, SCALES as REF_SCALES, SCORE_ABS, Yolo11, attention_exact, attention_logit_std,
                              attention_tiled, make_case, row_errors, yolo11_forward)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = "nsmlx"
# learnable parameters (conv weights, BN weight and bias, the biased 1x1 convs) plus the 16 DFL weights; BN running statistics are buffers.
# The nc = 80 counts are the ones ultralytics prints for the unfused models (2.6 / 9.5 / 20.1 / 25.4 / 57.0 M)
COUNTS = {80: {"n": 2624080, "s": 9458752, "m": 20114688, "l": 25372160, "x": 56966176},
          2: {"n": 2590230, "s": 9428566, "m": 20054550, "l": 25312022, "x": 56876086}}


def _learnable(shapes):
    return sum(torch.Size(s).numel() for k, s in shapes.items() if not (k.endswith("running_mean") or k.endswith("running_var")))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("nc", [80, 2])
def test_pinned_parameter_counts(scale, nc):
    assert _learnable(yolo11_param_shapes(nc, scale)) == COUNTS[nc][scale]


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("nc", [1, 2, 80])
def test_param_shapes_match_the_module_tree(scale, nc):
    """Same keys, same shapes, same (module) order; and the module tree's own parameter count is the pinned one."""
    m = Yolo11(nc, scale)
    want = [(k, tuple(v.shape)) for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked")]
    assert [(k, tuple(v)) for k, v in yolo11_param_shapes(nc, scale).items()] == want
    assert want[-1][0] == YOLO11_DFL_KEY == "model.23.dfl.conv.weight"
    if nc in COUNTS:
        assert sum(p.numel() for p in m.parameters()) == COUNTS[nc][scale]
    assert YOLO11_SCALES == REF_SCALES


@pytest.mark.parametrize("scale", SCALES)
def test_scale_round_trips(scale):
    sd = init_yolo11_state_dict(2, scale, seed=1)
    assert yolo11_scale(sd) == scale
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v) for k, v in yolo11_param_shapes(2, scale).items()}
    again = init_yolo11_state_dict(2, scale, seed=1)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    assert yolo11_scale(init_yolo11_state_dict(80, scale, seed=2)) == scale
    with pytest.raises(ValueError, match="unknown YOLO11 scale"):
        yolo11_param_shapes(2, "z")


@pytest.mark.parametrize("scale", SCALES)
def test_mismatched_dicts_are_refused(scale):
    sd = init_yolo11_state_dict(2, scale, seed=1)
    bad = dict(sd)
    w = bad["model.3.conv.weight"]                                   # one channel count changed
    bad["model.3.conv.weight"] = torch.zeros(w.shape[0] + 8, *w.shape[1:])
    with pytest.raises(ValueError, match="model.3.conv.weight"):
        yolo11_scale(bad)
    one = {k: v for k, v in sd.items() if k != "model.10.m.0.attn.pe.bn.running_var"}    # one tensor dropped
    with pytest.raises(ValueError, match="missing model.10.m.0.attn.pe.bn.running_var"):
        yolo11_scale(one)
    dfl = dict(sd)                                                                       # a DFL tensor that is not 0 .. 15
    dfl[YOLO11_DFL_KEY] = sd[YOLO11_DFL_KEY].flip(1)
    with pytest.raises(ValueError, match="model.23.dfl.conv.weight is not the constant"):
        yolo11_scale(dfl)


def test_other_networks_are_refused():
    v5, v8, v11 = init_yolov5_state_dict(2, "s", seed=0), init_yolov8_state_dict(2, "s", seed=0), init_yolo11_state_dict(2, "s", seed=0)
    for other in (v5, v8):
        with pytest.raises(ValueError, match="not an ultralytics YOLO11"):
            yolo11_scale(other)
    with pytest.raises(ValueError, match="state dict has no 'model.24.m.0.bias'"):      # and the other engines say what they always said
        yolov5_scale(v11)
    with pytest.raises(ValueError, match="state dict has no 'model.22.dfl.conv.weight': not an ultralytics YOLOv8"):
        yolov8_scale(v11)
    v11["model.0.conv.weight"] = torch.zeros(24, 3, 3, 3)
    with pytest.raises(ValueError, match="24 output channels"):
        yolo11_scale(v11)


def test_m_l_mix_up_and_wrong_max_channels_are_refused():
    """m and l share every width and differ in depth alone: an m dict with l's second model.2 block is taken for l and refused with the
    first keys l has and it lacks.  yolo11l caps its channels at 512: a dict with model.7 widened to 1024 has l's stem and depth but is
    not l."""
    m, l = init_yolo11_state_dict(2, "m", seed=0), init_yolo11_state_dict(2, "l", seed=0)
    mixed = dict(m)
    mixed.update({k: v for k, v in l.items() if k.startswith("model.2.")})
    with pytest.raises(ValueError, match=r"does not match yolo11l: missing model.4.m.1.cv1.conv.weight"):
        yolo11_scale(mixed)
    w = l["model.7.conv.weight"]
    l["model.7.conv.weight"] = torch.zeros(1024, *w.shape[1:])
    for s in ("weight", "bias", "running_mean", "running_var"):
        l[f"model.7.bn.{s}"] = torch.zeros(1024)
    with pytest.raises(ValueError, match=r"does not match yolo11l \(model.7 is 1024 wide, yolo11l caps it at 512: another max_channels\): "
                                         r"model.7.conv.weight: shape \(1024, 512, 3, 3\) != \(512, 512, 3, 3\)"):
        yolo11_scale(l)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", [(64, 64), (96, 160)])
def test_functional_restatement_matches_the_module_tree(scale, shape):
    sd = init_yolo11_state_dict(2, scale, seed=3)
    m = Yolo11(2, scale)
    res = m.load_state_dict(sd, strict=False)                        # strict apart from BN's num_batches_tracked
    assert not res.unexpected_keys and all(k.endswith("num_batches_tracked") for k in res.missing_keys)
    m.eval()
    x = torch.rand(2, 3, *shape, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        a, b = m(x), yolo11_forward(sd, x, scale, dtype=torch.float32)
    assert a.shape == b.shape == (2, shape[0] * shape[1] // 64 * 21 // 16, 7)
    assert (a - b).abs().max().item() < 1e-5 * a.abs().max().item()
    assert (a[..., 4] == 1).all()


def test_tiled_attention_restatement_is_the_plain_softmax():
    """The running-maximum form the kernel uses equals softmax(q k^T / sqrt 32) v (float64, 150 tokens: two full key tiles and a part)."""
    qkv = torch.randn(2, 150, 4 * 128, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    qkv[..., :64] *= 1.5
    assert (attention_tiled(qkv, 4) - attention_exact(qkv, 4)).abs().max().item() < 1e-13


@pytest.mark.parametrize("scale", SCALES)
def test_seeded_attention_logits_are_neither_flat_nor_one_hot(scale):
    """init_yolo11_state_dict's q / k gain: the logits 32^-1/2 q . k of every PSABlock, taken about each query's mean over the keys (the
    part its softmax sees), have a standard deviation of order 1 on the inputs the GPU tests use (where there is more than one token)."""
    for shape in ((64, 64), (96, 160)):
        sd, x = make_case(scale, shape, 3)
        with torch.no_grad():
            stds = attention_logit_std(sd, x)
        assert len(stds) == (2 if scale in "lx" else 1)
        assert all(0.5 < s < 3.0 for s in stds), (scale, shape, stds)


# A mistake that cannot show at a shape: with ONE token (32 x 32) the softmax is 1 whatever the logits are.
MUTATION_DROPPED = {"no_scale": (32, 32), "softmax_over_queries": (32, 32)}


@pytest.mark.parametrize("scale,shape,nc", sorted({(s, shape, nc) for s, shape, _, nc in NET_CASES}))
def test_reference_mutations_move_every_image(scale, shape, nc):
    """Each of MISTAKES planted in the CPU reference moves the predictions of EVERY image of the GPU test cases (same seeds, the largest
    batch of each shape; the batch-1 case is its first image) by at least 10 x the fp32 bound — box error / BOX_REL or score error /
    SCORE_ABS, whichever is larger — so a device network with that mistake cannot pass tests/test_gpu_yolo11.py.  float32 restatements:
    their own error is three orders below the margin.  Dropped (MUTATION_DROPPED, one shape per mistake at most): the missing scale
    factor and the softmax over queries at 32 x 32, where the one token's softmax is 1 whatever the logits are."""
    B = max(b for s, sh, b, n in NET_CASES if (s, sh, n) == (scale, shape, nc))
    sd, x = make_case(scale, shape, B, nc)
    with torch.no_grad():
        ref = yolo11_forward(sd, x, scale, dtype=torch.float32)
        for mistake in MISTAKES:
            if MUTATION_DROPPED.get(mistake) == shape:
                continue
            got = yolo11_forward(sd, x, scale, dtype=torch.float32, mistake=mistake)
            for i in range(B):
                box, score = row_errors(got[i], ref[i])
                assert max(box / BOX_REL, score / SCORE_ABS) >= 10, (mistake, i, box, score)


# ---------------------------------------------------------------- libeffocr_yolo11.so
def _handle(L, arch, nc, h=640, w=640):
    hnd = ctypes.c_void_p()
    rc = L.effocr_yolo11_create(arch, nc, h, w, ctypes.byref(hnd))
    return rc, hnd


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("nc", [1, 2, 80])
def test_cabi_handle_table_equals_the_python_table(scale, nc):
    L = _lib.yolo11_lib()
    rc, h = _handle(L, f"yolo11{scale}".encode(), nc)
    assert rc == 0
    try:
        n = L.effocr_yolo11_num_params(h)
        got = [(L.effocr_yolo11_param_name(h, i).decode(), L.effocr_yolo11_param_numel(h, i)) for i in range(n)]
        want = [(k, torch.Size(v).numel()) for k, v in yolo11_param_shapes(nc, scale).items()]
        assert sorted(got) == sorted(want)
        assert L.effocr_yolo11_num_predictions(h) == 8400 and L.effocr_yolo11_num_outputs(h) == nc + 5
        conv_w = sum(torch.Size(v).numel() for v in yolo11_param_shapes(nc, scale).values() if len(v) == 4)
        assert L.effocr_yolo11_weights_bytes(h) >= 4 * conv_w               # at least the folded fp32 weights
        assert L.effocr_yolo11_param_name(h, n) is None and L.effocr_yolo11_param_numel(h, n) == -1
    finally:
        L.effocr_yolo11_destroy(h)


def test_cabi_num_predictions_and_sizes_follow_shape_and_scale():
    L = _lib.yolo11_lib()
    rc, h = _handle(L, b"yolo11n", 2, 64, 96)
    assert rc == 0 and L.effocr_yolo11_num_predictions(h) == 126
    L.effocr_yolo11_destroy(h)
    ws, wb = {}, {}
    for scale in SCALES:
        rc, h = _handle(L, f"yolo11{scale}".encode(), 2)
        assert rc == 0
        ws[scale] = L.effocr_yolo11_workspace_bytes(h, 16)
        wb[scale] = L.effocr_yolo11_weights_bytes(h)
        assert L.effocr_yolo11_workspace_bytes(h, 0) == 0
        L.effocr_yolo11_set_option(h, b"direct_stem", 0)                    # the im2col rows exist only on the cross-check path
        assert L.effocr_yolo11_workspace_bytes(h, 16) == ws[scale] + 16 * 320 * 320 * 32 * 4
        L.effocr_yolo11_destroy(h)
    assert ws["n"] < ws["s"] < ws["m"] < ws["l"] < ws["x"]
    assert wb["n"] < wb["s"] < wb["m"] < wb["l"] < wb["x"]


def test_cabi_refusals():
    L = _lib.yolo11_lib()
    for bad in (b"yolov11n", b"yolo11n-seg", b"yolo11n-pose", b"yolo11n-obb", b"yolo11n-cls", b"yolo12n", b"yolo12s", b"yolov8s", b"yolov5s", b"yolo11",
                b"", b"yolo11z"):
        rc, h = _handle(L, bad, 2)
        assert rc == -2 and not h.value, bad
        assert b"unsupported architecture" in L.effocr_yolo11_last_error()
    for nc, hh, ww in ((0, 640, 640), (81, 640, 640), (2, 0, 640), (2, 640, 650), (2, -32, 64)):
        rc, h = _handle(L, b"yolo11s", nc, hh, ww)
        assert rc == -1 and not h.value, (nc, hh, ww)
    rc, h = _handle(L, b"yolo11n", 2, 64, 64)
    assert rc == 0
    try:
        one = (ctypes.c_float * 1)(0.0)
        assert L.effocr_yolo11_set_param(h, b"model.22.dfl.conv.weight", one, 1) == -1
        assert L.effocr_yolo11_set_param(h, b"model.23.dfl.conv.weight", one, 1) == -1
        assert b"expects 16 elements" in L.effocr_yolo11_last_error()
        assert L.effocr_yolo11_set_option(h, b"no_such_option", 1) == -1
        assert L.effocr_yolo11_set_option(h, b"call_size_invariant", 2) == -1
        assert L.effocr_yolo11_upload(h, ctypes.c_void_p(256), 1 << 40) == -5   # parameters never set: refused before any copy
    finally:
        L.effocr_yolo11_destroy(h)


def test_cabi_token_cap():
    """1600 tokens (1280 x 1280, or any shape with as many stride-32 pixels) build; one row of tokens more is EUNSUPPORTED, from create and
    from the attention entry point (before anything is launched)."""
    L = _lib.yolo11_lib()
    assert _lib.YOLO11_MAX_TOKENS == 1600
    for hh, ww in ((1280, 1280), (640, 2560)):
        rc, h = _handle(L, b"yolo11n", 2, hh, ww)
        assert rc == 0
        L.effocr_yolo11_destroy(h)
    rc, h = _handle(L, b"yolo11n", 2, 1312, 1280)
    assert rc == -2 and not h.value and b"1640 tokens" in L.effocr_yolo11_last_error()
    assert L.effocr_yolo11_op_attention(None, 1, 41, 40, 2, None, None) == -2


def test_library_exports_its_header_and_nothing_of_the_other_libraries():
    src = open(os.path.join(ROOT, "include", "effocr_yolo11.h")).read()
    declared = sorted(set(re.findall(r"\b(effocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert len(declared) == 17
    assert sorted(_lib.YOLO11_EXPORTS) == declared
    v = int(re.search(r"#define\s+EFFOCR_YOLO11_ABI_VERSION\s+(\d+)", src).group(1))
    assert _lib.yolo11_lib().effocr_yolo11_abi_version() == v == _lib.YOLO11_ABI_VERSION == 1
    assert int(re.search(r"#define\s+EFFOCR_YOLO11_MAX_TOKENS\s+(\d+)", src).group(1)) == _lib.YOLO11_MAX_TOKENS
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.YOLO11_SO_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in nm.splitlines()) == declared
    _lib.lib()
    assert not set(declared) & set(_lib.EXPORTS) and not set(declared) & set(_lib.YOLOV8_EXPORTS)
    raw = ctypes.CDLL(_lib.YOLO11_SO_PATH)
    for hidden in ("effocr_abi_version", "effocr_localizer_create", "effocr_nms", "effocr_letterbox", "effocr_yolov8_create", "effocr_yolov8_forward"):
        assert not hasattr(raw, hidden), hidden
    assert not hasattr(ctypes.CDLL(_lib.SO_PATH), "effocr_yolo11_create")
    # and the YOLOv8 library still has exactly its 17 exports (15 + its two test entry points)
    nm8 = subprocess.run(["nm", "-D", "--defined-only", _lib.YOLOV8_SO_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in nm8.splitlines()) == sorted(_lib.YOLOV8_EXPORTS) and len(_lib.YOLOV8_EXPORTS) == 17
