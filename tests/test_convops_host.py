"""The operator parity tests must be able to fail (no GPU needed): the test-only library loads and refuses what it must before any
launch; the comparison functions tests/test_gpu_convops.py uses reject the float64 reference corrupted the way a kernel could be wrong,
for every real-valued geometry; and the exact-data premise holds (fp32 accumulation of the integer data is exact in any order)."""

import ctypes
import dataclasses
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests import convops_lib as CL
from tests import convops_ref as R

CUS = 256                                                  # the MI355X's CU count, for the dispatch-window geometries
CONV2D = R.conv2d_cases() + [c for c, _ in R.dispatch_cases(CUS)] + R.splitk_cases()
CONV16 = R.conv16_cases()
DUMMY = ctypes.c_void_p(256)                               # never dereferenced: every call below is refused before a launch


def test_library_loads_and_exports_every_wrapper():
    L = CL.lib()
    assert L.effocr_convops_abi_version() == CL.ABI_VERSION
    raw = ctypes.CDLL(CL.SO_PATH)
    for name in CL.EXPORTS:
        assert hasattr(raw, name), f"{name} is not exported"
    assert len(CL.EXPORTS) == 32                           # 22 + the nine effocr_convops_vit_* of the ViT path + effocr_convops_yolo_decode
    out = subprocess.run(["nm", "-D", "--defined-only", CL.SO_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert sorted(l.split()[-1] for l in out.splitlines() if " T " in l) == CL.EXPORTS      # no other function leaves the library
    assert CL.last_dispatch() == (0, 0) and CL.patch_last_dispatch() == (0, 0) and CL.qkv_attn_last_dispatch() == []


def _conv2d(L, Cin=32, Cout=32, sl=(0, 0, 0, 0, 0, 0), relu=0, silu=0):
    return L.effocr_convops_conv2d(DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 1, 4, 4, Cin, Cout, 3, 3, 1, 1, 4, 4, relu, *sl, silu, None, 0, None, None)


def test_refusals_before_any_launch():
    L = CL.lib()
    assert _conv2d(L, Cin=48) == CL.EUNSUPPORTED and "Cin" in CL.last_error()
    assert _conv2d(L, Cout=30, sl=(32, 0, 32, 0, 32, 0)) == CL.EUNSUPPORTED and "Cout" in CL.last_error()
    assert _conv2d(L, Cout=30) == CL.EUNSUPPORTED          # dense: the channel count is the stride
    for i in range(6):                                     # each stride and offset on its own: a multiple of 2 that is not one of 4
        sl = [64, 0, 64, 0, 64, 0]
        sl[i] += 2
        assert _conv2d(L, sl=tuple(sl)) == CL.EUNSUPPORTED and "multiples of 4" in CL.last_error(), i
    assert _conv2d(L, relu=1, silu=1) == CL.EINVAL
    assert _conv2d(L, sl=(64, 36, 0, 0, 0, 0)) == CL.EINVAL                                # a slice outside its row
    assert CL.last_dispatch() == (0, 0)                                                    # nothing was dispatched
    c16 = lambda prec, ci, co: L.effocr_convops_conv16(prec, DUMMY, DUMMY, DUMMY, None, DUMMY, 1, 4, 4, ci, co, 3, 3, 1, 1, 4, 4, 1, None)
    assert c16(CL.PREC_FP16, 32, 64) == CL.EUNSUPPORTED and c16(CL.PREC_BF16, 64, 96) == CL.EUNSUPPORTED
    assert c16(CL.PREC_FP32, 64, 64) == CL.EINVAL
    assert L.effocr_convops_avgpool(DUMMY, DUMMY, 1, 4, 516, 0, None) == CL.EUNSUPPORTED and "512" in CL.last_error()
    assert L.effocr_convops_avgpool16(CL.PREC_FP16, DUMMY, DUMMY, 1, 4, 4096, 0, None, None) == CL.EUNSUPPORTED
    assert L.effocr_convops_avgpool16(CL.PREC_FP16, DUMMY, DUMMY, 1, 4, 384, 0, None, None) == CL.EUNSUPPORTED
    assert L.effocr_convops_maxpool3x3s2(DUMMY, DUMMY, 1, 4, 4, 6, 2, 2, None) == CL.EUNSUPPORTED
    assert L.effocr_convops_maxpool16(CL.PREC_BF16, DUMMY, DUMMY, 1, 4, 4, 12, 2, 2, None) == CL.EUNSUPPORTED
    assert L.effocr_convops_maxpool5(DUMMY, 6, 0, DUMMY, 8, 0, 1, 4, 4, 4, None) == CL.EUNSUPPORTED
    assert L.effocr_convops_upsample2x(DUMMY, 8, 2, DUMMY, 8, 0, 1, 4, 4, 4, None) == CL.EUNSUPPORTED
    assert L.effocr_convops_im2col_nchw(DUMMY, DUMMY, 1, 3, 8, 8, 6, 6, 2, 2, 4, 4, 96, None) == CL.EINVAL      # kpad < 108 taps
    assert L.effocr_convops_stem6x6s2(DUMMY, DUMMY, 96, None, DUMMY, DUMMY, 1, 8, 8, 4, 4, 32, 0, 1, None) == CL.EINVAL
    assert L.effocr_convops_stem6x6s2_g16(DUMMY, DUMMY, 32, DUMMY, DUMMY, 1, 8, 12, 4, 6, 32, 0, 16, 32, None) == CL.EINVAL   # OW % 4
    assert L.effocr_convops_conv2d(None, DUMMY, DUMMY, None, DUMMY, 1, 4, 4, 32, 32, 3, 3, 1, 1, 4, 4, 0, 0, 0, 0, 0, 0, 0, 0, None, 0, None, None) == CL.EINVAL


def test_product_libraries_do_not_export_the_operators():
    import os
    for so in ("libeffocr_hip.so", "libeffocr_hip_ab.so", "libeffocr_resnet.so"):
        with open(os.path.join(CL.ROOT, "effocr_amd", so), "rb") as f:
            assert b"effocr_convops" not in f.read(), so


def _operands(kind):
    return {"fp32": None, "w16": torch.bfloat16, "bf16": torch.bfloat16, "f16": torch.float16}[kind]


def _mutants_rejected(case, operand, out_dtype, only=None):
    x, w, bias, resid = R.conv_data(case, "real")
    if out_dtype != torch.float32 and resid is not None:
        resid = R.round_to(resid, out_dtype)               # conv16 reads its residual in the operand type
    y, _ = R.conv_reference(case, x, w, bias, resid, operand)
    bound = R.conv_bound(case, x, w, bias, resid, operand, out_dtype)
    # the comparison accepts a correct kernel: the reference itself rounded once to the output type ...
    assert R.check_bound(y.to(out_dtype), y, bound, case.name) <= 1.0
    if operand is None:                                    # ... and an independent fp32 implementation (torch's CPU convolution)
        got = F.conv2d(x, w, bias, case.stride, case.pad)
        if case.silu:
            got = got * torch.sigmoid(got)
        if resid is not None:
            got = got + resid
        if case.relu:
            got = F.relu(got)
        R.check_bound(got, y, bound, case.name + " (torch fp32)")
    muts = R.conv_mutants(case, x, w, bias, resid, operand)
    assert {"border_tap_dropped", "pad_off_by_one"} <= set(muts)
    if out_dtype != torch.float32 and only is None:
        # A 16-bit output's own half ulp (relative to |y|) is of the order of the operand rounding's effect on y, so behind a residual
        # add and a ReLU few outputs are small enough to tell the two apart; and the worst-case term gamma_K sum|x||w| grows with K while
        # the operand rounding's effect grows with sqrt(K).  That mutant is judged on the same map, kernel and stride without the residual
        # and the ReLU (outputs near a sign change carry a small bound) and with 64 input channels (the shortest K of this kernel).
        muts.pop("operand_rounding_left_out")
        _mutants_rejected(dataclasses.replace(case, act="none", Cin=64), operand, out_dtype, only="operand_rounding_left_out")
    for name, ym in muts.items():
        if only is not None and name != only:
            continue
        with pytest.raises(R.Mismatch):
            R.check_bound(ym.to(out_dtype), y, bound, f"{case.name}/{name}")
    return set(muts)


@pytest.mark.parametrize("kind", ["fp32", "w16"])
@pytest.mark.parametrize("case", CONV2D, ids=lambda c: c.name)
def test_conv2d_comparison_rejects_every_mutant(case, kind):
    _mutants_rejected(case, _operands(kind), torch.float32)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("case", CONV16, ids=lambda c: c.name)
def test_conv16_comparison_rejects_every_mutant(case, kind):
    dt = _operands(kind)
    _mutants_rejected(case, dt, dt)


def test_every_mutation_is_exercised():
    seen = set()
    for case in CONV2D:
        x, w, bias, resid = R.conv_data(case, "real")
        seen |= set(R.conv_mutants(case, x, w, bias, resid, torch.bfloat16))
    assert seen == {"border_tap_dropped", "pad_off_by_one", "ky_kx_swapped", "last_k_stage_skipped", "residual_slice_shifted_4",
                    "relu_before_add", "last_pixel_copied", "operand_rounding_left_out"}


def test_exact_comparison_rejects_one_wrong_element():
    case = CONV2D[0]
    x, w, bias, resid = R.conv_data(case, "exact")
    y, _ = R.conv_reference(case, x, w, bias, resid)
    got = y.float()
    R.check_exact(got, y)
    got[0, 1, 2, 3] += 1.0
    with pytest.raises(R.Mismatch):
        R.check_exact(got, y)
    with pytest.raises(R.Mismatch):
        R.check_exact(torch.full_like(got, float("nan")), y)


@pytest.mark.parametrize("case", CONV2D + CONV16, ids=lambda c: c.name)
def test_exact_data_premise(case):
    """On the integer data torch's fp32 CPU convolution (another summation order) equals the float64 one bit for bit, the 2^24 headroom
    holds, and so does the 16-bit operand rounding (the integers are representable in bf16 and f16)."""
    if case.silu:
        return                                             # SiLU cases have no exact form
    x, w, bias, resid = R.conv_data(case, "exact")
    for t in (x, w, bias) + ((resid,) if resid is not None else ()):
        assert torch.equal(t, t.to(torch.bfloat16).float()) and torch.equal(t, t.half().float()) and torch.equal(t, t.round())
    y, sabs = R.conv_reference(case, x, w, bias, resid)
    R.assert_exact_premise(sabs, bias, resid)
    got = F.conv2d(x, w, bias, case.stride, case.pad)
    if resid is not None:
        got = got + resid
    if case.relu:
        got = F.relu(got)
    R.check_exact(got, y, case.name)
    assert torch.equal(y, y.round())


def test_unfold_reference_matches_a_convolution():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, 9, 11, generator=g).double()
    w = torch.randn(5, 3, 7, 7, generator=g).double()
    rows = R.unfold_ref(x, 7, 2, 3, 160)
    assert torch.equal(rows[:, 147:], torch.zeros(rows.shape[0], 13, dtype=rows.dtype))
    y = rows[:, :147] @ R.pack_w(w).t()
    ref = F.conv2d(x, w, None, 2, 3).permute(0, 2, 3, 1).reshape(-1, 5)
    torch.testing.assert_close(y, ref, rtol=1e-12, atol=1e-12)
