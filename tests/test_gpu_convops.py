"""Operator parity of the convolution, pooling and data-movement kernels on the MI355X (-m gpu): each launcher of resnet.hip,
resnet16.hip and yolo.hip on its own, through the test-only library (tests/convops_lib.py), against float64 torch on the CPU.

Every geometry runs on two kinds of data (tests/convops_ref.py): integers, where the kernel must equal the float64 result cast to the
output type BIT FOR BIT, and real values, where every output element must lie within a bound derived from the arithmetic.  Every call
writes into a buffer pre-filled with a sentinel (the channels outside the output slice and a guard row after the last pixel must keep
it), must leave its inputs unchanged, and the convolution tests assert the kernel variant the dispatcher chose (last_dispatch).
tests/test_convops_host.py shows on the CPU that these comparisons reject wrong kernels.  Each test prints its largest error / bound."""

import math

import pytest
import torch
import torch.nn.functional as F

from effocr_amd import _lib
from tests import convops_lib as CL
from tests import convops_ref as R

pytestmark = pytest.mark.gpu

SENT = 24576.0                                             # representable in fp32, bf16 and f16; far from every test value
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
PREC = {BF16: CL.PREC_BF16, F16: CL.PREC_FP16, F32: CL.PREC_FP32}
_RATIOS = {}


def _record(op, ratio):
    _RATIOS[op] = max(_RATIOS.get(op, 0.0), ratio)
    print(f"[convops] {op}: largest error / bound {ratio:.3f} (largest so far for this operator {_RATIOS[op]:.3f})")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _unchanged(dev_t, host_t, what):
    assert torch.equal(_bits(dev_t.cpu()), _bits(host_t)), f"{what} was modified by the call"


def _ok(rc):
    assert rc == 0, f"rc {rc}: {CL.last_error()}"


def _sliced(t, ld, off, g):
    """NHWC [..., C] -> [..., ld] with the tensor in channels off .. off + C and other data around it (ld = 0: dense)."""
    if ld == 0:
        return t.contiguous()
    buf = torch.randint(-3, 4, t.shape[:-1] + (ld,), generator=g).to(t.dtype)
    buf[..., off:off + t.shape[-1]] = t
    return buf


def _out_buffer(M, ld, dtype, dev):
    return torch.full((M + 1, ld), SENT, dtype=dtype, device=dev)          # one guard row after the last pixel


def _take(out, M, off, C, what):
    """The result slice of a sentinel-filled output [M + 1, ld]; everything around it must still hold the sentinel."""
    o = out.cpu()
    assert bool((o[M] == SENT).all()), f"{what}: wrote past the last pixel"
    assert bool((o[:M, :off] == SENT).all()) and bool((o[:M, off + C:] == SENT).all()), f"{what}: wrote outside its channel slice"
    return o[:M, off:off + C].contiguous()


def _stream(dev):
    return _lib.current_stream(dev)


# ---------------------------------------------------------------------------------------------------------------------------------
# conv2d_nhwc (resnet.hip): fp32 operands and bf16 operands (w16)

_CACHE = {}


def _conv_ref(case, kind, operand, out_dtype=F32, mod=None):
    """(x, w, bias, resid, y float64, bound or sabs) once per geometry, data kind and operand type (the float64 references are the slow part)."""
    key = (case, kind, operand, out_dtype, mod)
    if key not in _CACHE:
        x, w, bias, resid = R.conv_data(case, kind)
        if out_dtype != F32 and resid is not None:
            resid = R.round_to(resid, out_dtype)
        if mod is not None:
            x = x.clone()
            for (idx, val) in mod:
                x[idx] = val
        y, sabs = R.conv_reference(case, x, w, bias, resid, operand)
        if kind == "exact":
            R.assert_exact_premise(sabs, bias, resid)
            aux = sabs
        else:
            aux = R.conv_bound(case, x, w, bias, resid, operand, out_dtype) if mod is None else None
        _CACHE[key] = (x, w, bias, resid, y, aux)
    return _CACHE[key]


def _run_conv2d(dev, case, x, w, bias, resid, w16, partial_bytes=0):
    """One effocr_convops_conv2d call -> (result [B,Cout,OH,OW] fp32 on the CPU, (nw, ksplit))."""
    L = CL.lib()
    g = torch.Generator().manual_seed(7)
    in_ld, in_off, out_ld, out_off, res_ld, res_off = case.slices()
    xin = _sliced(R.to_nhwc(x), in_ld, in_off, g)
    rin = _sliced(R.to_nhwc(resid), res_ld, res_off, g) if resid is not None else None
    d_x, d_r = xin.to(dev), (rin.to(dev) if rin is not None else None)
    d_w = R.pack_w(w).to(dev)
    d_w16 = R.pack_w16(w).to(dev) if w16 else None
    d_b = bias.to(dev)
    M = case.M
    out = _out_buffer(M, out_ld or case.Cout, F32, dev)
    part = None
    if partial_bytes:
        part = torch.full((partial_bytes // 4 + 64,), SENT, device=dev)
    rc = L.effocr_convops_conv2d(CL.ptr(d_x), CL.ptr(d_w), CL.ptr(d_b), CL.ptr(d_r), CL.ptr(out), case.B, case.H, case.W, case.Cin, case.Cout,
                                 case.k, case.k, case.stride, case.pad, case.OH, case.OW, int(case.relu), in_ld, in_off, out_ld, out_off,
                                 res_ld, res_off, int(case.silu), CL.ptr(part), partial_bytes, CL.ptr(d_w16), _stream(dev))
    _ok(rc)
    disp = CL.last_dispatch()
    torch.cuda.synchronize(dev)
    _unchanged(d_x, xin, "the input")
    if rin is not None:
        _unchanged(d_r, rin, "the residual")
    if part is not None:
        assert bool((part[-64:].cpu() == SENT).all()), "wrote past the split-K scratch"
    got = _take(out, M, out_off, case.Cout, case.name)
    return got.reshape(case.B, case.OH, case.OW, case.Cout).permute(0, 3, 1, 2).contiguous(), disp


def _tile_by_cout(cout):
    return 32 if cout <= 32 else (64 if cout <= 64 else 128)


def _check_conv2d(dev, case, w16, expect_nw, op):
    operand = BF16 if w16 else None
    for kind in ("exact", "real"):
        if kind == "exact" and case.silu:
            continue
        x, w, bias, resid, y, aux = _conv_ref(case, kind, operand)
        got, (nw, ks) = _run_conv2d(dev, case, x, w, bias, resid, w16)
        assert (nw, ks) == (expect_nw, 1), f"{case.name}: dispatched tile {nw}, split {ks}; meant {expect_nw}, 1"
        if kind == "exact":
            R.check_exact(got, y, f"{case.name} {op} exact")
        else:
            _record(op, R.check_bound(got, y, aux, f"{case.name} {op} real"))


@pytest.mark.parametrize("w16", [False, True], ids=["fp32", "w16"])
@pytest.mark.parametrize("case", R.conv2d_cases(), ids=lambda c: c.name)
def test_conv2d(dev, case, w16):
    cus = CL.lib().effocr_convops_device_cus()
    nw = _tile_by_cout(case.Cout)
    tiles = -(-case.M // 128) * -(-case.Cout // nw)
    assert tiles * 2 <= cus, "the geometry must lie below the 128 -> 64 switch window"
    _check_conv2d(dev, case, w16, nw, "conv2d w16" if w16 else "conv2d fp32")


@pytest.mark.parametrize("w16", [False, True], ids=["fp32", "w16"])
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["half_round", "half_round_plus_1", "full_round", "full_round_plus_1"])
def test_conv2d_tile_switch_window(dev, which, w16):
    """128-channel layers of cus/2, cus/2 + 1, cus and cus + 1 pixel tiles: 128-wide tiles outside (cus/2, cus], 64-wide inside."""
    cus = CL.lib().effocr_convops_device_cus()
    assert cus >= 16
    case, nw = R.dispatch_cases(cus)[which]
    _check_conv2d(dev, case, w16, nw, "conv2d w16" if w16 else "conv2d fp32")


def _expected_split(case, w16, cus, partial_bytes):
    nw = _tile_by_cout(case.Cout)
    grid = -(-case.M // 128) * -(-case.Cout // nw)
    nks = -(-case.K // 64) if w16 else case.K // 32
    sp = min(cus // grid, nks // 2, 32)
    while sp > 1 and sp * case.M * case.Cout * 4 > partial_bytes:
        sp -= 1
    return nw, sp, nks


@pytest.mark.parametrize("w16", [False, True], ids=["fp32", "w16"])
@pytest.mark.parametrize("case", R.splitk_cases(), ids=lambda c: c.name)
def test_conv2d_split_k(dev, case, w16):
    """Few tiles and a long K: with scratch the launch splits K (partial sums + conv_reduce_kernel), with a small scratch it splits less,
    without scratch it does not split; every form within the bound, and on the integer data all three bit-equal."""
    cus = CL.lib().effocr_convops_device_cus()
    operand = BF16 if w16 else None
    op = "conv2d split-K w16" if w16 else "conv2d split-K fp32"
    full = 32 * case.M * case.Cout * 4
    small = 5 * case.M * case.Cout * 4
    nw, sp_full, nks = _expected_split(case, w16, cus, full)
    _, sp_small, _ = _expected_split(case, w16, cus, small)
    assert sp_full > sp_small > 1 and (nks % sp_full != 0 or nks % sp_small != 0), "the case must split, split less, and split unevenly"
    for kind in ("exact", "real"):
        if kind == "exact" and case.silu:
            continue
        x, w, bias, resid, y, aux = _conv_ref(case, kind, operand)
        outs = []
        for pb, sp in ((0, 1), (full, sp_full), (small, sp_small)):
            got, disp = _run_conv2d(dev, case, x, w, bias, resid, w16, partial_bytes=pb)
            assert disp == (nw, sp), f"{case.name}: dispatched {disp}, meant {(nw, sp)}"
            if kind == "exact":
                R.check_exact(got, y, f"{case.name} {op} split {sp} exact")
            else:
                _record(op, R.check_bound(got, y, aux, f"{case.name} {op} split {sp} real"))
            outs.append(got)
        if kind == "exact":
            assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))


def test_conv2d_refusals_on_device(dev):
    """Refusals stay refusals with real buffers: the error code, no launch, the output untouched."""
    L = CL.lib()
    out = _out_buffer(16, 64, F32, dev)
    buf = torch.zeros(16 * 9 * 64, device=dev)
    call = lambda Cin, Cout, sl: L.effocr_convops_conv2d(CL.ptr(buf), CL.ptr(buf), CL.ptr(buf), None, CL.ptr(out), 1, 4, 4, Cin, Cout, 3, 3, 1, 1, 4, 4, 1,
                                                         *sl, 0, None, 0, None, _stream(dev))
    assert call(48, 32, (64, 0, 64, 0, 0, 0)) == CL.EUNSUPPORTED
    assert call(32, 30, (64, 0, 64, 0, 0, 0)) == CL.EUNSUPPORTED
    assert call(32, 32, (62, 0, 64, 0, 0, 0)) == CL.EUNSUPPORTED
    assert call(32, 32, (64, 2, 64, 0, 0, 0)) == CL.EUNSUPPORTED
    assert call(32, 32, (64, 0, 64, 6, 0, 0)) == CL.EUNSUPPORTED
    assert CL.last_dispatch() == (0, 0)
    torch.cuda.synchronize(dev)
    assert bool((out.cpu() == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# rn_conv16 (resnet16.hip): f16 and bf16 operands and outputs

def _run_conv16(dev, case, dtype, x, w, bias, resid):
    L = CL.lib()
    xin = R.to_nhwc(x).to(dtype)
    rin = R.to_nhwc(resid).to(dtype) if resid is not None else None
    d_x, d_r = xin.to(dev), (rin.to(dev) if rin is not None else None)
    d_w = R.pack_w(w).to(dtype).to(dev)
    d_b = bias.to(dev)
    out = _out_buffer(case.M, case.Cout, dtype, dev)
    rc = L.effocr_convops_conv16(PREC[dtype], CL.ptr(d_x), CL.ptr(d_w), CL.ptr(d_b), CL.ptr(d_r), CL.ptr(out), case.B, case.H, case.W, case.Cin,
                                 case.Cout, case.k, case.k, case.stride, case.pad, case.OH, case.OW, int(case.relu), _stream(dev))
    _ok(rc)
    torch.cuda.synchronize(dev)
    _unchanged(d_x, xin, "the input")
    if rin is not None:
        _unchanged(d_r, rin, "the residual")
    got = _take(out, case.M, 0, case.Cout, case.name)
    return got.reshape(case.B, case.OH, case.OW, case.Cout).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", R.conv16_cases(), ids=lambda c: c.name)
def test_conv16(dev, case, dtype):
    op = "conv16 " + ("f16" if dtype == F16 else "bf16")
    for kind in ("exact", "real"):
        x, w, bias, resid, y, aux = _conv_ref(case, kind, dtype, dtype)
        got = _run_conv16(dev, case, dtype, x, w, bias, resid)
        if kind == "exact":
            R.check_exact(got, y, f"{case.name} {op} exact")
        else:
            _record(op, R.check_bound(got, y, aux, f"{case.name} {op} real"))


def test_conv16_f16_overflow_is_inf(dev):
    """An exact sum beyond f16's 65504 must come out as inf, as .to(float16) gives, not wrapped or clamped (64 * 2 * 576 = 73728)."""
    case = R.ConvCase("f16_overflow", 1, 5, 5, 64, 64, 3, 1, 1, "none")
    x = torch.full((1, 64, 5, 5), 64.0)
    w = torch.full((64, 64, 3, 3), 2.0)
    w[1::2] = -2.0
    w[2::4] = 1.0
    bias = torch.zeros(64)
    y, sabs = R.conv_reference(case, x, w, bias, None, F16)
    R.assert_exact_premise(sabs)
    want = y.to(F16)
    assert bool((want == float("inf")).any()) and bool((want == float("-inf")).any()) and bool(want.isfinite().any())
    R.check_exact(_run_conv16(dev, case, F16, x, w, bias, None), y, "f16 overflow")


# ---------------------------------------------------------------------------------------------------------------------------------
# NaN and infinity: a non-finite input element reaches exactly the outputs whose window covers it, as in torch

def _nonfinite_check(got, y_mod, bound, what):
    """Where torch's result is non-finite the kernel's is the same value; everywhere else it is within the bound (that of the clean data:
    an output whose window does not cover the element is the clean one, one that -inf and a ReLU turn into 0 is exact)."""
    want = y_mod.to(got.dtype)
    bad = ~want.isfinite()
    assert bool(bad.any()) and not bool(bad.all())
    same = (got == want) | (got.isnan() & want.isnan())
    if not bool(same[bad].all()):
        i = tuple((bad & ~same).nonzero()[0].tolist())
        raise R.Mismatch(f"{what}: {int((bad & ~same).sum())} of {int(bad.sum())} non-finite outputs differ from torch; first at {i}: "
                         f"got {got[i].item()!r}, want {want[i].item()!r}")
    zero = torch.zeros_like(y_mod)
    R.check_bound(torch.where(bad, zero.to(got.dtype), got), torch.where(bad, zero, y_mod), bound, what + " (finite part)")


def _mods(case, what):
    mid = (0, 1, case.H // 2, case.W // 2)
    if what == "nan_first":                                # element 0: the address the masked taps of resnet.hip's stage loader read
        return (((0, 0, 0, 0), float("nan")),)
    if what == "nan_mid":
        return ((mid, float("nan")),)
    return ((mid, float("inf")), ((case.B - 1, 2, 0, case.W - 1), float("-inf")))


NONFINITE = ["nan_first", "nan_mid", "inf"]
NAN_CASES = [R.ConvCase("nf_relu", 2, 7, 7, 32, 36, 3, 1, 1, "relu"), R.ConvCase("nf_res_relu", 2, 7, 7, 64, 68, 3, 2, 1, "res_relu", True),
             R.ConvCase("nf_none", 2, 5, 12, 32, 132, 3, 1, 1, "none")]


@pytest.mark.parametrize("what", NONFINITE)
@pytest.mark.parametrize("w16", [False, True], ids=["fp32", "w16"])
@pytest.mark.parametrize("case", NAN_CASES, ids=lambda c: c.name)
def test_conv2d_nonfinite_input(dev, case, w16, what):
    operand = BF16 if w16 else None
    _, w, bias, resid, _, bound = _conv_ref(case, "real", operand)
    xm, _, _, _, y_mod, _ = _conv_ref(case, "real", operand, mod=_mods(case, what))
    got, _ = _run_conv2d(dev, case, xm, w, bias, resid, w16)
    _nonfinite_check(got, y_mod, bound, f"{case.name} {what}")


@pytest.mark.parametrize("what", NONFINITE)
@pytest.mark.parametrize("w16", [False, True], ids=["fp32", "w16"])
def test_conv2d_split_k_nonfinite_input(dev, w16, what):
    """The same through the split-K partial sums and the reduction kernel's ReLU."""
    case = R.splitk_cases()[0]
    operand = BF16 if w16 else None
    _, w, bias, resid, _, bound = _conv_ref(case, "real", operand)
    xm, _, _, _, y_mod, _ = _conv_ref(case, "real", operand, mod=_mods(case, what))
    got, (nw, ks) = _run_conv2d(dev, case, xm, w, bias, resid, w16, partial_bytes=32 * case.M * case.Cout * 4)
    assert ks > 1
    _nonfinite_check(got, y_mod, bound, f"{case.name} {what} split {ks}")


@pytest.mark.parametrize("what", NONFINITE)
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("act", ["relu", "res_relu"])
def test_conv16_nonfinite_input(dev, act, dtype, what):
    case = R.ConvCase("nf16_" + act, 2, 7, 7, 64, 64, 3, 1, 1, act)
    _, w, bias, resid, _, bound = _conv_ref(case, "real", dtype, dtype)
    xm, _, _, _, y_mod, _ = _conv_ref(case, "real", dtype, dtype, mod=_mods(case, what))
    got = _run_conv16(dev, case, dtype, xm, w, bias, resid)
    _nonfinite_check(got, y_mod, bound, f"{case.name} {what}")


# ---------------------------------------------------------------------------------------------------------------------------------
# pools and upsample

def _pool_data(B, C, H, W, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-40, 41, (B, C, H, W), generator=g).float() * 0.25          # representable in bf16 and f16
    if kind == "negative":                                 # the padding (-inf in the kernel, implicit in torch) must never win
        x = -x.abs() - 1.0
    elif kind == "neg_inf":
        x[:, :, ::2, :] = float("-inf")
        x[0, :, :, :] = float("-inf")
    elif kind == "nan":
        x[0, 1 % C, H // 2, W // 2] = float("nan")
        x[B - 1, 0, 0, 0] = float("nan")
    elif kind == "inf":
        x[0, 1 % C, H // 2, W // 2] = float("inf")
        x[B - 1, 0, H - 1, W - 1] = float("-inf")
    return x


POOL_KINDS = ["mixed", "negative", "neg_inf", "nan", "inf"]
POOL_MAPS = [(1, 1), (2, 2), (7, 7), (8, 8), (5, 12)]


def _pool_equal(got, want, what):
    """Bit equality with torch's pool, a NaN matching a NaN."""
    R.check_exact(got, want.double(), what)
    if bool(want.isnan().any()):
        assert bool(got.isnan().any())


@pytest.mark.parametrize("kind", POOL_KINDS)
@pytest.mark.parametrize("C", [4, 8, 64])
def test_maxpool3x3s2(dev, C, kind):
    L = CL.lib()
    for (H, W) in POOL_MAPS:
        x = _pool_data(2, C, H, W, kind, 11)
        want = F.max_pool2d(x.double(), 3, 2, 1)
        OH, OW = want.shape[2:]
        xin = R.to_nhwc(x)
        d_x = xin.to(dev)
        M = 2 * OH * OW
        out = _out_buffer(M, C, F32, dev)
        _ok(L.effocr_convops_maxpool3x3s2(CL.ptr(d_x), CL.ptr(out), 2, H, W, C, OH, OW, _stream(dev)))
        torch.cuda.synchronize(dev)
        _unchanged(d_x, xin, "the input")
        got = _take(out, M, 0, C, "maxpool3x3s2").reshape(2, OH, OW, C).permute(0, 3, 1, 2)
        _pool_equal(got, want, f"maxpool3x3s2 {H}x{W} C={C} {kind}")


@pytest.mark.parametrize("kind", POOL_KINDS)
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("C", [8, 64])
def test_maxpool16(dev, C, dtype, kind):
    L = CL.lib()
    for (H, W) in POOL_MAPS:
        x = _pool_data(2, C, H, W, kind, 12)
        want = F.max_pool2d(x.double(), 3, 2, 1)
        OH, OW = want.shape[2:]
        xin = R.to_nhwc(x).to(dtype)
        d_x = xin.to(dev)
        M = 2 * OH * OW
        out = _out_buffer(M, C, dtype, dev)
        _ok(L.effocr_convops_maxpool16(PREC[dtype], CL.ptr(d_x), CL.ptr(out), 2, H, W, C, OH, OW, _stream(dev)))
        torch.cuda.synchronize(dev)
        _unchanged(d_x, xin, "the input")
        got = _take(out, M, 0, C, "maxpool16").reshape(2, OH, OW, C).permute(0, 3, 1, 2)
        _pool_equal(got, want, f"maxpool16 {H}x{W} C={C} {kind}")


@pytest.mark.parametrize("kind", POOL_KINDS)
@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "sliced"])
@pytest.mark.parametrize("op", ["maxpool5", "upsample2x"])
def test_maxpool5_and_upsample2x(dev, op, sliced, kind):
    L = CL.lib()
    g = torch.Generator().manual_seed(5)
    for C in (4, 36):
        for (H, W) in POOL_MAPS:
            x = _pool_data(2, C, H, W, kind, 13)
            if op == "maxpool5":
                want = F.max_pool2d(x.double(), 5, 1, 2)
            else:
                want = F.interpolate(x.double(), scale_factor=2, mode="nearest")
            OH, OW = want.shape[2:]
            in_ld, in_off, out_ld, out_off = (C + 12, 4, C + 24, 20) if sliced else (C, 0, C, 0)
            xin = _sliced(R.to_nhwc(x), in_ld if sliced else 0, in_off, g)
            d_x = xin.to(dev)
            M = 2 * OH * OW
            out = _out_buffer(M, out_ld, F32, dev)
            fn = L.effocr_convops_maxpool5 if op == "maxpool5" else L.effocr_convops_upsample2x
            _ok(fn(CL.ptr(d_x), in_ld, in_off, CL.ptr(out), out_ld, out_off, 2, H, W, C, _stream(dev)))
            torch.cuda.synchronize(dev)
            _unchanged(d_x, xin, "the input")
            got = _take(out, M, out_off, C, op).reshape(2, OH, OW, C).permute(0, 3, 1, 2)
            _pool_equal(got, want, f"{op} {H}x{W} C={C} {kind}")


def _avgpool_bound(x64, l2norm):
    """x64 [B, HW, C] float64 (the values the kernel reads).  mean: HW sequential adds and one division -> gamma_HW sum|x| / HW + u |mean|.
    l2norm: ss = sum v^2 (C squares, C adds in some order, each v off by e_v), sqrt (u), one division (u):
    |out - ref| <= e_v / n + |v| / n * rel_n + u |out|, rel_n = (sum 2 |v| e_v + gamma_(C+2) ss) / (2 ss) + u.  Returns (ref, bound)."""
    B, HW, C = x64.shape
    v = x64.mean(dim=1)
    gam = HW * R.U / (1 - HW * R.U)
    e_v = gam * x64.abs().sum(dim=1) / HW + R.U * v.abs()
    if not l2norm:
        return v, e_v + 2.0 ** -149
    ss = (v * v).sum(dim=1, keepdim=True)
    n = ss.sqrt().clamp_min(1e-12)
    ref = v / n
    gc = (C + 2) * R.U / (1 - (C + 2) * R.U)
    rel_n = torch.where(ss > 0, ((2 * v.abs() * e_v).sum(dim=1, keepdim=True) + gc * ss) / (2 * ss).clamp_min(1e-300), torch.zeros_like(ss)) + R.U
    return ref, (e_v / n + ref.abs() * rel_n) * (1 + 1e-3) + R.U * ref.abs() + 2.0 ** -149


@pytest.mark.parametrize("l2norm", [0, 1])
@pytest.mark.parametrize("C", [4, 64, 260, 512])
def test_avgpool(dev, C, l2norm):
    L = CL.lib()
    g = torch.Generator().manual_seed(21)
    for HW in (1, 4, 49):
        for kind in ("exact", "real"):
            x = torch.randint(-8, 9, (3, HW, C), generator=g).float() if kind == "exact" else torch.randn(3, HW, C, generator=g)
            x[1] = 0.0                                     # an all-zero row: F.normalize's 1e-12 clamp
            d_x = x.to(dev)
            out = _out_buffer(3, C, F32, dev)
            _ok(L.effocr_convops_avgpool(CL.ptr(d_x), CL.ptr(out), 3, HW, C, l2norm, _stream(dev)))
            torch.cuda.synchronize(dev)
            _unchanged(d_x, x, "the input")
            got = _take(out, 3, 0, C, "avgpool")
            ref, bound = _avgpool_bound(x.double(), l2norm)
            assert bool((got[1] == 0).all())
            if kind == "exact" and not l2norm:
                R.check_exact(got, x.double().sum(dim=1) / HW, f"avgpool C={C} HW={HW}")
            else:
                if l2norm:
                    torch.testing.assert_close(ref, F.normalize(x.double().mean(dim=1), dim=1), rtol=1e-12, atol=1e-300)
                _record("avgpool fp32", R.check_bound(got, ref, bound, f"avgpool C={C} HW={HW} l2norm={l2norm} {kind}"))


@pytest.mark.parametrize("l2norm", [0, 1])
def test_avgpool_nonfinite_row(dev, l2norm):
    """A NaN or inf element: its channel of the mean, and with l2norm what F.normalize gives (a NaN norm is not clamped to 1e-12)."""
    L = CL.lib()
    x = torch.randn(3, 4, 64, generator=torch.Generator().manual_seed(23))
    x[0, 2, 5] = float("nan")
    x[2, 1, 7] = float("inf")
    d_x = x.to(dev)
    out = _out_buffer(3, 64, F32, dev)
    _ok(L.effocr_convops_avgpool(CL.ptr(d_x), CL.ptr(out), 3, 4, 64, l2norm, _stream(dev)))
    torch.cuda.synchronize(dev)
    got = _take(out, 3, 0, 64, "avgpool")
    want = x.double().mean(dim=1)
    if l2norm:
        want = F.normalize(want, dim=1)
    bad = ~want.isfinite()
    assert torch.equal(got.isnan(), want.isnan()) and torch.equal(got[bad & ~want.isnan()].double(), want[bad & ~want.isnan()])
    ref, bound = _avgpool_bound(x.double()[1:2], l2norm)
    R.check_bound(got[1:2], ref, bound, "avgpool, the finite row")
    if l2norm:
        assert bool((got[2][~got[2].isnan()] == 0).all())      # finite / inf


def test_avgpool_refuses_more_than_512_channels(dev):
    L = CL.lib()
    x = torch.zeros(2, 4, 516, device=dev)
    out = _out_buffer(2, 516, F32, dev)
    assert L.effocr_convops_avgpool(CL.ptr(x), CL.ptr(out), 2, 4, 516, 0, _stream(dev)) == CL.EUNSUPPORTED
    torch.cuda.synchronize(dev)
    assert bool((out.cpu() == SENT).all())


@pytest.mark.parametrize("l2norm", [0, 1])
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["fp32", "f16", "bf16"])
@pytest.mark.parametrize("C", [512, 2048])
def test_avgpool16(dev, C, dtype, l2norm):
    """rn_avgpool in all three element types; the status word is set for a non-finite row and only then."""
    L = CL.lib()
    g = torch.Generator().manual_seed(22)
    name = {F32: "fp32", F16: "f16", BF16: "bf16"}[dtype]
    for HW in (1, 4, 49):
        for kind in ("exact", "real", "inf", "nan"):
            x = torch.randint(-8, 9, (3, HW, C), generator=g).float() if kind == "exact" else torch.randn(3, HW, C, generator=g)
            x = x.to(dtype)
            if kind in ("inf", "nan"):
                x[2, HW - 1, C - 3] = float(kind)
            d_x = x.to(dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            out = _out_buffer(3, C, F32, dev)
            _ok(L.effocr_convops_avgpool16(PREC[dtype], CL.ptr(d_x), CL.ptr(out), 3, HW, C, l2norm, CL.ptr(status), _stream(dev)))
            torch.cuda.synchronize(dev)
            _unchanged(d_x, x, "the input")
            got = _take(out, 3, 0, C, "avgpool16")
            rows = 2 if kind in ("inf", "nan") else 3
            assert status.item() == (1 if rows == 2 else 0), f"status word {status.item()} for {kind} data"
            ref, bound = _avgpool_bound(x.double()[:rows], l2norm)
            if kind == "exact" and not l2norm:
                R.check_exact(got, x.double().sum(dim=1) / HW, f"avgpool16 {name} C={C} HW={HW}")
            else:
                _record(f"avgpool16 {name}", R.check_bound(got[:rows], ref, bound, f"avgpool16 {name} C={C} HW={HW} l2norm={l2norm} {kind}"))
            if rows == 2:
                want = x.double()[2].mean(dim=0)
                if l2norm:
                    want = want / (want * want).sum().sqrt().clamp_min(1e-12)
                assert torch.equal(got[2].isnan(), want.isnan()) and not bool(got[2].isfinite().all())
                fin = want.isfinite() if not l2norm else torch.zeros_like(want, dtype=torch.bool)
                assert torch.equal(got[2][~want.isnan() & ~fin], want[~want.isnan() & ~fin].float())


# ---------------------------------------------------------------------------------------------------------------------------------
# im2col

@pytest.mark.parametrize("hw", [(33, 33), (64, 96)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_im2col_conv1(dev, hw):
    L = CL.lib()
    H, W = hw
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(31))
    OH, OW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    want = R.unfold_ref(x, 7, 2, 3, 160)
    d_x = x.to(dev)
    out = _out_buffer(2 * OH * OW, 160, F32, dev)
    _ok(L.effocr_convops_im2col_conv1(CL.ptr(d_x), CL.ptr(out), 2, H, W, OH, OW, _stream(dev)))
    torch.cuda.synchronize(dev)
    _unchanged(d_x, x, "the input")
    got = _take(out, 2 * OH * OW, 0, 160, "im2col_conv1")
    assert bool((got[:, 147:] == 0).all())
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("geo", [(3, 6, 2, 2, 128), (3, 6, 2, 2, 108), (4, 3, 1, 1, 64), (3, 7, 2, 3, 160)], ids=lambda g: "c%d_k%d_s%d_p%d_kpad%d" % g)
@pytest.mark.parametrize("hw", [(33, 33), (64, 96)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_im2col_nchw(dev, hw, geo):
    L = CL.lib()
    H, W = hw
    Cin, k, s, p, kpad = geo
    x = torch.randn(2, Cin, H, W, generator=torch.Generator().manual_seed(32))
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    want = R.unfold_ref(x, k, s, p, kpad)
    assert want.shape[0] == 2 * OH * OW
    d_x = x.to(dev)
    out = _out_buffer(2 * OH * OW, kpad, F32, dev)
    _ok(L.effocr_convops_im2col_nchw(CL.ptr(d_x), CL.ptr(out), 2, Cin, H, W, k, k, s, p, OH, OW, kpad, _stream(dev)))
    torch.cuda.synchronize(dev)
    _unchanged(d_x, x, "the input")
    got = _take(out, 2 * OH * OW, 0, kpad, "im2col_nchw")
    assert bool((got[:, k * k * Cin:] == 0).all())
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("hw", [(33, 33), (64, 96)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_im2col16(dev, hw, dtype):
    """The stem rows of the 16-bit path: 192 columns, rounded exactly as .to(T) rounds (values up to +-60000 included for f16's range)."""
    L = CL.lib()
    H, W = hw
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(33))
    x[0, 0, 0, :8] = torch.tensor([65519.0, 65520.0, -65520.0, 1e-8, -1e-8, 6e-8, 2049.0, 0.33325195])   # f16: last finite, first inf, subnormals, ties
    OH, OW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    want = R.unfold_ref(x, 7, 2, 3, 192).to(dtype)
    d_x = x.to(dev)
    out = _out_buffer(2 * OH * OW, 192, dtype, dev)
    _ok(L.effocr_convops_im2col16(PREC[dtype], CL.ptr(d_x), CL.ptr(out), 2, H, W, OH, OW, _stream(dev)))
    torch.cuda.synchronize(dev)
    _unchanged(d_x, x, "the input")
    got = _take(out, 2 * OH * OW, 0, 192, "im2col16")
    assert bool((got[:, 147:] == 0).all())
    assert torch.equal(_bits(got), _bits(want))


# ---------------------------------------------------------------------------------------------------------------------------------
# YOLOv5 stems: Conv(3, c, 6, 2, 2) + bias (+ SiLU) straight from NCHW

def _stem_ref(x, w, bias, silu):
    """float64 result [B,OH,OW,C] and the bound: 108 fused multiply-adds in tap order (gamma_108 sum|x||w|), the bias add, SiLU."""
    acc = F.conv2d(x.double(), w.double(), None, 2, 2)
    sabs = F.conv2d(x.double().abs(), w.double().abs(), None, 2, 2)
    gam = 108 * R.U / (1 - 108 * R.U)
    y = acc + bias.double().view(1, -1, 1, 1)
    e = gam * sabs + R.U * y.abs()
    if silu:
        assert y.abs().max().item() + e.max().item() <= R.SILU_XMAX
        y = y * torch.sigmoid(y)
        e = R.SILU_LIP * e + R.SILU_RHO * y.abs()
    return R.to_nhwc(y), R.to_nhwc(e) + 2.0 ** -149, sabs


def _stem_data(B, H, W, cout, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "exact":
        return (torch.randint(-3, 4, (B, 3, H, W), generator=g).float(), torch.randint(-1, 2, (cout, 3, 6, 6), generator=g).float(),
                torch.randint(-4, 5, (cout,), generator=g).float())
    return (torch.randn(B, 3, H, W, generator=g), torch.randn(cout, 3, 6, 6, generator=g) * (0.6 / math.sqrt(108)), torch.randn(cout, generator=g) * 0.5)


def _run_stem(dev, x, w, bias, silu, with_wt, misalign, out_ld=48, out_off=12):
    L = CL.lib()
    B, _, H, W = x.shape
    OH, OW = (H + 4 - 6) // 2 + 1, (W + 4 - 6) // 2 + 1
    rows = torch.zeros(32, 128)
    rows[:, :108] = R.pack_w(w)                            # [co][(ky*6 + kx)*3 + c], row stride 128
    d_w, d_wt, d_b = rows.to(dev), (R.pack_w(w).t().contiguous().to(dev) if with_wt else None), bias.to(dev)
    flat = torch.zeros(x.numel() + 2, device=dev)          # torch allocations are 256-byte aligned: + 1 element = a 4-byte offset
    d_x = flat[1:1 + x.numel()] if misalign else flat[:x.numel()]
    d_x.copy_(x.reshape(-1))
    assert d_x.data_ptr() % 8 == (4 if misalign else 0)
    out = _out_buffer(B * OH * OW, out_ld, F32, dev)
    _ok(L.effocr_convops_stem6x6s2(CL.ptr(d_x), CL.ptr(d_w), 128, CL.ptr(d_wt), CL.ptr(d_b), CL.ptr(out), B, H, W, OH, OW, out_ld, out_off, silu, _stream(dev)))
    torch.cuda.synchronize(dev)
    assert torch.equal(_bits(d_x.cpu()), _bits(x.reshape(-1))), "the input was modified by the call"
    return _take(out, B * OH * OW, out_off, 32, "stem6x6s2").reshape(B, OH, OW, 32)


@pytest.mark.parametrize("hw", [(16, 24), (18, 40), (17, 23), (6, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_stem6x6s2(dev, hw):
    """With the transposed weights, an even W and an 8-byte aligned input the scalar-weight kernel runs; without them, with an odd W or
    with an input 4 bytes off that alignment the LDS-weight kernel does.  Both against float64, and bit for bit against each other."""
    H, W = hw
    for kind, silu in (("exact", 0), ("real", 0), ("real", 1)):
        x, w, bias = _stem_data(2, H, W, 32, kind, 41)
        y, bound, sabs = _stem_ref(x, w, bias, silu)
        outs = [_run_stem(dev, x, w, bias, silu, with_wt, mis) for with_wt, mis in ((True, False), (False, False), (True, True))]
        for got in outs:
            if kind == "exact":
                R.assert_exact_premise(sabs, bias)
                R.check_exact(got, y, f"stem6x6s2 {H}x{W}")
            else:
                _record("stem6x6s2", R.check_bound(got, y, bound, f"stem6x6s2 {H}x{W} silu={silu}"))
        assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))


@pytest.mark.parametrize("width", [(16, 32), (48, 64), (64, 64), (80, 96)], ids=["n", "m", "l", "x"])
def test_stem6x6s2_g16(dev, width):
    """The stem at the yolov5 n / m / l / x widths: channel groups of 16, the padded channels cout .. cout_st exactly 0."""
    L = CL.lib()
    cout, cout_st = width
    for (H, W) in ((10, 16), (7, 24), (16, 8)):
        x, w, bias = _stem_data(2, H, W, cout, "real", 42)
        y, bound, _ = _stem_ref(x, w, bias, 1)
        OH, OW = (H + 4 - 6) // 2 + 1, (W + 4 - 6) // 2 + 1
        assert OW % 4 == 0
        wt = torch.zeros(108, cout_st)
        wt[:, :cout] = R.pack_w(w).t()
        bz = torch.zeros(cout_st)
        bz[:cout] = bias
        d_x, d_wt, d_b = x.to(dev), wt.to(dev), bz.to(dev)
        out_ld, out_off = cout_st + 8, 4
        out = _out_buffer(2 * OH * OW, out_ld, F32, dev)
        _ok(L.effocr_convops_stem6x6s2_g16(CL.ptr(d_x), CL.ptr(d_wt), cout_st, CL.ptr(d_b), CL.ptr(out), 2, H, W, OH, OW, out_ld, out_off, cout, cout_st,
                                           _stream(dev)))
        torch.cuda.synchronize(dev)
        _unchanged(d_x, x, "the input")
        got = _take(out, 2 * OH * OW, out_off, cout_st, "stem6x6s2_g16").reshape(2, OH, OW, cout_st)
        assert torch.equal(_bits(got[..., cout:]), _bits(torch.zeros_like(got[..., cout:]))), "padded channels must be exactly +0"
        _record("stem6x6s2_g16", R.check_bound(got[..., :cout].contiguous(), y, bound, f"stem6x6s2_g16 {cout}/{cout_st} {H}x{W}"))
