"""libeffocr_levit.so's own kernels alone on the MI355X (-m gpu), through the test entry points of include/effocr_levit.h: the attention
(queries and keys 16 or 32 wide, values 2 or 4 times that, the (|dy|, |dx|) bias, stride-1 and strided queries, every key count around the
32-key MFMA tile and the 4-key tail of the 14 x 14 grid) and the stem convolution, each against float64 on operands already rounded to the
mode's type.

Bounds (max norm relative to max|ref|).  Attention: fp32 1e-5; 16-bit modes 2 x the error of attention_emulated (tests/levit_ref.py) — the
float64 computation with only the roundings csrc/levit.hpp declares (P and the output) — on the same case, computed on the CPU at run time;
the factor 2 is for accumulation order and the hardware exp, which the emulation does not model.  Stem convolution: what is left on rounded
operands is fp32 accumulation (1e-5) and, where the output is 16-bit, its one rounding: half an ulp, 2^-11 (f16) / 2^-8 (bf16)."""
import pytest
import torch
import torch.nn.functional as F

from effocr_amd import _lib
from tests.levit_ref import attention_emulated, attention_ref, bias_index, hardswish, header_grids, sub

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
PREC = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}
OP_FP32 = 1e-5
HALF_ULP = {"fp32": 0.0, "fp16": 2.0 ** -11, "bf16": 2.0 ** -8}
B_OP, HEADS_OP = 2, 2


GRIDS, KTILE, KTAIL = header_grids()                       # tests/test_levit_host.py checks that the grids surround the tile sizes


def rel_err(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def _case(seed, R, stride, kd, vd, prec, zero_qk=False):
    """q [B, h, Tq, kd], k [B, h, Tk, kd], v [B, h, Tk, vd] already rounded to the mode's type (as float64), table [h, R^2] fp32."""
    g = torch.Generator().manual_seed(seed)
    Tk, Tq = R * R, (sub(R) if stride == 2 else R) ** 2
    q = torch.randn(B_OP, HEADS_OP, Tq, kd, generator=g)
    k = torch.randn(B_OP, HEADS_OP, Tk, kd, generator=g)
    v = torch.randn(B_OP, HEADS_OP, Tk, vd, generator=g)
    table = torch.randn(HEADS_OP, Tk, generator=g)
    if zero_qk:
        q, k, table = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(table)
    return tuple(t.to(DT[prec]).double() for t in (q, k, v)) + (table,)


def _op_attention(dev, q, k, v, table, R, stride, prec, act=0, tail_value=None):
    """effocr_levit_op_attention in the product's two layouts: stride 1 — one buffer of rows [q kd | k kd | v vd] per head; stride 2 — a
    kv buffer of rows [k kd | v vd] per head and a q buffer.  The output is pre-filled with NaN; ``tail_value``: 64 rows of that value lie
    BEHIND the key / value rows in the same allocation — what a kernel that reads a padded key of the last crop would fetch."""
    L = _lib.levit_lib()
    dt = DT[prec]
    B, h, Tq, kd = q.shape
    Tk, vd = v.shape[2], v.shape[3]
    rows = lambda t: t.transpose(1, 2).reshape(t.shape[0] * t.shape[2], h, t.shape[3])          # [B*T, h, d]
    if stride == 1:
        kvbuf = torch.cat([rows(q), rows(k), rows(v)], dim=2).reshape(B * Tk, -1)
        hs, koff, voff = 2 * kd + vd, kd, 2 * kd
    else:
        kvbuf = torch.cat([rows(k), rows(v)], dim=2).reshape(B * Tk, -1)
        hs, koff, voff = kd + vd, 0, kd
    if tail_value is not None:
        kvbuf = torch.cat([kvbuf, torch.full((64, kvbuf.shape[1]), tail_value, dtype=kvbuf.dtype)])
    kvbuf = kvbuf.to(dt).to(dev).contiguous()
    if stride == 1:
        qbuf, ldq, qhs = kvbuf, h * hs, hs
    else:
        qbuf, ldq, qhs = rows(q).reshape(B * Tq, -1).to(dt).to(dev).contiguous(), h * kd, kd
    tb = table.float().to(dev).contiguous()
    out = torch.full((B * Tq, h * vd), float("nan"), dtype=dt, device=dev)
    _lib.levit_check(L.effocr_levit_op_attention(_lib.ptr(qbuf), ldq, qhs, 0, _lib.ptr(kvbuf), h * hs, hs, koff, voff, _lib.ptr(tb), B, R, stride,
                                                 h, kd, vd, act, PREC[dt], _lib.ptr(out), _lib.current_stream(dev)), "effocr_levit_op_attention")
    torch.cuda.synchronize(dev)
    return out.cpu().double().reshape(B, Tq, h, vd).transpose(1, 2)


def _bound(q, k, v, table, R, stride, prec, act=False):
    ref = attention_ref(q, k, v, table.double(), R, stride, act=act)
    if prec == "fp32":
        return ref, OP_FP32, 0.0
    emu = rel_err(attention_emulated(q, k, v, table, R, stride, act=act, dtype=DT[prec]), ref)
    return ref, 2 * emu, emu


def _check(dev, what, q, k, v, table, R, stride, prec, act=0, tail_value=None):
    ref, bound, emu = _bound(q, k, v, table, R, stride, prec, bool(act))
    got = _op_attention(dev, q, k, v, table, R, stride, prec, act, tail_value)
    assert torch.isfinite(got).all()                       # every row was written
    e = rel_err(got, ref)
    print(f"levit op_attention {prec} kd={q.shape[-1]} vd={v.shape[-1]} R={R} stride={stride} {what}: max-norm {e:.3e}  emulated {emu:.3e}  bound {bound:.3e}")
    assert e <= bound, (what, R, stride, q.shape[-1], v.shape[-1], e, bound)
    return got, ref, bound


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("kd", [16, 32])
def test_op_attention(dev, prec, kd):
    """random N(0, 1) q, k, v and biases: every grid, both strides, both value widths; hardswish on and off"""
    for R in GRIDS:
        for stride in (1, 2):
            for mult in (2, 4):
                q, k, v, table = _case(100 * R + 10 * stride + mult, R, stride, kd, mult * kd, prec)
                _check(dev, "random", q, k, v, table, R, stride, prec, act=(R + mult) % 2)


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("kd", [16, 32])
def test_op_attention_padding_is_exact(dev, prec, kd):
    """q = k = 0 with zero biases: every output row is the mean of exactly that crop-head's Tk value rows.  The rows behind a crop in memory
    (the next crop's, and 64 rows of 50.0 behind the last) are what an unmasked padded key would bring in."""
    for R in GRIDS:
        for stride, mult in ((1, 2), (2, 4)):
            q, k, v, table = _case(7000 + R, R, stride, kd, mult * kd, prec, zero_qk=True)
            ref, bound, _ = _bound(q, k, v, table, R, stride, prec)
            mean = v.mean(2, keepdim=True).expand_as(ref)
            assert rel_err(ref, mean) < 1e-13
            # on the CPU: a mean with one padded key included, or one live key dropped, is outside the bound at this key count
            nxt = torch.cat([v[1:], torch.full_like(v[:1], 50.0)])[:, :, :1]       # the value row behind each crop's keys
            plus = torch.cat([v, nxt], dim=2).mean(2)
            assert rel_err(plus, v.mean(2)) > bound, (R, rel_err(plus, v.mean(2)), bound)
            if R > 1:
                assert rel_err(v[:, :, :-1].mean(2), v.mean(2)) > bound, (R, bound)
            _check(dev, "q=k=0", q, k, v, table, R, stride, prec, tail_value=50.0)


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("stride", [1, 2])
def test_op_attention_bias_spike(dev, prec, stride):
    """One bias entry at +40, (|dy|, |dx|) = (2, 3) of the 14 x 14 grid: every query's softmax collapses onto the keys at that offset (one
    to four of them), in whichever key tile they lie; |dy| and |dx| swapped would pick other keys."""
    R, kd, vd = 14, 16, 32
    q, k, v, table = _case(9000 + stride, R, stride, kd, vd, prec)
    table[:, 2 * R + 3] = 40.0
    idx = bias_index(R, stride)
    hit = (idx == 2 * R + 3).double()                      # [Tq, Tk]
    some = hit.sum(1) > 0
    assert some.sum() > 20 and hit.sum(1).max() == 4
    got, ref, bound = _check(dev, "spike", q, k, v, table, R, stride, prec)
    # on the CPU: the reference rows of those queries weigh every other key e^-30 or less ...
    w = (q @ k.transpose(-1, -2) * kd ** -0.5 + table.double()[:, idx]).softmax(-1)
    assert (w * (1 - hit)).sum(-1)[:, :, some].max() < 1e-9
    # ... and the same table read with |dy| and |dx| swapped lands on other keys: far outside the bound
    swapped = table.reshape(-1, R, R).transpose(1, 2).reshape(-1, R * R)
    assert rel_err(attention_ref(q, k, v, swapped.double(), R, stride), ref) > 10 * bound


# -- the stem convolution -----------------------------------------------------------------------------------------------------------
def _conv_case(seed, B, H, cin, cout, prec):
    g = torch.Generator().manual_seed(seed)
    dt = DT[prec]
    x = torch.randn(B, cin, H, H, generator=g).to(dt).double()
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)).to(dt).double()
    bias = torch.randn(cout, generator=g) * 0.2
    return x, w, bias


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("form", ["nchw", "tokens", "tokens_f32"])
def test_op_stem_conv(dev, prec, form):
    """3x3 / stride 2 / pad 1 + bias (+ hardswish) against F.conv2d in float64 on the same rounded operands: the NCHW fp32 crops (3
    channels), token-major 16-bit rows (24 -> 48 channels, the levit_192 widths) and the last convolution's fp32 rows with zeroed padding
    columns; an even and an odd size (the bottom / right taps fall outside the odd one), two crops, more than one workgroup."""
    L = _lib.levit_lib()
    dt = DT[prec]
    for H in (14, 13):
        cin, cout, act = (3, 16, 1) if form == "nchw" else (24, 48, 1 if form == "tokens" else 0)
        ldo = cout if form != "tokens_f32" else 128
        out_f32 = form == "tokens_f32"
        x, w, bias = _conv_case(31 * H + cin, 2, H, cin, cout, prec)
        ref = F.conv2d(x, w, stride=2, padding=1) + bias.double()[None, :, None, None]
        ref = (hardswish(ref) if act else ref).flatten(2).transpose(1, 2)                      # [B, OH^2, cout]
        OH = (H - 1) // 2 + 1
        assert ref.shape == (2, OH * OH, cout)
        wt = w.permute(2, 3, 1, 0).reshape(9 * cin, cout).float().to(dev).contiguous()         # row (ky*3 + kx)*cin + c
        xin = x.float().to(dev).contiguous() if form == "nchw" else x.flatten(2).transpose(1, 2).to(dt).to(dev).contiguous()
        out = torch.full((2, OH * OH, ldo), float("nan"), dtype=torch.float32 if out_f32 else dt, device=dev)
        b = bias.to(dev)
        _lib.levit_check(L.effocr_levit_op_stem_conv(_lib.ptr(xin), int(form == "nchw"), 2, H, cin, _lib.ptr(wt), _lib.ptr(b), cout, act, PREC[dt],
                                                     _lib.ptr(out), ldo, int(out_f32), _lib.current_stream(dev)), "effocr_levit_op_stem_conv")
        torch.cuda.synchronize(dev)
        got = out.cpu().double()
        assert (got[..., cout:] == 0).all()                # the padding columns are written as zeros
        e = rel_err(got[..., :cout], ref)
        bound = OP_FP32 + (0.0 if out_f32 else HALF_ULP[prec])
        print(f"levit op_stem_conv {prec} {form} H={H}: max-norm {e:.3e}  bound {bound:.3e}")
        assert e <= bound


def test_op_refusals(dev):
    L = _lib.levit_lib()
    p = _lib.ptr(torch.zeros(4096, device=dev))
    assert L.effocr_levit_op_attention(p, 64, 64, 0, p, 64, 64, 16, 32, p, 1, 15, 1, 1, 16, 32, 0, 1, p, None) == -2     # grid 15
    assert L.effocr_levit_op_attention(p, 64, 64, 0, p, 64, 64, 16, 32, p, 1, 2, 3, 1, 16, 32, 0, 1, p, None) == -2      # stride 3
    assert L.effocr_levit_op_attention(p, 64, 64, 0, p, 64, 64, 16, 32, p, 1, 2, 1, 1, 16, 48, 0, 1, p, None) == -1      # v does not fit its row
    assert L.effocr_levit_op_attention(p, 128, 128, 0, p, 128, 128, 16, 32, p, 1, 2, 1, 1, 16, 96, 0, 1, p, None) == -2  # value width 96
    assert L.effocr_levit_op_attention(p, 64, 64, 0, p, 64, 64, 16, 32, None, 1, 2, 1, 1, 16, 32, 0, 1, p, None) == -1
    assert L.effocr_levit_op_stem_conv(p, 0, 1, 8, 12, p, p, 16, 1, 1, p, 16, 0, None) == -2                             # cin 12 in token rows
    assert L.effocr_levit_op_stem_conv(p, 1, 1, 8, 3, p, p, 18, 1, 1, p, 20, 0, None) == -2                              # cout 18
