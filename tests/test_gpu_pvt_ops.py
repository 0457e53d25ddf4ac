"""libeffocr_pvt.so's own kernels alone on the MI355X (-m gpu), through the test entry points of include/effocr_pvt.h that no product code
calls: the reduced-key attention, the depthwise 3x3 + GELU on token rows, the 7x7/4 stem, the 3x3/2 down-sampling and the spatial
reduction (the last three with the LayerNorm behind them), each against float64 on operands already rounded to the mode's type.

Bounds (max norm relative to max|ref|).
  attention, depthwise + GELU   fp32: 1e-5, the project's exact-mode bound.  16-bit: 2 x the error of the CPU emulation of the declared
                                roundings (csrc/pvt.hpp) on the same case, computed at run time — attention: tests/pvt_ref.py
                                attention_emulated (P and the output rounded); depthwise: the float64 result rounded once on the store.
                                The factor 2 covers fp32 accumulation order and the hardware exp, as in tests/test_gpu_vit8.py.
  stem, down-sampling,          1e-5 in every mode: these operators write fp32 from rounded operands (the crop pixels are rounded as they
  reduction                     are read, which the reference does too), so only the accumulation order and the fp32 LayerNorm are left.
"""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from effocr_amd import _lib
from tests import pvt_ref as R

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
PREC = {"bf16": 0, "fp16": 1, "fp32": 2}
PRECS = ["fp32", "fp16", "bf16"]
OP_FP32 = 1e-5
B_OP = 2
_HPP = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "effocr_amd", "csrc", "pvt.hpp")).read()
QBLK = int(re.search(r"constexpr int PVT_QBLK = (\d+);", _HPP).group(1))       # the query tile, read where the kernel states it
QCHUNK = int(re.search(r"constexpr int PVT_QCHUNK = (\d+);", _HPP).group(1))   # queries per workgroup
KEYS = (1, 4, 9, 16, 25, 36, 49)
QUERIES = sorted({1, 4, 49, 196, QBLK - 1, QBLK, QBLK + 1, QCHUNK + 1})


def rel_err(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def stream(dev):
    return _lib.current_stream(dev)


# ---------------------------------------------------------------------------------------------------------------- attention
def _qkv(seed, N, M, heads, hd, prec, gain=1.0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B_OP * N, heads * hd, generator=g) * gain
    kv = torch.randn(B_OP * M, 2 * heads * hd, generator=g)
    kv[:, :heads * hd] *= gain
    return q.to(DT[prec]).double(), kv.to(DT[prec]).double()


def _op_attention(dev, q, kv, N, M, heads, hd, prec, tail_value=None):
    """effocr_pvt_op_attention; the output is pre-filled with NaN.  ``tail_value``: 64 rows of that value lie BEHIND the kv rows in the same
    allocation — what a kernel that reads a padded key of the last crop would fetch."""
    dt = DT[prec]
    if tail_value is not None:
        kv = torch.cat([kv, torch.full((64, kv.shape[1]), tail_value, dtype=kv.dtype)])
    qd, kvd = q.to(dt).to(dev).contiguous(), kv.to(dt).to(dev).contiguous()
    out = torch.full((B_OP * N, heads * hd), float("nan"), dtype=dt, device=dev)
    _lib.pvt_check(_lib.pvt_lib().effocr_pvt_op_attention(_lib.ptr(qd), _lib.ptr(kvd), B_OP, N, M, heads, hd, PREC[prec], _lib.ptr(out), stream(dev)),
                   "effocr_pvt_op_attention")
    torch.cuda.synchronize(dev)
    return out.cpu().double()


def _attn_bound(q, kv, N, M, heads, hd, prec):
    ref = R.attention_ref(q, kv, B_OP, N, M, heads, hd)
    if prec == "fp32":
        return ref, OP_FP32, 0.0
    emu = rel_err(R.attention_emulated(q, kv, B_OP, N, M, heads, hd, prec), ref)
    return ref, 2 * emu, emu


def _attn_check(dev, what, q, kv, N, M, heads, hd, prec, tail_value=None):
    ref, bound, emu = _attn_bound(q, kv, N, M, heads, hd, prec)
    got = _op_attention(dev, q, kv, N, M, heads, hd, prec, tail_value)
    assert torch.isfinite(got).all()                       # every row was written
    e = rel_err(got, ref)
    print(f"pvt op_attention {prec} heads={heads} hd={hd} N={N} M={M} {what}: max-norm {e:.3e}  emulated {emu:.3e}  bound {bound:.3e}")
    assert e <= bound, (what, N, M, heads, hd, e, bound)
    return got, ref, bound


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("heads,hd", [(2, 32), (5, 32), (2, 64), (5, 64)])
def test_op_attention_grid(dev, prec, heads, hd):
    """random N(0, 1) q, k, v: every key count, every query count around the query tile and the workgroup's query chunk"""
    for M in KEYS:
        for N in QUERIES:
            q, kv = _qkv(1000 * M + N, N, M, heads, hd, prec)
            _attn_check(dev, "random", q, kv, N, M, heads, hd, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_op_attention_3136_queries(dev, prec):
    """the first stage at 224^2: 3136 queries on 49 keys, seven query chunks per (crop, head)"""
    q, kv = _qkv(77, 3136, 49, 2, 64, prec)
    _attn_check(dev, "stage 0", q, kv, 3136, 49, 2, 64, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("hd", [32, 64])
def test_op_attention_padding_is_exact(dev, prec, hd):
    """q = k = 0: every output row is the mean of exactly that crop's M value rows.  The rows behind a crop in memory (the next crop's, and
    64 rows of 50.0 behind the last) are what an unmasked padded key would bring in."""
    heads, N = 2, QBLK + 1
    C = heads * hd
    for M in KEYS:
        _, kv = _qkv(31 * M, N, M, heads, hd, prec)
        kv[:, :C] = 0
        q = torch.zeros(B_OP * N, C, dtype=torch.float64)
        v = kv[:, C:].reshape(B_OP, M, C)
        mean = v.mean(1)
        ref, bound, _ = _attn_bound(q, kv, N, M, heads, hd, prec)
        assert torch.allclose(ref.reshape(B_OP, N, C), mean[:, None].expand(B_OP, N, C), rtol=1e-12, atol=1e-12)
        # on the CPU first: one row more (the next row in memory) or one row less would be caught
        behind = torch.cat([kv[:, C:], torch.full((64, C), 50.0, dtype=torch.float64)])
        for b in range(B_OP):
            more = (v[b].sum(0) + behind[(b + 1) * M]) / (M + 1)
            assert ((more - mean[b]).abs().max() / ref.abs().max()).item() > 2 * max(bound, 1e-5), (M, b)
            if M > 1:
                less = v[b, :-1].mean(0)
                assert ((less - mean[b]).abs().max() / ref.abs().max()).item() > 2 * max(bound, 1e-5), (M, b)
        _attn_check(dev, "padding", q, kv, N, M, heads, hd, prec, tail_value=50.0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("hd", [32, 64])
def test_op_attention_large_logits(dev, prec, hd):
    """q and k scaled so that the scaled scores reach about +-100: float64 is finite, and so is the kernel, within the bound.  Without
    the maximum subtracted before exp, fp16 (and fp32 beyond 88) overflows here."""
    heads, N, M = 2, 49, 49
    q, kv = _qkv(5, N, M, heads, hd, "fp32")
    s = torch.einsum("bnhd,bmhd->bhnm", q.reshape(B_OP, N, heads, hd), kv[:, :heads * hd].reshape(B_OP, M, heads, hd)) / math.sqrt(hd)
    gain = math.sqrt(100.0 / s.abs().max().item())
    q, kv = _qkv(5, N, M, heads, hd, prec, gain=gain)
    s = torch.einsum("bnhd,bmhd->bhnm", q.reshape(B_OP, N, heads, hd), kv[:, :heads * hd].reshape(B_OP, M, heads, hd)) / math.sqrt(hd)
    assert 90 < s.abs().max().item() < 110 and s.max().item() > 60 and s.min().item() < -60
    assert not torch.isfinite(torch.exp(s).to(torch.float16)).all()            # what skipping the subtraction would do
    ref = R.attention_ref(q, kv, B_OP, N, M, heads, hd)
    assert torch.isfinite(ref).all()
    _attn_check(dev, "logits +-100", q, kv, N, M, heads, hd, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_op_attention_isolation(dev, prec):
    """changing crop 1's kv leaves crop 0's output bitwise unchanged; changing head 1's leaves head 0's"""
    heads, hd, N, M = 2, 64, QBLK + 1, 25
    C = heads * hd
    q, kv = _qkv(9, N, M, heads, hd, prec)
    base = _op_attention(dev, q, kv, N, M, heads, hd, prec)
    kv2 = kv.clone()
    kv2[M:] = _qkv(10, N, M, heads, hd, prec)[1][M:]
    other = _op_attention(dev, q, kv2, N, M, heads, hd, prec)
    assert torch.equal(other[:N], base[:N]) and not torch.equal(other[N:], base[N:])
    kv3 = kv.clone()
    new = _qkv(11, N, M, heads, hd, prec)[1]
    kv3[:, hd:C], kv3[:, C + hd:] = new[:, hd:C], new[:, C + hd:]
    other = _op_attention(dev, q, kv3, N, M, heads, hd, prec)
    assert torch.equal(other[:, :hd], base[:, :hd]) and not torch.equal(other[:, hd:], base[:, hd:])


# ---------------------------------------------------------------------------------------------------------------- depthwise 3x3 + GELU
def _op_dwconv(dev, x, w, b, H, W, prec, tail_value=None):
    """x [B, H*W, C] (already rounded), w [C, 1, 3, 3] (already rounded), b [C] -> effocr_pvt_op_dwconv_gelu, output pre-filled with NaN"""
    dt = DT[prec]
    B, _, C = x.shape
    xin = x.reshape(B * H * W, C)
    if tail_value is not None:
        xin = torch.cat([xin, torch.full((64, C), tail_value, dtype=xin.dtype)])
    xd = xin.to(dt).to(dev).contiguous()
    wd = w.reshape(C, 9).t().float().to(dev).contiguous()                      # [9][C]
    bd = b.float().to(dev).contiguous()
    out = torch.full((B * H * W, C), float("nan"), dtype=dt, device=dev)
    _lib.pvt_check(_lib.pvt_lib().effocr_pvt_op_dwconv_gelu(_lib.ptr(xd), B, H, W, C, _lib.ptr(wd), _lib.ptr(bd), PREC[prec], _lib.ptr(out), stream(dev)),
                   "effocr_pvt_op_dwconv_gelu")
    torch.cuda.synchronize(dev)
    return out.cpu().double().reshape(B, H * W, C)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C", [64, 640])
def test_op_dwconv_gelu_grid(dev, prec, C):
    for H in (1, 2, 3, 7, 8, 14, 56):
        if H == 56 and C != 64:
            continue
        g = torch.Generator().manual_seed(100 * H + C)
        x = R.rnd(torch.randn(B_OP, H * H, C, generator=g), prec).double()
        w = R.rnd(torch.randn(C, 1, 3, 3, generator=g) / 3, prec).double()
        b = (torch.randn(C, generator=g) * 0.1).float().double()
        ref = R.dwconv_gelu_ref(x, w, b, H, H)
        emu = 0.0 if prec == "fp32" else rel_err(R.rnd(ref, prec), ref)
        bound = OP_FP32 if prec == "fp32" else 2 * emu
        got = _op_dwconv(dev, x, w, b, H, H, prec)
        assert torch.isfinite(got).all()
        e = rel_err(got, ref)
        print(f"pvt op_dwconv_gelu {prec} C={C} H=W={H}: max-norm {e:.3e}  emulated {emu:.3e}  bound {bound:.3e}")
        assert e <= bound, (H, C, e, bound)


@pytest.mark.parametrize("prec", PRECS)
def test_op_dwconv_gelu_borders(dev, prec):
    """x = 1 (crop 0) / 2 (crop 1), w = 1, b = 0: the pre-activation is the number of taps inside the crop's own grid — 9, 6 or 4 by position
    (fewer on grids under 3 wide) — times the crop's value.  A tap that crossed a row end, a crop end or the buffer end (64 rows of 50.0
    lie behind it) would change the count."""
    C = 64
    for H, W in ((1, 1), (2, 2), (3, 3), (7, 7), (3, 5), (5, 2)):
        x = torch.ones(B_OP, H * W, C, dtype=torch.float64)
        x[1] = 2.0
        w = torch.ones(C, 1, 3, 3, dtype=torch.float64)
        b = torch.zeros(C, dtype=torch.float64)
        ny = torch.tensor([min(y + 1, H - 1) - max(y - 1, 0) + 1 for y in range(H)])
        nx = torch.tensor([min(xx + 1, W - 1) - max(xx - 1, 0) + 1 for xx in range(W)])
        count = (ny[:, None] * nx[None, :]).double().reshape(1, H * W, 1)
        if H >= 3 and W >= 3:
            c2 = count.reshape(H, W)
            assert c2[0, 0] == c2[0, -1] == c2[-1, 0] == c2[-1, -1] == 4 and c2[0, 1] == c2[1, 0] == c2[-1, 1] == c2[1, -1] == 6 and c2[1, 1] == 9
        want = F.gelu(count * x)
        got = _op_dwconv(dev, x, w, b, H, W, prec, tail_value=50.0)
        half_ulp = {"fp32": 1e-6, "fp16": 2.0 ** -11, "bf16": 2.0 ** -8}[prec]
        assert (got - want).abs().max().item() <= 1.01 * half_ulp * want.abs().max().item(), (H, W)
        # and the general reference agrees with the count
        assert torch.allclose(R.dwconv_gelu_ref(x, w, b, H, W), want, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- patch embeddings, reduction
def _ln_params(g, C):
    return (torch.rand(C, generator=g) + 0.5).double(), (torch.randn(C, generator=g) * 0.1).double()


def _check_f32(what, got, ref):
    assert torch.isfinite(got).all()
    e = rel_err(got, ref)
    print(f"pvt {what}: max-norm {e:.3e}  bound {OP_FP32:.0e}")
    assert e <= OP_FP32, (what, e)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cout", [32, 64])
def test_op_stem(dev, prec, cout):
    for img in (32, 64, 224):
        g = torch.Generator().manual_seed(img + cout)
        x = R.crops(B_OP, img, seed=img).float()
        w = R.rnd(torch.randn(cout, 3, 7, 7, generator=g) / math.sqrt(147), prec).double()
        b = (torch.randn(cout, generator=g) * 0.1).double()
        lnw, lnb = _ln_params(g, cout)
        ref = R.conv_ln_ref(R.rnd(x, prec).double(), w, b, lnw, lnb, 4, 3).reshape(-1, cout)
        wp = torch.zeros(cout, 160, dtype=torch.float64)
        wp[:, :147] = w.reshape(cout, 147)
        dv = lambda t, dt=torch.float32: t.to(dt).to(dev).contiguous()
        out = torch.full((B_OP * (img // 4) ** 2, cout), float("nan"), dtype=torch.float32, device=dev)
        args = [dv(x), dv(wp, DT[prec]), dv(b), dv(lnw), dv(lnb)]
        _lib.pvt_check(_lib.pvt_lib().effocr_pvt_op_stem(_lib.ptr(args[0]), B_OP, img, cout, _lib.ptr(args[1]), _lib.ptr(args[2]), _lib.ptr(args[3]),
                                                         _lib.ptr(args[4]), PREC[prec], _lib.ptr(out), stream(dev)), "effocr_pvt_op_stem")
        torch.cuda.synchronize(dev)
        _check_f32(f"op_stem {prec} img={img} cout={cout}", out.cpu().double(), ref)


def _op_conv_ln(dev, tokens, side, w, b, lnw, lnb, k, stride, pad, prec):
    """tokens [B, side^2, Cin] and w [Cout, Cin, k, k] already rounded -> effocr_pvt_op_conv_ln and its float64 reference"""
    B, _, cin = tokens.shape
    cout = w.shape[0]
    ref = R.conv_ln_ref(R.tokens_to_img(tokens, side), w, b, lnw, lnb, stride, pad).reshape(-1, cout)
    dv = lambda t, dt=torch.float32: t.to(dt).to(dev).contiguous()
    args = [dv(tokens.reshape(-1, cin), DT[prec]), dv(w.permute(0, 2, 3, 1).reshape(cout, -1), DT[prec]), dv(b), dv(lnw), dv(lnb)]
    out = torch.full(ref.shape, float("nan"), dtype=torch.float32, device=dev)
    _lib.pvt_check(_lib.pvt_lib().effocr_pvt_op_conv_ln(_lib.ptr(args[0]), B, side, cin, cout, k, stride, pad, _lib.ptr(args[1]), _lib.ptr(args[2]),
                                                        _lib.ptr(args[3]), _lib.ptr(args[4]), PREC[prec], _lib.ptr(out), stream(dev)), "effocr_pvt_op_conv_ln")
    torch.cuda.synchronize(dev)
    return out.cpu().double(), ref


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 160), (160, 256), (320, 512)])
def test_op_downsample(dev, prec, cin, cout):
    for side in (2, 8, 14, 56):
        if side == 56 and cin != 32:
            continue
        g = torch.Generator().manual_seed(side * 1000 + cin)
        t = R.rnd(torch.randn(B_OP, side * side, cin, generator=g), prec).double()
        w = R.rnd(torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin), prec).double()
        b = (torch.randn(cout, generator=g) * 0.1).double()
        lnw, lnb = _ln_params(g, cout)
        got, ref = _op_conv_ln(dev, t, side, w, b, lnw, lnb, 3, 2, 1, prec)
        _check_f32(f"op_conv_ln 3x3/2 {prec} {cin}->{cout} side={side}", got, ref)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("sr,C,sides", [(8, 32, (8, 56)), (8, 64, (8,)), (4, 160, (4, 28)), (2, 320, (2, 14))])
def test_op_reduction(dev, prec, sr, C, sides):
    for side in sides:
        g = torch.Generator().manual_seed(side * 1000 + C)
        t = R.rnd(torch.randn(B_OP, side * side, C, generator=g), prec).double()
        w = R.rnd(torch.randn(C, C, sr, sr, generator=g) / math.sqrt(sr * sr * C), prec).double()
        b = (torch.randn(C, generator=g) * 0.1).double()
        lnw, lnb = _ln_params(g, C)
        got, ref = _op_conv_ln(dev, t, side, w, b, lnw, lnb, sr, sr, 0, prec)
        _check_f32(f"op_conv_ln {sr}x{sr}/{sr} {prec} C={C} side={side}", got, ref)
