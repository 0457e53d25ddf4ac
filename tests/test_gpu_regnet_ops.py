"""libeffocr_regnet.so's own kernels alone on the MI355X (-m gpu), through the test entry points of include/effocr_regnet.h: the grouped 3x3
convolution (group widths 8, 16 and 24; 1, 2, 3 and 7 groups, so that odd group counts leave a half-filled channel tile; every map size
around the 64-pixel run of a workgroup; both strides; all three precisions) with its tile sums, the squeeze-excite gate, the stem, the rows
of the strided shortcut and the ReLU behind the residual add.

Bounds (max norm relative to max|ref|).  Grouped convolution against float64 on weights already rounded to the mode's type: fp32 1e-5;
16-bit modes 2 x the error of gconv_emulated (tests/regnet_ref.py) — the roundings csrc/regnet.hpp declares, on the CPU — on the same
case, computed at run time; the factor 2 is for the accumulation order, which the emulation does not model.  Every output buffer is
pre-filled with NaN and 64 rows of 50.0 lie behind the last crop's input: a tap that reads past a crop shows."""
import pytest
import torch

from effocr_amd import _lib
from tests.regnet_ref import gconv_emulated, gconv_ref, round16

pytestmark = pytest.mark.gpu

PREC = {"bf16": 0, "fp16": 1, "fp32": 2}
B_OP = 2
GROUP_WIDTHS = (8, 16, 24)
GROUP_COUNTS = (1, 2, 3, 7)
SIZES = {1: (1, 2, 3, 7, 8, 14), 2: (2, 4, 8, 14, 16)}       # stride: input sizes (tests/test_regnet_host.py: they surround the tiles)
SE_SHAPES = ((24, 6), (24, 8), (48, 12), (336, 84))           # (C, R)
OP_FP32 = 1e-5


def rel_err(got, ref):
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _packed(w, gw, prec, dev):
    L = _lib.regnet_lib()
    C = w.shape[0]
    n = int(L.effocr_regnet_op_gconv_weight_bytes(PREC[prec], C, gw))
    host = torch.empty(n, dtype=torch.uint8)
    _lib.regnet_check(L.effocr_regnet_op_pack_gconv(PREC[prec], C, gw, _lib.ptr(w.float().contiguous()), _lib.ptr(host)), "pack_gconv")
    return host.to(dev)


def _op_gconv(dev, x, w, b, stride, gw, prec, want_part=False):
    """x [B,C,H,H] fp32 NCHW -> (out [B,C,Ho,Ho] float64 on the CPU, part [B,tiles,C] or None).  The output starts as NaN; 64 rows of 50.0
    lie behind the last crop's input in the same allocation."""
    L = _lib.regnet_lib()
    B, C, H, _ = x.shape
    Ho = (H - 1) // stride + 1
    buf = torch.cat([nhwc(x.float()).reshape(-1, C), torch.full((64, C), 50.0)]).to(dev).contiguous()
    wd, bd = _packed(w, gw, prec, dev), b.float().to(dev).contiguous()
    out = torch.full((B, Ho, Ho, C), float("nan"), dtype=torch.float32, device=dev)
    tiles = int(L.effocr_regnet_op_tiles(Ho))
    part = torch.full((B, tiles, C), float("nan"), dtype=torch.float32, device=dev) if want_part else None
    _lib.regnet_check(L.effocr_regnet_op_gconv(PREC[prec], _lib.ptr(buf), B, H, C, stride, gw, _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(out),
                                               _lib.ptr(part), _lib.current_stream(dev)), "effocr_regnet_op_gconv")
    torch.cuda.synchronize(dev)
    assert torch.equal(buf[-64:].cpu(), torch.full((64, C), 50.0))
    return out.cpu().double().permute(0, 3, 1, 2), (part.cpu().double() if want_part else None), out


def _shapes(stride):
    return [(n, H) for n in GROUP_COUNTS for H in SIZES[stride]]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("gw", GROUP_WIDTHS)
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_gconv_random_operands(dev, prec, gw, stride):
    for n, H in _shapes(stride):
        C = gw * n
        g = torch.Generator().manual_seed(1000 * gw + 10 * n + H + stride)
        x = torch.randn(B_OP, C, H, H, generator=g)
        w = torch.randn(C, gw, 3, 3, generator=g) / (3 * gw ** 0.5)
        b = torch.randn(C, generator=g) * 0.1
        wr = w if prec == "fp32" else round16(w, prec)                             # operands already rounded to the mode
        ref = gconv_ref(x.double(), wr.double(), b.double(), stride, gw)
        got, _, _ = _op_gconv(dev, x, wr, b, stride, gw, prec)
        assert got.shape == ref.shape and torch.isfinite(got).all(), (n, H)
        err = rel_err(got, ref)
        emu = rel_err(gconv_emulated(x, wr, b, stride, gw, prec).double(), ref)
        bound = OP_FP32 if prec == "fp32" else 2 * emu
        print(f"gconv {prec} gw {gw} groups {n} H {H} stride {stride}: err {err:.3e} emulated {emu:.3e} bound {bound:.3e}")
        assert err <= bound, (n, H, err, emu, bound)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("gw", GROUP_WIDTHS)
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_gconv_group_isolation(dev, prec, gw, stride):
    """The input is non-zero in one group's channels only: every output channel of every other group is ReLU(bias) exactly."""
    for n in (2, 3, 7):
        C, H = gw * n, SIZES[stride][3]
        g = torch.Generator().manual_seed(77 + n)
        w = torch.randn(C, gw, 3, 3, generator=g)
        b = torch.randn(C, generator=g)
        for live in sorted({0, n // 2, n - 1}):
            x = torch.zeros(B_OP, C, H, H)
            x[:, live * gw:(live + 1) * gw] = torch.randn(B_OP, gw, H, H, generator=g) * 3
            got, _, _ = _op_gconv(dev, x, w, b, stride, gw, prec)
            want = torch.relu(b).double()[None, :, None, None].expand_as(got)
            other = torch.ones(C, dtype=torch.bool)
            other[live * gw:(live + 1) * gw] = False
            assert torch.equal(got[:, other], want[:, other]), (n, live)
            assert not torch.equal(got[:, ~other], want[:, ~other])


def _tap_count(o, stride, H):
    return sum(1 for k in range(3) if 0 <= o * stride + k - 1 < H)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("gw", GROUP_WIDTHS)
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_gconv_borders(dev, prec, gw, stride):
    """Input and weights all ones, bias 0: an output is gw x (taps inside the map) — gw x {4, 6, 9} at corners, edges and the interior at
    stride 1 — small integers, exact in every mode, and the same for both crops: crop 0's bottom row does not see crop 1's top row, crop 1
    does not see the 50.0 rows."""
    for n in (1, 3):
        C = gw * n
        for H in SIZES[stride]:
            Ho = (H - 1) // stride + 1
            got, _, _ = _op_gconv(dev, torch.ones(B_OP, C, H, H), torch.ones(C, gw, 3, 3), torch.zeros(C), stride, gw, prec)
            cnt = torch.tensor([_tap_count(o, stride, H) for o in range(Ho)], dtype=torch.float64)
            want = (gw * cnt[:, None] * cnt[None, :])[None, None].expand(B_OP, C, Ho, Ho)
            assert torch.equal(got, want), (n, H)
            if stride == 1 and H >= 3:
                assert sorted(set(got.flatten().tolist())) == [4 * gw, 6 * gw, 9 * gw]
                assert got[0, 0, 0, 0] == 4 * gw and got[1, 0, H - 1, H - 1] == 4 * gw and got[0, 0, H - 1, 1] == 6 * gw and got[1, 0, 1, 1] == 9 * gw


@pytest.mark.parametrize("gw", GROUP_WIDTHS)
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_gconv_tile_sums(dev, prec, gw):
    """part [B][tiles][C] is the float64 sum of the STORED output over each run of 64 pixels within 1e-6; the tiles' sum over the pixel
    count reproduces mg_pool's mean (libeffocr_mnv3.so's entry point for the same kernel) within 1e-6."""
    M = _lib.mnv3_lib()
    for n, H, stride in ((1, 7, 1), (3, 8, 1), (2, 14, 1), (7, 14, 2), (3, 16, 2), (2, 1, 1)):
        C = gw * n
        g = torch.Generator().manual_seed(31 * gw + n + H)
        x = torch.randn(B_OP, C, H, H, generator=g)
        w = torch.randn(C, gw, 3, 3, generator=g) / (3 * gw ** 0.5)
        b = torch.randn(C, generator=g) * 0.1 + 0.2
        got, part, out_dev = _op_gconv(dev, x, w, b, stride, gw, prec, want_part=True)
        Ho = got.shape[2]
        rows = got.permute(0, 2, 3, 1).reshape(B_OP, Ho * Ho, C)
        tiles = part.shape[1]
        assert tiles == (Ho * Ho + 63) // 64
        want = torch.stack([rows[:, t * 64:(t + 1) * 64].sum(1) for t in range(tiles)], dim=1)
        assert torch.isfinite(part).all() and rel_err(part, want) <= 1e-6, (n, H, stride)
        pooled = torch.empty(B_OP, C, dtype=torch.float32, device=dev)
        _lib.mnv3_check(M.effocr_mnv3_op_pool(_lib.ptr(out_dev), B_OP, Ho * Ho, C, _lib.ptr(pooled), _lib.current_stream(dev)), "effocr_mnv3_op_pool")
        torch.cuda.synchronize(dev)
        assert rel_err(part.sum(1) / (Ho * Ho), pooled.cpu().double()) <= 1e-6


@pytest.mark.parametrize("C,R", SE_SHAPES)
def test_se_gate(dev, C, R):
    """rg_se_gate against float64, 1e-6: fp32 arithmetic in every mode (the kernel has no precision argument)."""
    L = _lib.regnet_lib()
    g = torch.Generator().manual_seed(C + R)
    NT, HW = 4, 196
    part = torch.rand(B_OP, NT, C, generator=g) * 60
    w1, b1 = torch.randn(R, C, generator=g) / C ** 0.5, torch.randn(R, generator=g) * 0.5
    w2, b2 = torch.randn(C, R, generator=g) * 2 / R ** 0.5, torch.randn(C, generator=g) * 0.5
    mean = part.double().sum(1) / HW
    hid = torch.relu(mean @ w1.double().t() + b1.double())
    want = torch.sigmoid(hid @ w2.double().t() + b2.double())
    assert want.min() < 0.3 and want.max() > 0.7 and (hid == 0).any() and (hid > 0).any()
    dpart, dw1, db1, dw2t, db2 = (t.float().contiguous().to(dev) for t in (part, w1, b1, w2.t(), b2))      # (kept alive over the launch)
    gate = torch.full((B_OP, C), float("nan"), dtype=torch.float32, device=dev)
    _lib.regnet_check(L.effocr_regnet_op_se_gate(_lib.ptr(dpart), B_OP, NT, HW, C, R, _lib.ptr(dw1), _lib.ptr(db1), _lib.ptr(dw2t),
                                                 _lib.ptr(db2), _lib.ptr(gate), _lib.current_stream(dev)), "effocr_regnet_op_se_gate")
    torch.cuda.synchronize(dev)
    err = rel_err(gate.cpu().double(), want)
    print(f"se_gate C {C} R {R}: err {err:.3e}")
    assert err <= 1e-6


@pytest.mark.parametrize("S", [32, 64])
def test_stem(dev, S):
    """The stem against float64 (an fp32 convolution in every mode: there is nothing to round), bound 1e-5; crop 1 must not see the rows
    behind it."""
    L = _lib.regnet_lib()
    g = torch.Generator().manual_seed(S)
    x = torch.randn(B_OP, 3, S, S, generator=g)
    w, b = torch.randn(32, 3, 3, 3, generator=g) / 27 ** 0.5, torch.randn(32, generator=g) * 0.1
    want = torch.relu(torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1))
    buf = torch.cat([x.flatten(), torch.full((64 * S,), 50.0)]).to(dev)
    wt = w.reshape(32, 27).t().contiguous().to(dev)
    out = torch.full((B_OP, S // 2, S // 2, 32), float("nan"), dtype=torch.float32, device=dev)
    bd = b.to(dev)
    _lib.regnet_check(L.effocr_regnet_op_stem(_lib.ptr(buf), B_OP, S, _lib.ptr(wt), _lib.ptr(bd), _lib.ptr(out), _lib.current_stream(dev)),
                      "effocr_regnet_op_stem")
    torch.cuda.synchronize(dev)
    got = out.cpu().double().permute(0, 3, 1, 2)
    err = rel_err(got, want)
    print(f"stem {S}: err {err:.3e}")
    assert torch.isfinite(got).all() and err <= OP_FP32 and (got == 0).any()


@pytest.mark.parametrize("H", [2, 4, 14])
def test_shortcut_rows(dev, H):
    L = _lib.regnet_lib()
    C = 24
    x = torch.randn(B_OP, H, H, C, generator=torch.Generator().manual_seed(H))
    Ho = (H - 1) // 2 + 1
    out = torch.full((B_OP, Ho, Ho, C), float("nan"), dtype=torch.float32, device=dev)
    xd = x.to(dev)
    _lib.regnet_check(L.effocr_regnet_op_gather2(_lib.ptr(xd), B_OP, H, C, _lib.ptr(out), _lib.current_stream(dev)), "effocr_regnet_op_gather2")
    torch.cuda.synchronize(dev)
    assert torch.equal(out.cpu(), x[:, ::2, ::2].contiguous())


def test_relu_after_add(dev):
    """conv3 + shortcut through mg_pw (no activation, the shortcut as its residual) leaves negative values; rg_relu clamps them in place and
    keeps NaN."""
    L = _lib.regnet_lib()
    x = torch.randn(1000, generator=torch.Generator().manual_seed(9))
    x[17] = float("nan")
    x[18], x[19] = -0.0, float("-inf")
    d = x.to(dev)
    _lib.regnet_check(L.effocr_regnet_op_relu(_lib.ptr(d), x.numel(), _lib.current_stream(dev)), "effocr_regnet_op_relu")
    torch.cuda.synchronize(dev)
    got = d.cpu()
    assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(torch.relu(x), nan=-7.0)) and torch.isnan(got[17]) and got[19] == 0
