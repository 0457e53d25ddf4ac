"""-m gpu: the two kernels of yolo11.hip alone, through the op entry points of libeffocr_yolo11.so — the attention against a float64
softmax and the depthwise 3x3 convolution against F.conv2d(groups=C) in float64.

Bound (both): the error of a float32 CPU restatement of the kernel's own algorithm (tests/yolo11_ref.py: attention_tiled, dwconv_taps)
against float64 on the same inputs, times 4, plus 1e-6 absolute.  The kernels sum in another order than the restatements (a lane's 16
keys and the quad shuffle; fused multiply-adds); 4 x leaves room for that and nothing more.  Every case prints both numbers
(``yolo11_parity op_...``); profiles/yolo11_parity.txt holds one run on an MI355X."""
import pytest
import torch
import torch.nn.functional as F

from effocr_amd import _lib
from tests.yolo11_ref import attention_exact, attention_tiled, dwconv_taps

pytestmark = pytest.mark.gpu

# one token | 2 x 2 | 15 (non-square) | 63, 64, 65: one below, at and above a 64-key tile | 400 (640 x 640) | the cap (1280 x 1280)
GRIDS = [(1, 1), (2, 2), (3, 5), (7, 9), (8, 8), (5, 13), (20, 20), (40, 40)]
_ATT = {}


def _attention_case(grid, heads):
    """(qkv [3, N, heads*128] float32, float64 reference, error of the float32 tiled restatement), once per case.  q and k are scaled by
    sqrt 3 each: the logits 32^-1/2 q . k then have a standard deviation of 3."""
    key = (grid, heads)
    if key not in _ATT:
        N = grid[0] * grid[1]
        qkv = torch.randn(3, N, heads, 128, generator=torch.Generator().manual_seed(100 * N + heads))
        qkv[..., :64] *= 3 ** 0.5
        qkv = qkv.reshape(3, N, heads * 128)
        ref = torch.cat([attention_exact(qkv[i:i + 1].double(), heads) for i in range(3)])
        cpu32 = (torch.cat([attention_tiled(qkv[i:i + 1], heads) for i in range(3)]).double() - ref).abs().max().item()
        _ATT[key] = (qkv, ref, cpu32)
    return _ATT[key]


def _attention(dev, qkv, grid, heads):
    L = _lib.yolo11_lib()
    x = qkv.to(dev).contiguous()
    out = torch.full((x.shape[0], x.shape[1], heads * 64), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.yolo11_check(L.effocr_yolo11_op_attention(_lib.ptr(x), x.shape[0], grid[0], grid[1], heads, _lib.ptr(out), _lib.current_stream(dev)),
                          "effocr_yolo11_op_attention")
    return out.cpu()


@pytest.mark.parametrize("heads", [2, 4, 6])
@pytest.mark.parametrize("grid", GRIDS)
def test_op_attention(dev, grid, heads):
    """Batch 3 against float64; the output of an image is bitwise the same alone (batch 1) and at every position of the batch."""
    qkv, ref, cpu32 = _attention_case(grid, heads)
    assert grid[0] * grid[1] <= _lib.YOLO11_MAX_TOKENS
    got = _attention(dev, qkv, grid, heads)
    err, bound = (got.double() - ref).abs().max().item(), 4 * cpu32 + 1e-6
    print(f"yolo11_parity op_attention {grid[0]}x{grid[1]} heads={heads} B=3: device {err:.3e} | cpu fp32 {cpu32:.3e} | bound {bound:.3e}")
    assert torch.isfinite(got).all() and err < bound, (err, bound)
    for i in range(3):
        assert torch.equal(_attention(dev, qkv[i:i + 1], grid, heads)[0], got[i])
    rolled = _attention(dev, qkv.roll(1, 0), grid, heads)
    assert torch.equal(rolled.roll(-1, 0), got)


def test_op_attention_refuses_more_tokens_than_the_cap(dev):
    L = _lib.yolo11_lib()
    x = torch.zeros(1, 41 * 40, 256, device=dev)
    out = torch.zeros(1, 41 * 40, 128, device=dev)
    assert L.effocr_yolo11_op_attention(_lib.ptr(x), 1, 41, 40, 2, _lib.ptr(out), None) == -2
    assert b"1600 tokens" in L.effocr_yolo11_last_error()


_DW = {}


def _dw_case(hw, C, silu):
    key = (hw, C, silu)
    if key not in _DW:
        g = torch.Generator().manual_seed(7 * hw[0] + 13 * hw[1] + C + silu)
        x = torch.randn(2, hw[0], hw[1], C, generator=g)
        w = torch.randn(C, 9, generator=g) / 3
        b = torch.randn(C, generator=g)
        y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().view(C, 1, 3, 3), b.double(), padding=1, groups=C)
        ref = (F.silu(y) if silu else y).permute(0, 2, 3, 1)
        cpu32 = (dwconv_taps(x, w, b, silu).double() - ref).abs().max().item()
        _DW[key] = (x, w, b, ref, cpu32)
    return _DW[key]


@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("C", [64, 384])
@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (5, 3), (20, 20), (80, 80)])
def test_op_dwconv3x3(dev, hw, C, silu):
    """Dense rows, then rows wider than C on both sides (the channel-slice views the network uses): the same bits, and nothing written
    past channel C."""
    x, w, b, ref, cpu32 = _dw_case(hw, C, silu)
    L = _lib.yolo11_lib()
    wd, bd = w.to(dev).contiguous(), b.to(dev).contiguous()

    def run(ld_in, ld_out):
        xin = torch.full((2, hw[0], hw[1], ld_in), float("nan"), dtype=torch.float32, device=dev)
        xin[..., :C] = x.to(dev)
        out = torch.full((2, hw[0], hw[1], ld_out), -7.0, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.yolo11_check(L.effocr_yolo11_op_dwconv3x3(_lib.ptr(xin), 2, hw[0], hw[1], C, ld_in, _lib.ptr(wd), _lib.ptr(bd), silu, _lib.ptr(out), ld_out,
                                                           _lib.current_stream(dev)), "effocr_yolo11_op_dwconv3x3")
        return out.cpu()

    got = run(C, C)
    err, bound = (got.double() - ref).abs().max().item(), 4 * cpu32 + 1e-6
    print(f"yolo11_parity op_dwconv3x3 {hw[0]}x{hw[1]} C={C} silu={silu} B=2: device {err:.3e} | cpu fp32 {cpu32:.3e} | bound {bound:.3e}")
    assert err < bound, (err, bound)
    wide = run(C + 32, C + 64)
    assert torch.equal(wide[..., :C], got) and (wide[..., C:] == -7.0).all()
