"""Float64 references, test data, derived error bounds and the comparison functions of the operator parity tests
(tests/test_gpu_convops.py on the GPU; tests/test_convops_host.py proves on the CPU that the comparisons reject wrong kernels).

Two kinds of data per geometry, neither with a measured tolerance:

* exact: small integers (activations -3..3, weights -1/0/1, integer bias and residual).  Every product and partial sum is an integer
  below 2^24, so fp32 accumulation in ANY order is exact and the kernel must equal the float64 result cast to the output type bit for
  bit (`check_exact`).  `conv_reference` returns the float64 sum of |x||w| per output; `assert_exact_premise` holds it under 2^24.
* real: normal data compared elementwise against a bound derived from the arithmetic (`conv_bound`, `check_bound`).

Error model of the bound, with u = 2^-24 (fp32 unit roundoff) and K = KH*KW*Cin:
  an fp32 dot product of length K in any summation order errs by at most gamma_K * sum|x_i w_i|, gamma_K = K u / (1 - K u)
  (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; products of fp32 or bf16 operands are exact or rounded once,
  both inside the model); each of the bias add, the residual add and the ReLU adds at most u * |its result|; an output rounded to a
  16-bit type adds half an ulp of that type (2^-8 relative for bf16, 2^-11 for f16) of the computed value plus the type's smallest
  subnormal; fp32 outputs add the smallest fp32 subnormal.

SiLU (common.hpp silu_fast: x * v_rcp_f32(1 + v_exp_f32(x * fl(-log2 e))), both transcendentals 1 ulp = 2 u relative at most):
  t = fl(x c) with c = fl(-log2 e): the constant's rounding and the product's each perturb t by u |t|, so 2^t moves by a relative
  ln2 * 2 u |t| = 2 u |x|; v_exp adds 2 u.  e = 2^t enters 1 + e with weight e / (1 + e) = sigmoid(-x) <= 1; the add rounds (u), v_rcp
  adds 2 u, the final product u.  Relative error of silu_fast at an exact argument: <= 2 u (|x| + 1) + 4 u, i.e. 22 u for |x| <= 8;
  SILU_RHO = 24 u covers the second-order terms.  An argument that is itself off by eps moves silu by at most 1.1 eps (max |silu'| =
  1.0999).  The tests assert |pre-activation| <= SILU_XMAX so the constant holds."""

import dataclasses
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
SILU_XMAX = 8.0
SILU_RHO = 24 * U
SILU_LIP = 1.1
HALF_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.float32: 2.0 ** -149, torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24}
ACTS = ("none", "relu", "res_relu", "silu", "silu_res")


@dataclasses.dataclass(frozen=True)
class ConvCase:
    name: str
    B: int
    H: int
    W: int
    Cin: int
    Cout: int
    k: int
    stride: int
    pad: int
    act: str = "none"           # none | relu | res_relu | silu | silu_res (SiLU before the residual add, ReLU after it)
    sliced: bool = False        # channel-slice addressing on input, output and residual (offsets multiples of 4, not of 32)
    why: str = ""

    @property
    def OH(self):
        return (self.H + 2 * self.pad - self.k) // self.stride + 1

    @property
    def OW(self):
        return (self.W + 2 * self.pad - self.k) // self.stride + 1

    @property
    def M(self):
        return self.B * self.OH * self.OW

    @property
    def K(self):
        return self.k * self.k * self.Cin

    @property
    def has_res(self):
        return self.act in ("res_relu", "silu_res")

    @property
    def silu(self):
        return self.act in ("silu", "silu_res")

    @property
    def relu(self):
        return self.act in ("relu", "res_relu")

    def slices(self):
        """(in_ld, in_off, out_ld, out_off, res_ld, res_off); 0 = dense."""
        if not self.sliced:
            return (0, 0, 0, 0, 0, 0)
        return (self.Cin + 12, 4, self.Cout + 24, 20, self.Cout + 8, 4)


def conv_data(case, kind, seed=0):
    """x [B,Cin,H,W], w [Cout,Cin,k,k], bias [Cout], resid [B,Cout,OH,OW] or None, all fp32.  The last row of image b is bright and the
    first row of image b + 1 dark: a window that crossed the image boundary instead of reading padding would read the neighbour."""
    g = torch.Generator().manual_seed(1000 + seed + sum(map(ord, case.name)))
    xs, ws = (case.B, case.Cin, case.H, case.W), (case.Cout, case.Cin, case.k, case.k)
    rs = (case.B, case.Cout, case.OH, case.OW)
    if kind == "exact":
        x = torch.randint(-3, 4, xs, generator=g).float()
        w = torch.randint(-1, 2, ws, generator=g).float()
        bias = torch.randint(-4, 5, (case.Cout,), generator=g).float()
        resid = torch.randint(-8, 9, rs, generator=g).float() if case.has_res else None
        x[:, :, -1, :] = 3.0
        x[1:, :, 0, :] = -3.0
    else:
        # SiLU cases: pre-activations inside +-SILU_XMAX (asserted by conv_bound): weights scaled by 0.6 / sqrt(K)
        x = torch.randn(xs, generator=g)
        w = torch.randn(ws, generator=g) * (0.6 / math.sqrt(case.K))
        bias = torch.randn(case.Cout, generator=g) * 0.5
        resid = torch.randn(rs, generator=g) if case.has_res else None
        x[:, :, -1, :] += 1.5
        x[1:, :, 0, :] -= 1.5
    return x, w, bias, resid


def round_to(t, dtype):
    """Operand rounding of a kernel's contract: fp32 values rounded once (nearest even) to `dtype`, returned as fp32."""
    return t if dtype is None or dtype == torch.float32 else t.to(dtype).float()


def conv_acc(case, x, w, pad=None):
    """float64 convolution sums [B,Cout,OH,OW] (no bias)."""
    p = case.pad if pad is None else pad
    return F.conv2d(x.double(), w.double(), None, case.stride, p)[:, :, :case.OH, :case.OW]


def conv_finish(case, acc, bias, resid, relu_before_add=False):
    y = acc + bias.double().view(1, -1, 1, 1)
    if case.silu:
        y = y * torch.sigmoid(y)
    if relu_before_add and case.relu:
        y = F.relu(y)
    if resid is not None:
        y = y + resid.double()
    if case.relu and not relu_before_add:
        y = F.relu(y)
    return y


def conv_reference(case, x, w, bias, resid, operand=None):
    """float64 result of the operator on operands rounded to `operand` (None = fp32 operands as they are; bias stays fp32; the residual is
    passed in the values the kernel reads).  Returns (y, sabs): sabs = float64 sum of |x||w| per output."""
    xr, wr = round_to(x, operand), round_to(w, operand)
    y = conv_finish(case, conv_acc(case, xr, wr), bias, resid)
    sabs = conv_acc(case, xr.abs(), wr.abs())
    return y, sabs


def conv_bound(case, x, w, bias, resid, operand=None, out_dtype=torch.float32):
    """Elementwise bound on |kernel - float64 reference| from the module docstring's model."""
    xr, wr = round_to(x, operand), round_to(w, operand)
    K = case.K
    assert K * U < 0.01
    gamma = K * U / (1 - K * U)
    acc = conv_acc(case, xr, wr)
    e = gamma * conv_acc(case, xr.abs(), wr.abs())
    y = acc + bias.double().view(1, -1, 1, 1)
    e = e + U * y.abs()                                    # the bias add
    if case.silu:
        assert y.abs().max().item() + e.max().item() <= SILU_XMAX, "SiLU case outside the range its constant is derived for"
        y = y * torch.sigmoid(y)
        e = SILU_LIP * e + SILU_RHO * y.abs()
    if resid is not None:
        y = y + resid.double()
        e = e + U * y.abs()                                # the residual add
    if case.relu:
        y = F.relu(y)
        e = e + U * y.abs()                                # the ReLU (exact in every kernel; kept for the issue's accounting)
    h = HALF_ULP[out_dtype]
    return e * (1 + h) + h * y.abs() + TINY[out_dtype]


def assert_exact_premise(sabs, bias=None, resid=None):
    """The exact-data premise: every partial sum of every output is an integer below 2^24 in magnitude."""
    top = sabs.max().item() + (bias.abs().max().item() if bias is not None else 0) + (resid.abs().max().item() if resid is not None else 0)
    assert top < 2 ** 24, f"exact-data premise broken: sum |x||w| reaches {top}"


class Mismatch(AssertionError):
    pass


def check_exact(got, ref64, what=""):
    """Bit equality of `got` with the float64 reference cast to got's type (NaN payloads aside: a NaN matches a NaN)."""
    want = ref64.to(got.dtype)
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    same = (got == want) | (got.isnan() & want.isnan())
    # -0.0 == +0.0 compares equal; the sign of a zero is part of the bit pattern only where the reference is non-zero-signed exactly
    if not bool(same.all()):
        bad = (~same).nonzero()
        i = tuple(bad[0].tolist())
        raise Mismatch(f"{what}: {bad.shape[0]} of {same.numel()} elements differ; first at {i}: got {got[i].item()!r}, want {want[i].item()!r}")


def check_bound(got, ref64, bound, what=""):
    """Every element of `got` within `bound` of the float64 reference (a NaN or inf in `got` fails).  Returns the largest error / bound."""
    assert got.shape == ref64.shape == bound.shape, f"{what}: shapes {tuple(got.shape)} {tuple(ref64.shape)} {tuple(bound.shape)}"
    err = (got.double() - ref64).abs()
    ok = err <= bound                                       # NaN compares false
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise Mismatch(f"{what}: {bad.shape[0]} of {ok.numel()} elements outside the bound; first at {i}: got {got[i].item()!r}, "
                       f"reference {ref64[i].item()!r}, error {err[i].item():.3e} > bound {bound[i].item():.3e}")
    return (err / bound).max().item()


# ---------------------------------------------------------------------------------------------------------------------------------
# mutants: the float64 reference corrupted the way a kernel could be wrong (tests/test_convops_host.py)

def stage_len(case, operand16):
    """k values of the LAST K-stage: 32 (fp32 operands), 64 (16-bit), or the live part of a zero-padded last stage (K % 64)."""
    if not operand16:
        return 32
    return case.K % 64 or 64


def conv_mutants(case, x, w, bias, resid, operand=None):
    """{name: float64 result of a wrong kernel}; only the mutations that apply to the geometry."""
    xr, wr = round_to(x, operand), round_to(w, operand)
    acc = conv_acc(case, xr, wr)
    out = {}
    # one border tap dropped: the outputs of the last column lose the tap over the window's own pixel (inside the image in every geometry)
    c = min(case.pad, case.k - 1)
    wt = torch.zeros_like(wr)
    wt[:, :, c, c] = wr[:, :, c, c]
    a = acc.clone()
    a[:, :, :, -1] -= conv_acc(case, xr, wt)[:, :, :, -1]
    out["border_tap_dropped"] = conv_finish(case, a, bias, resid)
    # padding off by one: every window starts one pixel early
    out["pad_off_by_one"] = conv_finish(case, conv_acc(case, xr, wr, pad=case.pad + 1), bias, resid)
    if case.k > 1 and max(case.H, case.W) > 1:              # (a 1x1 map sees the centre tap only)
        out["ky_kx_swapped"] = conv_finish(case, conv_acc(case, xr, wr.transpose(2, 3)), bias, resid)
    n = stage_len(case, operand is not None)
    if n <= case.Cin and case.k - 1 - case.pad < min(case.H, case.W):   # (the last tap lies inside the image for some output)
        wl = wr.clone()
        wl[:, case.Cin - n:, -1, -1] = 0
        out["last_k_stage_skipped"] = conv_finish(case, conv_acc(case, xr, wl), bias, resid)
    if resid is not None:
        out["residual_slice_shifted_4"] = conv_finish(case, acc, bias, torch.roll(resid, 4, dims=1))
        if case.relu:
            out["relu_before_add"] = conv_finish(case, acc, bias, resid, relu_before_add=True)
    y = conv_finish(case, acc, bias, resid)
    if case.M >= 2:
        ym = y.permute(0, 2, 3, 1).reshape(case.M, case.Cout).clone()
        ym[-1] = ym[-2]
        out["last_pixel_copied"] = ym.reshape(case.B, case.OH, case.OW, case.Cout).permute(0, 3, 1, 2)
    if operand is not None:
        out["operand_rounding_left_out"] = conv_finish(case, conv_acc(case, x, w), bias, resid)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# geometries (the GPU tests add the ones whose size follows from the device's CU count: dispatch_cases)

def _c(name, B, H, W, Cin, Cout, k, s, p, act="none", sliced=False, why=""):
    return ConvCase(name, B, H, W, Cin, Cout, k, s, p, act, sliced, why)


def conv2d_cases():
    cs = []
    for co in (4, 32, 36, 64, 68, 128, 132, 252):
        cs.append(_c(f"cout{co}", 1, 3, 43, 32, co, 1, 1, 0, "relu", why="each channel tile with and without clamped weight rows / masked columns; M = 129"))
    for m in (1, 127, 128, 129):
        cs.append(_c(f"m{m}", 1, 1, m, 32, 36, 3, 1, 1, "relu", why="pixel-tile tails: one pixel, one short of / exactly / one past a tile"))
    for s in (1, 2):
        for (h, w_) in ((1, 1), (2, 2), (7, 7), (8, 8), (5, 12)):
            cs.append(_c(f"k3s{s}_{h}x{w_}", 2, h, w_, 32, 36, 3, s, 1, "res_relu", why="3x3 windows over tiny, odd, even and non-square maps; B = 2: "
                         "the neighbouring image must never be read for padding"))
    cs.append(_c("k1s2_7x7", 2, 7, 7, 64, 128, 1, 2, 0, "none", why="the downsample shortcut on an odd map"))
    cs.append(_c("cin64", 1, 7, 7, 64, 32, 3, 1, 1, "relu", why="two K-stages per tap"))
    cs.append(_c("cin96", 1, 7, 7, 96, 32, 3, 1, 1, "relu", why="tap_advance wrapping at a non-power-of-two channel count"))
    cs.append(_c("cin96_k1", 1, 7, 7, 96, 64, 1, 1, 0, "relu", why="bf16 operands: K = 96, the zero tail of the last stage is live"))
    cs.append(_c("cin160_k1", 2, 9, 9, 160, 64, 1, 1, 0, "relu", why="the stem's im2col rows run as a 1x1"))
    for act in ACTS:
        cs.append(_c(f"act_{act}", 2, 5, 12, 32, 68, 3, 1, 1, act, why="every epilogue: SiLU before the residual add, ReLU after it"))
    for act in ("relu", "res_relu", "silu", "silu_res"):
        cs.append(_c(f"sliced_{act}", 2, 5, 12, 32, 68, 3, 2, 1, act, True, why="channel-slice addressing on all three tensors (YOLO concatenations)"))
    cs.append(_c("sliced_k1", 1, 3, 43, 64, 36, 1, 1, 0, "res_relu", True, why="slices with a partly filled pixel tile and masked channel columns"))
    return cs


def dispatch_cases(cus):
    """1x1 32 -> 128 layers of g pixel tiles around the window (cus / 2, cus] in which conv2d_nhwc runs 64-channel tiles instead of 128;
    the last is also the case of several hundred tiles.  (name, case, expected channel tile)."""
    out = []
    for g, nw in ((cus // 2, 128), (cus // 2 + 1, 64), (cus, 64), (cus + 1, 128)):
        out.append((_c(f"tiles{g}", 1, 1, g * 128 - 3, 32, 128, 1, 1, 0, "relu", why="the 128 -> 64 channel-tile switch between half a round and a round of CUs"), nw))
    return out


def splitk_cases():
    return [_c("splitk_7x7x512", 1, 7, 7, 512, 512, 3, 1, 1, "res_relu", why="a deep, small-map layer: few tiles, 144 K-stages"),
            _c("splitk_silu", 1, 4, 4, 256, 64, 3, 1, 1, "silu_res", why="the reduction kernel's SiLU + residual epilogue"),
            _c("splitk_sliced", 2, 3, 3, 288, 36, 3, 1, 1, "res_relu", True, why="the reduction kernel's slice addressing; 81 stages")]


def conv16_cases():
    cs = []
    for ci, co in ((64, 64), (64, 128), (64, 192), (128, 64), (192, 128)):
        cs.append(_c(f"c{ci}_{co}", 2, 7, 7, ci, co, 3, 1, 1, "res_relu", why="both channel tiles (Cout % 128) and one to three K-stages per tap"))
    cs.append(_c("wide2048", 2, 7, 7, 64, 2048, 1, 1, 0, "res_relu", why="the 2048-wide 1x1 of resnet50's last stage"))
    for m in (1, 127, 128, 129):
        cs.append(_c(f"m{m}", 1, 1, m, 64, 64, 3, 1, 1, "relu", why="pixel-tile tails"))
    for s in (1, 2):
        for (h, w_) in ((1, 1), (2, 2), (7, 7), (8, 8), (5, 12)):
            cs.append(_c(f"k3s{s}_{h}x{w_}", 2, h, w_, 64, 64, 3, s, 1, "res_relu", why="3x3 windows over tiny, odd, even and non-square maps, B = 2"))
    cs.append(_c("k1s2_7x7", 2, 7, 7, 128, 128, 1, 2, 0, "none", why="the downsample shortcut on an odd map"))
    cs.append(_c("act_relu", 2, 5, 12, 64, 64, 3, 1, 1, "relu", why="ReLU without a residual"))
    cs.append(_c("act_none", 2, 5, 12, 64, 64, 3, 1, 1, "none", why="no epilogue but the bias"))
    return cs


# ---------------------------------------------------------------------------------------------------------------------------------
# layouts

def to_nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def pack_w(w):
    """[Cout,Cin,KH,KW] -> [Cout][ky][kx][ci]."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def pack_w16(w):
    """bf16 weight rows zero-padded to a multiple of 64 (ConvArgs::w16)."""
    p = pack_w(w)
    Kp = (p.shape[1] + 63) // 64 * 64
    o = torch.zeros(p.shape[0], Kp, dtype=torch.bfloat16)
    o[:, :p.shape[1]] = p.to(torch.bfloat16)
    return o


def unfold_ref(x, k, stride, pad, kpad):
    """im2col rows [B*OH*OW][kpad] with column (ky*k + kx)*Cin + c, built from F.pad + unfold; pad columns zero."""
    B, C, H, W = x.shape
    xp = F.pad(x, (pad, pad, pad, pad))
    u = xp.unfold(2, k, stride).unfold(3, k, stride)       # [B, C, OH, OW, ky, kx]
    OH, OW = u.shape[2], u.shape[3]
    rows = u.permute(0, 2, 3, 4, 5, 1).reshape(B * OH * OW, k * k * C)
    out = torch.zeros(B * OH * OW, kpad, dtype=x.dtype)
    out[:, :k * k * C] = rows
    return out
