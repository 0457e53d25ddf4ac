"""Float64 restatements, test data, derived error bounds and mutants of the six operators of csrc/mnv3g.hip (mg_stem, mg_dw, mg_se_gate,
mg_pw, mg_pool, mg_finish), on caller-made tensors in the kernels' own layouts (fp32, channels-last).  tests/test_gpu_mobilenetv3_ops.py
runs the kernels against them on the GPU; tests/test_mobilenetv3_ops_host.py proves on the CPU that every bound rejects every mutant and
admits a float32 evaluation.  Comparison functions and the SiLU constants are tests/convops_ref.py's.

Error model (convops_ref's), u = 2^-24, gamma_n = n u / (1 - n u):
  * an fp32 sum of n products (or terms) in ANY order errs by at most gamma_n * sum |terms|; a bias the chain starts from is one more term;
  * every further fp32 operation (bias add, residual add, a product with the gate, a division by the pixel count) adds u * |its result|;
  * an error e in front of an activation leaves it as L e + rho |act(y)|:  ReLU L = 1, rho = u (exact in the kernels; kept as the few u
    the accounting allows);  hard-swish y * clamp(y + 3, 0, 6) / 6: L = max |(2 y + 3) / 6| = 1.5, rho = 4 u (add, divide, multiply, each
    relative in the region where the clamp is live);  hard-sigmoid: L = 1 / 6, rho = 3 u;  SiLU: SILU_LIP, SILU_RHO inside +-SILU_XMAX.
  * mg_pw's 16-bit modes: the weights handed over are exactly representable in the operand type, the fp32 activation x enters as
    hi = rn16(x) plus lo = rn16(x - hi).  x - hi is exact in fp32 and at most half an ulp16 of x, so lo's rounding leaves a remainder of at
    most 2^-17 |x| (bf16, 8 significant bits) or 2^-23 |x| (f16, 11 bits; SPLIT uses 2^-22) as long as lo is not a subnormal f16 coarser
    than that: f16 subnormals are 2^-24 apart, so |x| >= 2^-3 keeps the remainder under 2^-22 |x| (`assert_split_premise`).  The products
    hi w and lo w are exact in fp32; 2 K of them are accumulated in an unspecified order: gamma_2K * sum (|hi| + |lo|) |w|, with
    |hi| + |lo| <= (1 + 2^-7) |x|."""
import dataclasses
import math

import torch
import torch.nn.functional as F

from tests.convops_ref import SILU_LIP, SILU_RHO, SILU_XMAX, TINY, U, round_to

ACT_NONE, ACT_RELU, ACT_HS, ACT_SILU = 0, 1, 2, 3
ACT_NAME = {ACT_NONE: "none", ACT_RELU: "relu", ACT_HS: "hs", ACT_SILU: "silu"}
HS_LIP, HS_RHO = 1.5, 4 * U
HSIG_LIP, HSIG_RHO = 1.0 / 6.0, 3 * U
DTYPE = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
SPLIT = {"fp32": 0.0, "bf16": 2.0 ** -17, "fp16": 2.0 ** -22}
FP16_SPLIT_MIN = 2.0 ** -3
TINY32 = TINY[torch.float32]


def gamma(n):
    assert n * U < 0.01
    return n * U / (1 - n * U)


def act64(y, act):
    if act == ACT_RELU:
        return F.relu(y)
    if act == ACT_HS:
        return F.hardswish(y)
    if act == ACT_SILU:
        return y * torch.sigmoid(y)
    return y


def act_bound(y, e, act):
    """(act(y), bound on the error behind the activation) for a pre-activation y known to within e."""
    a = act64(y, act)
    if act == ACT_RELU:
        return a, e + U * a.abs()
    if act == ACT_HS:
        return a, HS_LIP * e + HS_RHO * a.abs()
    if act == ACT_SILU:
        assert y.abs().max().item() + e.max().item() <= SILU_XMAX, "SiLU case outside the range its constant is derived for"
        return a, SILU_LIP * e + SILU_RHO * a.abs()
    return a, e


def _gen(*key):
    return torch.Generator().manual_seed(7919 + sum((i + 1) * int(k) for i, k in enumerate(key)))


# ------------------------------------------------------------------------------------------------------------------------ mg_stem
STEM_CASES = [(10, 2), (32, 3)]                                 # (S, B): a map that is mostly border; several workgroups


def stem_data(S, B):
    g = _gen(1, S, B)
    x = torch.randn(B, 3, S, S, generator=g)
    x[:, :, -1, :] += 1.5                                       # the last row of crop b bright, the first row of crop b + 1 dark
    x[1:, :, 0, :] -= 1.5
    return dict(x=x, w=torch.randn(16, 3, 3, 3, generator=g) / 27 ** 0.5, b=torch.randn(16, generator=g) * 0.5)


def _conv_cl(x, w, b, stride, pad, groups, Ho, late=0):
    """float64 conv on NCHW x, result channels-last [B,Ho,Ho,C]; `late`: every window starts that many pixels later."""
    k = w.shape[-1]
    xp = F.pad(x.double(), (pad, k + late, pad, k + late))[:, :, late:, late:]
    y = F.conv2d(xp, w.double(), None if b is None else b.double(), stride=stride, groups=groups)
    return y[:, :, :Ho, :Ho].permute(0, 2, 3, 1).contiguous()


def stem_pre(d, w=None, pad=1, late=0):
    S = d["x"].shape[-1]
    return _conv_cl(d["x"], d["w"] if w is None else w, d["b"], 2, pad, 1, S // 2, late)


def stem_ref(d):
    return F.hardswish(stem_pre(d))


def stem_bound(d):
    S = d["x"].shape[-1]
    sabs = _conv_cl(d["x"].abs(), d["w"].abs(), d["b"].abs(), 2, 1, 1, S // 2)
    y, e = act_bound(stem_pre(d), gamma(28) * sabs, ACT_HS)
    return e + TINY32


def stem_f32(d):
    y = F.conv2d(d["x"], d["w"], d["b"], stride=2, padding=1)
    return F.hardswish(y).permute(0, 2, 3, 1).contiguous()


def stem_mutants(d):
    return {"taps_transposed": F.hardswish(stem_pre(d, w=d["w"].transpose(2, 3))),
            "pad_off_by_one": F.hardswish(stem_pre(d, pad=2)),
            "window_one_pixel_late": F.hardswish(stem_pre(d, late=1))}


def pack_stem_w(w):
    return w.reshape(16, 27).T.contiguous()                     # [(ci, ky, kx)][16]


# ------------------------------------------------------------------------------------------------------------------------ mg_dw
@dataclasses.dataclass(frozen=True)
class DwCase:
    B: int
    C: int
    H: int
    k: int
    stride: int
    act: int

    @property
    def Ho(self):
        return (self.H - 1) // self.stride + 1

    @property
    def name(self):
        return f"B{self.B}_C{self.C}_H{self.H}_k{self.k}_s{self.stride}_{ACT_NAME[self.act]}"


DW_CASES = [DwCase(3, 16, 16, 3, 2, ACT_RELU), DwCase(3, 72, 7, 5, 2, ACT_HS), DwCase(2, 96, 1, 5, 1, ACT_HS),
            DwCase(2, 40, 2, 5, 2, ACT_HS), DwCase(3, 24, 9, 3, 1, ACT_RELU)]


def dw_data(c):
    g = _gen(2, c.B, c.C, c.H, c.k, c.stride)
    x = torch.randn(c.B, c.H, c.H, c.C, generator=g)
    x[:, -1] += 1.5
    x[1:, 0] -= 1.5
    return dict(x=x, w=torch.randn(c.C, c.k, c.k, generator=g) / c.k, b=torch.randn(c.C, generator=g) * 0.5)


def dw_pre(c, d, w=None, pad=None, late=0, x=None, b=True):
    w = d["w"] if w is None else w
    x = d["x"] if x is None else x
    return _conv_cl(x.permute(0, 3, 1, 2), w[:, None], d["b"] if b is True else b, c.stride, c.k // 2 if pad is None else pad, c.C,
                    c.Ho, late)


def dw_ref(c, d):
    return act64(dw_pre(c, d), c.act)


def dw_bound(c, d):
    sabs = dw_pre(c, d, w=d["w"].abs(), x=d["x"].abs(), b=d["b"].abs())
    y, e = act_bound(dw_pre(c, d), gamma(c.k * c.k + 1) * sabs, c.act)
    return e + TINY32


def dw_f32(c, d):
    y = F.conv2d(d["x"].permute(0, 3, 1, 2), d["w"][:, None], d["b"], stride=c.stride, padding=c.k // 2, groups=c.C)
    return act64(y, c.act).permute(0, 2, 3, 1).contiguous()


def dw_mutants(c, d):
    out = {"pad_off_by_one": act64(dw_pre(c, d, pad=c.k // 2 + 1), c.act)}
    if c.H > 1:                                                 # (a 1x1 map sees the centre tap only)
        out["taps_transposed"] = act64(dw_pre(c, d, w=d["w"].transpose(1, 2)), c.act)
    if c.stride == 2:
        out["window_one_pixel_late"] = act64(dw_pre(c, d, late=1), c.act)
    return out


def pack_dw_w(w):
    C, k, _ = w.shape
    return w.reshape(C, k * k).T.contiguous()                   # [ky * k + kx][C]


# ------------------------------------------------------------------------------------------------------------------------ mg_se_gate
# (B, C, R, HW): 16-lane channel groups; 32-lane groups with idle lanes; 64-lane groups; fewer pixels than groups; R > 128; the caps
SE_CASES = [(3, 16, 8, 64), (3, 24, 8, 49), (2, 72, 24, 49), (2, 960, 240, 1), (2, 672, 168, 4), (1, 1024, 256, 9)]
SE_REFUSED = [(1, 1028, 8, 4), (1, 16, 260, 4)]


def se_data(B, C, R, HW):
    g = _gen(3, B, C, R, HW)
    t = torch.randn(B, HW, C, generator=g) + torch.linspace(-1, 1, C)      # channel means differ, and differ between crops
    t[1:] += 0.7
    return dict(t=t, wr=torch.randn(R, C, generator=g) / C ** 0.5, br=torch.randn(R, generator=g) * 0.3,
                we=torch.randn(C, R, generator=g) * (2.0 / R ** 0.5), be=torch.randn(C, generator=g) * 0.3)


def se_ref(d, mean=None, wr=None, we=None):
    t = d["t"].double()
    m = t.mean(1) if mean is None else mean
    wr = d["wr"].double() if wr is None else wr
    we = d["we"].double() if we is None else we
    h = F.relu(m @ wr.T + d["br"].double())
    return F.hardsigmoid(h @ we.T + d["be"].double())


def se_bound(d):
    t = d["t"].double()
    HW, C = t.shape[1:]
    R = d["wr"].shape[0]
    wr, we = d["wr"].double(), d["we"].double()
    m = t.mean(1)
    e_m = gamma(HW) * t.abs().mean(1) + U * m.abs()
    s = m @ wr.T + d["br"].double()
    e_h = gamma(C + 1) * (m.abs() @ wr.abs().T + d["br"].double().abs()) + e_m @ wr.abs().T
    h, e_h = act_bound(s, e_h, ACT_RELU)
    z = h @ we.T + d["be"].double()
    e_z = gamma(R + 1) * (h @ we.abs().T + d["be"].double().abs()) + e_h @ we.abs().T
    return HSIG_LIP * e_z + HSIG_RHO * F.hardsigmoid(z) + TINY32


def se_f32(d):
    m = d["t"].mean(1)
    return F.hardsigmoid(F.relu(m @ d["wr"].T + d["br"]) @ d["we"].T + d["be"])


def se_mutants(d):
    t = d["t"].double()
    B, HW, C = t.shape
    R = d["wr"].shape[0]
    out = {"mean_drops_last_pixel": se_ref(d, mean=t[:, :-1].sum(1) / HW),
           "reduce_weight_transposed": se_ref(d, wr=d["wr"].double().reshape(C, R).T),
           "expand_weight_transposed": se_ref(d, we=d["we"].double().reshape(R, C).T)}
    if B > 1:
        out["mean_of_neighbouring_crop"] = se_ref(d, mean=torch.roll(t.mean(1), 1, 0))
    return out


# ------------------------------------------------------------------------------------------------------------------------ mg_pw
@dataclasses.dataclass(frozen=True)
class PwCase:
    M: int
    K: int
    N: int
    HW: int
    gate: bool
    resid: bool
    act: int
    why: str = ""

    @property
    def name(self):
        return f"M{self.M}_K{self.K}_N{self.N}_HW{self.HW}_{'g' if self.gate else ''}{'r' if self.resid else ''}_{ACT_NAME[self.act]}"

    @property
    def crops(self):
        return -(-self.M // self.HW)


PW_CASES = [
    PwCase(1, 8, 16, 1, False, False, ACT_HS, "Kp = 16 with three of four k-quads outside K"),
    PwCase(147, 24, 40, 49, True, True, ACT_NONE, "three crops; waves straddle crop borders; last workgroup 19 live rows; n-tile 2 half-filled"),
    PwCase(20, 72, 24, 4, True, False, ACT_NONE, "five crops inside one wave's rows; K tail of 8"),
    PwCase(3, 960, 1280, 1, False, False, ACT_HS, "the head: 20 block columns"),
    PwCase(65, 40, 88, 65, False, True, ACT_RELU, "second block column with two absent tiles; one row in the second workgroup"),
    PwCase(64, 16, 16, 16, True, False, ACT_SILU, "EfficientNet's form"),
]


def pw_data(c, prec):
    """a with 0.25 <= |a| and gates in [0.5, 1]: |a g| >= 2^-3, the f16 split's premise.  w holds the values the kernel is handed: rounded
    once to the operand type (exactly representable there)."""
    g = _gen(4, c.M, c.K, c.N, c.HW)
    a = torch.randn(c.M, c.K, generator=g)
    a = torch.where(a < 0, a - 0.25, a + 0.25)
    w = torch.randn(c.N, c.K, generator=g) * (0.6 / math.sqrt(c.K))
    # Row 0 against channel N - 3: 1 + j 2^-7 (exact in both 16-bit types) plus a remainder of 0.9 * 2^-11, below f16's half ulp, and
    # weights of one sign.  A kernel that rounds the activation to 16 bits errs by 0.9 * 2^-11 sum |a||w| there, all terms aligned: above
    # the accumulation term gamma_2K sum |a||w| up to K = 960, where random remainders (which add up like sqrt(K)) would hide under it.
    a[0] = 1.0 + torch.randint(0, 8, (c.K,), generator=g) * 2.0 ** -7 + 0.9 * 2.0 ** -11
    w[c.N - 3] = w[c.N - 3].abs()
    d = dict(a=a, w=round_to(w, DTYPE[prec]),
             bias=torch.randn(c.N, generator=g) * 0.5,
             gate=torch.rand(c.crops, c.K, generator=g) * 0.5 + 0.5 if c.gate else None,
             resid=torch.randn(c.M, c.N, generator=g) if c.resid else None)
    return d


def _gated(c, d, gate="own"):
    a = d["a"].double()
    if d["gate"] is None or gate is None:
        return a
    g = d["gate"].double()
    if gate == "neighbour":
        g = torch.roll(g, 1, 0)
    return a * g[torch.arange(c.M) // c.HW]


def assert_split_premise(c, d, prec):
    if prec == "fp16":
        x = (d["a"] * d["gate"][torch.arange(c.M) // c.HW]) if d["gate"] is not None else d["a"]
        assert x.abs().min().item() >= FP16_SPLIT_MIN, "an activation below 2^-3: f16's lo part may be a subnormal coarser than 2^-22 |x|"


def pw_finish(c, d, acc, resid="own", act_after_resid=False):
    y = acc + d["bias"].double()
    r = d["resid"].double() if (d["resid"] is not None and resid == "own") else None
    if act_after_resid and r is not None:
        return act64(y + r, c.act)
    y = act64(y, c.act)
    return y if r is None else y + r


def pw_ref(c, d):
    return pw_finish(c, d, _gated(c, d) @ d["w"].double().T)


def pw_bound(c, d, prec):
    assert_split_premise(c, d, prec)
    ag, w = _gated(c, d), d["w"].double()
    sabs = ag.abs() @ w.abs().T
    u_gate = U if d["gate"] is not None else 0.0
    if prec == "fp32":
        e = (gamma(c.K) + u_gate * (1 + gamma(c.K))) * sabs
    else:
        e = (gamma(2 * c.K) * (1 + 2.0 ** -7) + SPLIT[prec] + u_gate * (1 + 2.0 ** -7)) * sabs
    y = ag @ w.T + d["bias"].double()
    y, e = act_bound(y, e + U * y.abs(), c.act)
    if d["resid"] is not None:
        y = y + d["resid"].double()
        e = e + U * y.abs()
    return e + TINY32


def pw_f32(c, d):
    a = d["a"] if d["gate"] is None else d["a"] * d["gate"][torch.arange(c.M) // c.HW]
    y = act64(a @ d["w"].T + d["bias"], c.act)
    return y if d["resid"] is None else y + d["resid"]


def pw_mutants(c, d, prec):
    w = d["w"].double()
    acc = _gated(c, d) @ w.T
    out = {}
    if c.K % 16:
        wl = w.clone()
        wl[:, -4:] = 0
        out["last_k_quad_dropped"] = pw_finish(c, d, _gated(c, d) @ wl.T)
    if c.N % 16:
        y = pw_ref(c, d).clone()
        n0 = c.N // 16 * 16
        y[:, n0:] = torch.roll(y[:, n0:], 4, 1)
        out["last_n_tile_shifted_4"] = y
    if c.gate:
        out["gate_left_out"] = pw_finish(c, d, _gated(c, d, None) @ w.T)
        if c.crops > 1:
            out["gate_of_neighbouring_crop"] = pw_finish(c, d, _gated(c, d, "neighbour") @ w.T)
    if c.resid:
        out["residual_left_out"] = pw_finish(c, d, acc, resid=None)
        if c.act != ACT_NONE:
            out["activation_after_residual"] = pw_finish(c, d, acc, act_after_resid=True)
    if prec != "fp32":
        out["lo_part_dropped"] = pw_finish(c, d, _gated(c, d).float().to(DTYPE[prec]).double() @ w.T)
    return out


def pack_pw_w(w, prec):
    """The weight as the forward reads it: fp32 [N][K]; 16-bit [16 ceil(N / 16)][Kp], Kp = K rounded up to 16, zero padded."""
    if prec == "fp32":
        return w.contiguous()
    N, K = w.shape
    o = torch.zeros((N + 15) // 16 * 16, (K + 15) // 16 * 16, dtype=DTYPE[prec])
    o[:N, :K] = w.to(DTYPE[prec])
    assert torch.equal(o[:N, :K].float(), w), "the weight handed over is not exactly representable in the operand type"
    return o


# ------------------------------------------------------------------------------------------------------------------------ mg_pool
POOL_CASES = [(3, 1, 48), (3, 49, 960)]                         # (B, HW, C)


def pool_data(B, HW, C):
    g = _gen(5, B, HW, C)
    return dict(t=torch.randn(B, HW, C, generator=g) + torch.linspace(-1, 1, C))


def pool_ref(d, count=None):
    t = d["t"].double()
    return t.sum(1) / (t.shape[1] if count is None else count)


def pool_bound(d):
    t = d["t"].double()
    return gamma(t.shape[1]) * t.abs().mean(1) + U * t.mean(1).abs() + TINY32


def pool_f32(d):
    return d["t"].mean(1)


def pool_mutants(d):
    t = d["t"].double()
    HW = t.shape[1]
    return {"divided_by_wrong_count": pool_ref(d, HW + 1), "last_pixel_dropped": (t.sum(1) - t[:, -1]) / HW,
            "neighbouring_crop": torch.roll(pool_ref(d), 1, 0)}


# ------------------------------------------------------------------------------------------------------------------------ mg_finish
FINISH_DIMS = [1024, 1280]


def finish_data(D):
    """Rows: 0 and 2 ordinary (different scales), 1 all zero, 3 tiny (norm far below 1 but above the 1e-12 clamp).  The last column is
    large: a norm that misses it shows."""
    g = _gen(6, D)
    e = torch.randn(4, D, generator=g)
    e[:, -1] = 6.0
    return dict(e=e * torch.tensor([1.0, 0.0, 37.0, 1e-9])[:, None])


def finish_ref(d, l2, norm=None):
    e = d["e"].double()
    if not l2:
        return e
    n = e.norm(dim=1, keepdim=True) if norm is None else norm
    return e / n.clamp_min(1e-12)


def finish_bound(d, l2):
    e = d["e"].double()
    if not l2:
        return torch.zeros_like(e)                              # untouched: bit-equal
    D = e.shape[1]
    # sum of D squares in any order (one more u each for the squares): relative gamma_(D+1) on the sum, half of it behind the root;
    # sqrtf and the division at most 2 u each
    return (gamma(D + 1) + 4 * U) * finish_ref(d, l2).abs() + TINY32


def finish_f32(d, l2):
    return F.normalize(d["e"], dim=1) if l2 else d["e"]


def finish_mutants(d, l2):
    if not l2:
        return {}
    e = d["e"].double()
    return {"norm_misses_last_column": finish_ref(d, l2, norm=e[:, :-1].norm(dim=1, keepdim=True)),
            "norm_not_rooted": finish_ref(d, l2, norm=(e * e).sum(1, keepdim=True)),
            "norm_of_neighbouring_row": finish_ref(d, l2, norm=torch.roll(e.norm(dim=1, keepdim=True), 2, 0))}


# ------------------------------------------------------------------------------------------------------------------------ non-finite data
NONFINITE = {"nan": float("nan"), "inf": float("inf"), "-inf": float("-inf")}


def check_nonfinite(got, ref64, what=""):
    """The set of non-finite outputs and their values equal the reference's (a NaN matches a NaN, an inf an inf of the same sign)."""
    from tests.convops_ref import Mismatch
    want = ref64.to(got.dtype)
    assert got.shape == want.shape
    nf = ~torch.isfinite(got) | ~torch.isfinite(want)
    same = (got == want) | (got.isnan() & want.isnan())
    bad = nf & ~same
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise Mismatch(f"{what}: {int(bad.sum())} of {int(nf.sum())} non-finite outputs differ from torch; first at {i}: "
                       f"got {got[i].item()!r}, want {want[i].item()!r}")
    return int(nf.sum())
