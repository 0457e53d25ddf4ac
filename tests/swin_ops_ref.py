"""Float64 restatements, test data, derived error bounds and mutants of the operators of libeffocr_swin.so: the five kernels of
csrc/swin.hip (stem, layernorm, merge, window attention, head) and the linears of swin_forward (csrc/swin_api.hip: swin_linear), on
caller-made tensors in the kernels' own layouts.  tests/test_gpu_swin_ops.py runs the kernels against them through the
effocr_swin_op_* entry points; tests/test_swin_ops_host.py proves on the CPU that every bound admits a float32 evaluation and rejects
the mutants.  Comparison functions and the rounding constants are tests/convops_ref.py's; the window partition, the relative position
index and the region mask are tests/swin_ref.py's (pinned to transformers by tests/test_swin_host.py).

Every reference works on the REAL channels only ([..., :C]); the GPU test fills the pad channels of its inputs with NaN and asserts
the pad channels of the outputs to be exactly 0 on its own.

Error model (convops_ref's), u = 2^-24, gamma_n = n u / (1 - n u):
  * an fp32 dot product of n terms in ANY order errs by at most gamma_n sum |terms|; every further fp32 add or multiply adds
    u |its result|; a division, a square root, v_rcp and v_exp 2 u; a 16-bit store half an ulp of the type plus its smallest subnormal.
  * the LayerNorm sums of swin.hip are not "any order" but a tree: two levels inside the thread ((v0 + v1) + (v2 + v3)), five
    xor-shuffle levels inside the 32-lane half, then at most 12 halves in ascending order: depth <= 19.  A summation tree of depth D
    errs by at most gamma_D sum |terms| (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), so the statistics are
    bounded with gamma_LN_DEPTH, LN_DEPTH = 20 — far tighter than gamma_C at C = 1536, and what lets the bound see a one-pass variance.
  * LayerNorm (`ln_bound`), input x known to within ex:  mean: em = mean(ex) + gamma_D mean|x| + 2 u |mean| (the sum, the product with
    fl(1 / C));  d = x - mean: ed = ex + em + u |d|;  var: ev = gamma_(D+3) var + mean(2 |d| ed + ed^2);  rstd = 1 / sqrt(var + eps):
    er = the larger one-sided change of rstd under var +- (ev + 2 u (var + eps)), plus 4 u rstd (sqrt and division);
    y = d rstd g + b: ey = |g| (ed rstd + |d| er + ed er + 2 u |d| rstd) + u |y|.
  * softmax (`wa_bound`): q' = fl(q 32^-0.5) is off by 2 u |q'|; a score s = q' . k + table + mask by
    es = (gamma_32 + 2 u) sum |q' k| + u |q' . k + table| + u |s|.  Softmax is invariant under a common shift, so the kernel's maximum
    is as good as the true one: the argument x = s - max is off by ex = es + u (|x| + max es).  __expf(x) = v_exp_f32(x log2 e): relative
    rho = expm1(ex) + 2 u (|x| + ex + 1) + 2 u (convops_ref's SiLU argument), absolute 2^-126 where the result is a flushed subnormal.
    Sum of 49: gamma_48; reciprocal 2 u; weight product u: a weight w_j is off by relative pi_j = rho_j + sum_k rho_k w_k + gamma_48 + 3 u.
    P . V over 49 keys: sum_j (pi_j + gamma_49) w_j |v_j|.  The kernel rounds nothing to 16 bits between its loads and its store.
  * GELU: an error e in front of it leaves GELU_LIP e (max |gelu'| = 1.129); gelu(y) = 0.5 y (1 + erf(y / sqrt 2)) with the kernel's erf
    off by at most E absolute adds 0.5 |y| E, its three products and one add 4 u |gelu|.  16-bit modes run common.hpp's gelu_erf_fast,
    a polynomial whose distance to erf (`erf_fast_abs_error`, evaluated in float64 from the coefficients, clamp included) is E, plus
    16 u for its fp32 Horner steps and the rounding of its argument.  fp32 runs libm's erff, which cannot be bounded from the
    project's source: ERF_F32_ABS is measured (see the constant), and the bound term is twice it."""
import math

import torch
import torch.nn.functional as F

from tests.convops_ref import HALF_ULP, TINY, U, round_to
from tests.swin_ref import region_mask, relative_index, unwindows, windows

EPS = 1e-5
LN_DEPTH = 20
WS, NW, HD = 7, 49, 32
SCALE = HD ** -0.5
DTYPE = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
PRECS = ["fp32", "fp16", "bf16"]
TINY32 = TINY[torch.float32]
FLUSH = 2.0 ** -126
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_BIAS_F32 = 0, 1, 2, 5
EPI_NAME = {EPI_BIAS: "bias", EPI_BIAS_GELU: "gelu", EPI_BIAS_RESID: "resid", EPI_BIAS_F32: "f32"}
GELU_LIP = 1.13
# Worst |kernel gelu(x) - float64 gelu(x)| / (0.5 |x|) of the fp32 GELU epilogue (gemm.hip: gelu_erf, libm erff) over 240001 points of
# [-6, 6], i.e. the absolute error of its (1 + erf) factor, erff's own error and the factor's roundings together.  Measured on an MI355X
# through effocr_swin_op_linear with an identity weight against float64 torch.erf: 2.195e-07 = 3.68 u, recorded in
# profiles/swin_ops_parity.txt.  The bound term is twice it; tests/test_gpu_swin_ops.py::test_erf_f32_measured_constant_holds
# re-measures it and fails if the kernel's error leaves that term.
ERF_F32_ABS = 2.195e-07


def gamma(n):
    assert n * U < 0.01
    return n * U / (1 - n * U)


def _gen(*key):
    return torch.Generator().manual_seed(104729 + sum((i + 1) * 131 ** i * int(k) for i, k in enumerate(key)) % (2 ** 31))


def stored(e, y, dtype):
    """Bound behind the store of y (known to within e) in `dtype`."""
    h = HALF_ULP[dtype]
    return e * (1 + h) + h * y.abs() + TINY[dtype]


def to_out(t, dtype):
    """A float32 evaluation stored in the output type, as float32."""
    return t.to(dtype).float()


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm
def ln64(x, g, b, eps=EPS, stats=None):
    """float64 LayerNorm over the last axis; stats = (mean, var) to use in place of the row's own."""
    x = x.double()
    mean, var = stats if stats is not None else (x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True))
    return (x - mean) / torch.sqrt(var + eps) * g.double() + b.double()


def ln_bound(x, ex, g, b, eps=EPS):
    """(y, ey): float64 LayerNorm of x and the bound on the kernel's fp32 result before its store, x known to within ex.
    eps: the kernel's epsilon (Swin's 1e-5 by default; tests/convnext_ops_ref.py passes ConvNeXt's 1e-6).  LN_DEPTH = 20 also holds for
    convnext.hip's seg_layernorm, whose tree is 2 levels in the thread + 5 in the half + at most 6 halves in order = 13 deep."""
    x, g, b = x.double(), g.double(), b.double()
    mean = x.mean(-1, keepdim=True)
    em = ex.mean(-1, keepdim=True) + gamma(LN_DEPTH) * x.abs().mean(-1, keepdim=True) + 2 * U * mean.abs()
    d = x - mean
    ed = ex + em + U * d.abs()
    var = (d * d).mean(-1, keepdim=True)
    ev = gamma(LN_DEPTH + 3) * var + (2 * d.abs() * ed + ed * ed).mean(-1, keepdim=True) + 2 * U * (var + eps)
    assert bool((ev < 0.5 * (var + eps)).all()), "LayerNorm data too ill-conditioned for a bound"
    rstd = 1 / torch.sqrt(var + eps)
    er = torch.maximum(1 / torch.sqrt(var + eps - ev) - rstd, rstd - 1 / torch.sqrt(var + eps + ev)) + 4 * U * rstd
    y = d * rstd * g + b
    ey = g.abs() * (ed * rstd + d.abs() * er + ed * er + 2 * U * d.abs() * rstd) + U * y.abs()
    return y, ey


def _tokens(M, C, g, kind="real"):
    """[M, C] fp32 rows of different scales (1, 0.01, 3, 0.3: eps matters in the small ones) and means; 'cancel': |mean| = 100 std."""
    scale = torch.tensor([1.0, 0.01, 3.0, 0.3])[torch.arange(M) % 4][:, None]
    if kind == "cancel":
        return scale * (100.0 + torch.randn(M, C, generator=g))
    off = torch.linspace(-1.0, 1.0, M)[:, None] if M > 1 else torch.full((1, 1), 0.4)
    return scale * (torch.randn(M, C, generator=g) + off + torch.linspace(-0.5, 0.5, C))


def _affine(n, g):
    return torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g) * 0.5


def pad_cols(t, Cp, fill=0.0):
    """[..., C] -> [..., Cp] with `fill` in the pad channels."""
    out = torch.full(t.shape[:-1] + (Cp,), fill, dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


# ------------------------------------------------------------------------------------------------------------------------ stem
# (S, B, C0): M = 4 in one part-filled block; M = 27 with a tail of 3 and crop borders inside a block; 98 tokens; no pad channels
STEM_CASES = [(8, 1, 96), (12, 3, 96), (28, 2, 96), (12, 2, 128)]


def stem_data(S, B, C0):
    g = _gen(1, S, B, C0)
    x = torch.randn(B, 3, S, S, generator=g)
    x[:, :, -1, :] += 1.5                                       # the last row of crop b bright, the first row of crop b + 1 dark
    x[1:, :, 0, :] -= 1.5
    lnw, lnb = _affine(C0, g)
    return dict(x=x, w=torch.randn(C0, 3, 4, 4, generator=g) / 48 ** 0.5, b=torch.randn(C0, generator=g) * 0.5, lnw=lnw, lnb=lnb)


def pack_stem(d):
    """(wt [48 taps (c, ky, kx)][128], b, lnw, lnb [128]) as pack_swin lays them out: zeros beyond C0."""
    C0 = d["w"].shape[0]
    wt = torch.zeros(48, 128)
    wt[:, :C0] = d["w"].reshape(C0, 48).T
    return wt, pad_cols(d["b"], 128), pad_cols(d["lnw"], 128), pad_cols(d["lnb"], 128)


def _stem_conv(x, w, b):
    y = F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride=4)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


def stem_ref(d, eps=EPS):
    return ln64(_stem_conv(d["x"], d["w"], d["b"]), d["lnw"], d["lnb"], eps)


def stem_bound(d, eps=EPS):
    ec = gamma(49) * _stem_conv(d["x"].abs(), d["w"].abs(), d["b"].abs())       # 48 FMAs on top of the bias
    y, ey = ln_bound(_stem_conv(d["x"], d["w"], d["b"]), ec, d["lnw"], d["lnb"], eps)
    return ey + TINY32


def stem_f32(d, eps=EPS):
    C0 = d["w"].shape[0]
    y = F.conv2d(d["x"], d["w"], d["b"], stride=4).permute(0, 2, 3, 1).reshape(-1, C0)
    return F.layer_norm(y, (C0,), d["lnw"], d["lnb"], eps)


def stem_mutants(d, eps=EPS):
    C0 = d["w"].shape[0]
    conv = _stem_conv(d["x"], d["w"], d["b"])
    out = {"ky_kx_swapped": ln64(_stem_conv(d["x"], d["w"].transpose(2, 3), d["b"]), d["lnw"], d["lnb"], eps),
           "channel_major_taps": ln64(_stem_conv(d["x"], pack_stem(d)[0].flatten().view(128, 48)[:C0].reshape(C0, 3, 4, 4), d["b"]),
                                      d["lnw"], d["lnb"], eps),
           "bias_after_norm": ln64(_stem_conv(d["x"], d["w"], None), d["lnw"], d["lnb"], eps) + d["b"].double()}
    if C0 < 128:
        p = pad_cols(conv, 128)
        out["norm_over_128"] = ln64(conv, d["lnw"], d["lnb"], eps, stats=(p.mean(-1, keepdim=True), p.var(-1, unbiased=False, keepdim=True)))
    return out


# ------------------------------------------------------------------------------------------------------------------------ layernorm
LN_SEGS = {128: 8, 256: 4, 384: 2, 768: 1, 1024: 1}            # tokens per workgroup (swin_layernorm)
LN_GEOM = [(96, 128), (192, 256), (384, 384), (768, 768), (1024, 1024)]
# (C, Cp, M, kind): one token (every other segment clamped to it); one token past two full workgroups; 37 tokens; |mean| = 100 std
LN_CASES = ([(C, Cp, 1, "real") for C, Cp in LN_GEOM] + [(C, Cp, 2 * LN_SEGS[Cp] + 1, "real") for C, Cp in LN_GEOM]
            + [(96, 128, 37, "real"), (96, 128, 17, "cancel")])


def ln_data(C, Cp, M, kind):
    g = _gen(2, C, Cp, M, kind == "cancel")
    lnw, lnb = _affine(C, g)
    return dict(x=_tokens(M, C, g, kind), lnw=lnw, lnb=lnb)


def ln_ref(d):
    return ln64(d["x"], d["lnw"], d["lnb"])


def ln_op_bound(d, prec):
    y, ey = ln_bound(d["x"], torch.zeros_like(d["x"], dtype=torch.float64), d["lnw"], d["lnb"])
    return stored(ey, y, DTYPE[prec])


def ln_f32(d, prec):
    return to_out(F.layer_norm(d["x"], d["x"].shape[-1:], d["lnw"], d["lnb"], EPS), DTYPE[prec])


def ln_mutants(d, Cp, kind="real"):
    x = d["x"].double()
    M, C = x.shape
    mean, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    out = {"unbiased_variance": ln64(x, d["lnw"], d["lnb"], stats=(mean, x.var(-1, unbiased=True, keepdim=True))),
           "eps_1e-6": ln64(x, d["lnw"], d["lnb"], eps=1e-6)}
    if C < Cp:
        p = pad_cols(x, Cp)
        out["statistics_over_Cp"] = ln64(x, d["lnw"], d["lnb"], stats=(p.mean(-1, keepdim=True), p.var(-1, unbiased=False, keepdim=True)))
    if M > 1:
        out["neighbouring_token_statistics"] = ln64(x, d["lnw"], d["lnb"], stats=(torch.roll(mean, 1, 0), torch.roll(var, 1, 0)))
    if kind == "cancel":
        x32 = d["x"]
        m32 = x32.mean(-1, keepdim=True)
        v32 = (x32 * x32).mean(-1, keepdim=True) - m32 * m32                    # E[x^2] - mean^2 in fp32
        out["one_pass_variance_fp32"] = ln64(x, d["lnw"], d["lnb"], stats=(m32.double(), v32.double().clamp_min(0)))
    return out


# ------------------------------------------------------------------------------------------------------------------------ merge
QUADRANTS = [(0, 0), (1, 0), (0, 1), (1, 1)]                    # (dy, dx): timm's [x(2i,2j), x(2i+1,2j), x(2i,2j+1), x(2i+1,2j+1)]
# (B, H, C, Cp): segs 2 with crop borders inside blocks; M = 49 odd; one 192-thread segment; 384 threads, hs[12]; 8 segments, M = 9
MERGE_CASES = [(3, 4, 96, 128), (1, 14, 96, 128), (3, 2, 192, 256), (2, 2, 384, 384), (1, 6, 32, 128)]


def merge_data(B, H, C, Cp):
    g = _gen(3, B, H, C, Cp)
    x = torch.randn(B, H, H, C, generator=g)
    x += torch.linspace(-1, 1, H)[None, :, None, None] + 0.5 * torch.linspace(-1, 1, H)[None, None, :, None] ** 3
    x += 0.4 * torch.arange(B)[:, None, None, None] + torch.linspace(-0.5, 0.5, C)
    lnw, lnb = _affine(4 * C, g)
    return dict(x=x, lnw=lnw, lnb=lnb)


def _gather(x, order=QUADRANTS):
    return torch.cat([x[:, dy::2, dx::2] for dy, dx in order], dim=-1).reshape(-1, 4 * x.shape[-1])


def merge_ref(d):
    return ln64(_gather(d["x"]), d["lnw"], d["lnb"])


def merge_bound(d, prec):
    r = _gather(d["x"])
    y, ey = ln_bound(r, torch.zeros_like(r, dtype=torch.float64), d["lnw"], d["lnb"])
    return stored(ey, y, DTYPE[prec])


def merge_f32(d, prec):
    r = _gather(d["x"])
    return to_out(F.layer_norm(r, r.shape[-1:], d["lnw"], d["lnb"], EPS), DTYPE[prec])


def merge_mutants(d, Cp):
    x = d["x"]
    B, H, _, C = x.shape
    g, b = d["lnw"], d["lnb"]
    r = _gather(x)
    out = {"quadrants_row_major": ln64(_gather(x, [(0, 0), (0, 1), (1, 0), (1, 1)]), g, b),
           "norm_per_quadrant": torch.cat([ln64(r[:, q * C:(q + 1) * C], g[q * C:(q + 1) * C], b[q * C:(q + 1) * C]) for q in range(4)], -1)}
    out["unbiased_variance"] = ln64(r, g, b, stats=(r.double().mean(-1, keepdim=True), r.double().var(-1, unbiased=True, keepdim=True)))
    late = x.clone()
    late[:, H - 1] = torch.roll(x[:, 0], -1, 0)                                 # row H of crop b = row 0 of crop b + 1
    out["last_row_from_next_crop"] = ln64(_gather(late), g, b)
    if C < Cp:
        out["row_stride_C_for_Cp"] = ln64(_gather(pad_cols(x, Cp).flatten()[:x.numel()].view(B, H, H, C)), g, b)
    return out


# ------------------------------------------------------------------------------------------------------------------------ window attention
# (B, H, shift, C, Cp): one window; 12 windows unshifted; four windows with four mask patterns (the last with all nine regions); an
# interior unmasked window beside masked ones; the launcher's extreme shifts without pad channels; 6 heads
WA_CASES = [(1, 7, 0, 96, 128), (3, 14, 0, 96, 128), (3, 14, 3, 96, 128), (1, 21, 3, 96, 128), (2, 14, 1, 64, 64), (2, 14, 6, 64, 64),
            (1, 14, 3, 192, 256)]
WA_KINDS = ["random", "zeroqk", "leak", "flat"]
WA_RUNS = [(c, k) for c in WA_CASES for k in WA_KINDS if k != "leak" or c[2]]     # no 'leak' without a shift: there is no mask to leak through
LEAK = 5.125            # 32 * 5.125^2 * 32^-0.5 = 148.6: a masked pair's score, 100 < 148.6 - (in-region scores, |.| < 45) < 200


def region_ids(H, shift, cuts=None):
    """[H, H] region id of every ROLLED position (data and mutants only: the reference's mask is swin_ref.region_mask)."""
    cuts = (H - WS, H - shift) if cuts is None else cuts
    r = sum((torch.arange(H) >= c).long() for c in cuts)
    return r[:, None] * 3 + r[None, :]


def _mask_of(ids, fill=-100.0):
    w = windows(ids.double().view(1, *ids.shape, 1), WS).squeeze(-1)
    dlt = w[:, None, :] - w[:, :, None]
    return torch.where(dlt != 0, torch.full_like(dlt, fill), torch.zeros_like(dlt))


def wa_data(case, kind, prec):
    """q, k, v [B, H, H, C] and table [169, heads], values already rounded to the operand type.
    leak: queries of region 8 (the corner [H-shift, H)^2 of the rolled map) and keys of every other region are the constant vector
    LEAK: such a pair scores 148.6 before the mask, 48.6 behind it, far above the in-region scores of that query — with -100 the masked
    keys carry the softmax, with a hard mask they carry nothing."""
    B, H, shift, C, Cp = case
    g = _gen(4, B, H, shift, C, WA_KINDS.index(kind))
    heads = C // HD
    q, k, v = (torch.randn(B, H, H, C, generator=g) for _ in range(3))
    v = v + torch.linspace(-1, 1, C) + 0.3 * torch.arange(B)[:, None, None, None] + torch.linspace(-0.7, 0.7, H)[None, :, None, None]
    table = torch.randn((2 * WS - 1) ** 2, heads, generator=g)
    if kind == "zeroqk":
        q, k, table = torch.zeros_like(q), torch.zeros_like(k), table * 3
    elif kind == "flat":
        q, k, table = torch.zeros_like(q), torch.zeros_like(k), torch.full_like(table, 0.5)
    elif kind == "leak" and shift:
        corner = torch.roll(region_ids(H, shift) == 8, (shift, shift), (0, 1))   # rolled position -> the token's own position
        q[:, corner] = LEAK
        k[:, ~corner] = LEAK
    dt = DTYPE[prec]
    return dict(q=round_to(q, dt), k=round_to(k, dt), v=round_to(v, dt), table=table)


def pack_qkv(d, Cp, dtype, fill=float("nan")):
    """[B*H*H][3][Cp] in the operand type, pad columns of q, k and v filled with `fill`."""
    return torch.stack([pad_cols(d[n].reshape(-1, d[n].shape[-1]), Cp, fill) for n in "qkv"], 1).to(dtype).contiguous()


def _wa_parts(case, d, dtype, roll=-1, index="ref", table="ref", scale_pow=1, mask="ref", v_shift=0):
    B, H, shift, C, Cp = case
    heads = C // HD

    def part(t):
        t = t.to(dtype)
        if shift:
            t = torch.roll(t, (roll * shift, roll * shift), (1, 2))
        return windows(t, WS).view(-1, NW, heads, HD).transpose(1, 2)           # [B nW, heads, 49, 32]
    qq, kk, vv = part(d["q"]) * SCALE ** scale_pow, part(d["k"]), part(d["v"])
    if v_shift:
        vv = torch.roll(vv, v_shift, 1)
    idx = relative_index(WS)
    if index == "dydx_swapped":
        idx = (idx % 13) * 13 + idx // 13
    elif index == "sign_flipped":
        idx = idx.T
    tab = d["table"].to(dtype)
    if table == "heads_major":
        tab = tab.flatten().view(heads, -1).T
    bias = tab[idx.flatten()].view(NW, NW, heads).permute(2, 0, 1)
    m = None
    if shift and mask != "none":
        if mask in ("ref", "hard"):
            m = region_mask(H, H, WS, shift, dtype)
            if mask == "hard":
                m = torch.where(m != 0, torch.full_like(m, float("-inf")), m)
        else:
            m = _mask_of(region_ids(H, shift, cuts=(H - shift,) if mask == "hshift_only" else (H - WS,))).to(dtype)
        m = m[None, :, None].expand(B, -1, heads, -1, -1).reshape(-1, heads, NW, NW)
    return qq, kk, vv, bias, m


def _wa_tokens(case, o, roll=-1, unroll=True):
    """[B nW, heads, 49, 32] -> [B*H*H, C] at the tokens' own positions."""
    B, H, shift, C, Cp = case
    o = unwindows(o.transpose(1, 2).reshape(-1, NW, C), WS, B, H, H)
    if shift and unroll:
        o = torch.roll(o, (-roll * shift, -roll * shift), (1, 2))
    return o.reshape(-1, C)


def wa_eval(case, d, dtype=torch.float64, roll=-1, unroll=True, pad64=False, **kw):
    qq, kk, vv, bias, m = _wa_parts(case, d, dtype, roll=roll, **kw)
    s = qq @ kk.transpose(-2, -1) + bias
    if m is not None:
        s = s + m
    if pad64:
        p = torch.cat([s, torch.zeros_like(s[..., :15])], -1).softmax(-1)[..., :NW]
    else:
        p = s.softmax(-1)
    return _wa_tokens(case, p @ vv, roll, unroll)


def wa_ref(case, d):
    return wa_eval(case, d)


def wa_bound(case, d, prec):
    qq, kk, vv, bias, m = _wa_parts(case, d, torch.float64)
    dot = qq @ kk.transpose(-2, -1)
    s = dot + bias + (0 if m is None else m)
    es = (gamma(HD) + 2 * U) * (qq.abs() @ kk.abs().transpose(-2, -1)) + U * (dot + bias).abs() + U * s.abs()
    x = s - s.amax(-1, keepdim=True)
    ex = es + U * (x.abs() + es.amax(-1, keepdim=True))
    rho = torch.expm1(ex) + 2 * U * (x.abs() + ex + 1) + 2 * U
    w = s.softmax(-1)
    pi = rho + (rho * w).sum(-1, keepdim=True) + gamma(NW - 1) + 3 * U
    eo = ((pi + gamma(NW)) * w) @ vv.abs() + FLUSH * vv.abs().sum(-2, keepdim=True)
    return stored(_wa_tokens(case, eo), _wa_tokens(case, w @ vv), DTYPE[prec])


def wa_f32(case, d, prec):
    return to_out(wa_eval(case, d, torch.float32), DTYPE[prec])


def wa_mutants(case, d):
    shift = case[2]
    out = {"index_dydx_swapped": wa_eval(case, d, index="dydx_swapped"), "index_sign_flipped": wa_eval(case, d, index="sign_flipped"),
           "table_heads_major": wa_eval(case, d, table="heads_major"), "scale_twice": wa_eval(case, d, scale_pow=2),
           "scale_left_out": wa_eval(case, d, scale_pow=0), "v_of_next_head": wa_eval(case, d, v_shift=-1),
           "v_of_previous_head": wa_eval(case, d, v_shift=1), "softmax_over_64": wa_eval(case, d, pad64=True)}
    if shift:
        out.update({"roll_plus_shift": wa_eval(case, d, roll=1), "stored_unrolled": wa_eval(case, d, unroll=False),
                    "mask_none": wa_eval(case, d, mask="none"), "mask_split_at_H-7_only": wa_eval(case, d, mask="h7_only"),
                    "mask_hard": wa_eval(case, d, mask="hard")})
    return out


def wa_required(case, kind):
    """The mutants a (geometry, data kind) must reject.  Which kind sees what: zero q and k leave the scale without effect; a constant
    table the index; exp(-100) = 4e-44 is nothing next to weights of ordinary size, so only 'leak' tells -100 from a hard mask."""
    shift = case[2]
    geo = ["roll_plus_shift", "stored_unrolled", "mask_none", "mask_split_at_H-7_only"] if shift else []
    idx = ["index_dydx_swapped", "index_sign_flipped", "table_heads_major"]
    rest = ["v_of_next_head", "v_of_previous_head", "softmax_over_64"]
    if kind == "random":
        return geo + idx + rest + ["scale_twice", "scale_left_out"]
    if kind == "zeroqk":
        return geo + idx + rest
    if kind == "flat":
        return geo + rest
    return ["mask_hard", "mask_none"]


# ------------------------------------------------------------------------------------------------------------------------ head
# (B, HW, C, Cp, kind): one token; the forward's shape; pad channels; 256 threads; lnw = lnb = 0: every embedding is the zero vector
HEAD_CASES = [(3, 1, 768, 768, "real"), (3, 49, 768, 768, "real"), (2, 4, 128, 256, "real"), (1, 49, 1024, 1024, "real"),
              (2, 4, 128, 256, "zero")]


def head_data(B, HW, C, Cp, kind):
    g = _gen(5, B, HW, C, Cp)
    lnw, lnb = _affine(C, g)
    if kind == "zero":
        lnw, lnb = torch.zeros(C), torch.zeros(C)
    return dict(x=_tokens(B * HW, C, g).view(B, HW, C), lnw=lnw, lnb=lnb)


def _l2(m, norm=None, clamp=True):
    n = m.norm(dim=1, keepdim=True) if norm is None else norm
    return m / (n.clamp_min(1e-12) if clamp else n)


def head_ref(d, l2):
    m = ln64(d["x"], d["lnw"], d["lnb"]).mean(1)
    return _l2(m) if l2 else m


def head_bound(d, l2):
    HW = d["x"].shape[1]
    y, ey = ln_bound(d["x"], torch.zeros_like(d["x"], dtype=torch.float64), d["lnw"], d["lnb"])
    m = y.mean(1)
    e = (ey.sum(1) + gamma(HW) * y.abs().sum(1)) / HW + 2 * U * m.abs()         # HW adds in order, one division
    return l2_bound(m, e) if l2 else e + TINY32


def l2_bound(m, e):
    """Bound behind x / max(||x||, 1e-12) of the rows of m, known to within e (the sum of squares runs on the LayerNorm tree)."""
    ss = (m * m).sum(1, keepdim=True)
    ess = (2 * m.abs() * e + e * e).sum(1, keepdim=True) + gamma(LN_DEPTH + 2) * ss
    n = torch.sqrt(ss).clamp_min(1e-12)
    en = ess / (2 * n) + 2 * U * n
    out = m / n
    return e / n + m.abs() * en / (n * n) + 2 * U * out.abs() + TINY32


def head_f32(d, l2):
    C = d["x"].shape[-1]
    m = F.layer_norm(d["x"], (C,), d["lnw"], d["lnb"], EPS).mean(1)
    return F.normalize(m, dim=1) if l2 else m


def head_mutants(d, l2, Cp, kind="real"):
    x = d["x"].double()
    B, HW, C = x.shape
    y = ln64(x, d["lnw"], d["lnb"])
    fin = (lambda m: _l2(m)) if l2 else (lambda m: m)
    out = {"mean_over_HW_plus_1": fin(y.sum(1) / (HW + 1)),
           "unbiased_variance": fin(ln64(x, d["lnw"], d["lnb"], stats=(x.mean(-1, keepdim=True), x.var(-1, unbiased=True, keepdim=True))).mean(1))}
    if HW > 1:
        out["mean_before_norm"] = fin(ln64(x.mean(1), d["lnw"], d["lnb"]))
    if l2 and C < Cp:
        # the pad lanes' unmasked normalised values (0 - mean) rstd, averaged, taken into the norm
        pads = (-x.mean(-1) / torch.sqrt(x.var(-1, unbiased=False) + EPS)).mean(1, keepdim=True)
        m = y.mean(1)
        out["l2_norm_over_Cp"] = _l2(m, norm=torch.sqrt((m * m).sum(1, keepdim=True) + (Cp - C) * pads * pads))
    if l2 and kind == "zero":
        out["clamp_left_out"] = _l2(y.mean(1), clamp=False)
    return out


# ------------------------------------------------------------------------------------------------------------------------ linear
ROW_TILE = {"fp32": 128, "fp16": 256, "bf16": 256}             # gemm.hip (tile128.hpp BM); gemm2.hip G2M: the 16-bit modes' kernel at every pair
K_CHUNK = {"fp32": 32, "fp16": 64, "bf16": 64}                 # one K-stage: 128 bytes of every row
SWIN_STAGES = [(96, 128), (192, 256), (384, 384), (768, 768)]


def linear_roles():
    """(name, N, K, epilogue) of every linear of build_swin: 19 roles over 17 distinct (N, K)."""
    out = []
    for i, (C, Cp) in enumerate(SWIN_STAGES):
        if i:
            out.append((f"s{i}_reduction", Cp, 4 * SWIN_STAGES[i - 1][0], EPI_BIAS_F32))
        out += [(f"s{i}_qkv", 3 * Cp, Cp, EPI_BIAS), (f"s{i}_proj", Cp, Cp, EPI_BIAS_RESID), (f"s{i}_fc1", 4 * C, Cp, EPI_BIAS_GELU),
                (f"s{i}_fc2", Cp, 4 * C, EPI_BIAS_RESID)]
    return out


LINEAR_ROW_IDS = ["M1", "M49", "M130", "Mtile+1"]


def linear_rows(prec):
    return [1, 49, 130, ROW_TILE[prec] + 1]


def lin_data(N, K, M, epi, prec, kind="real", zero_bias=False):
    g = _gen(6, N, K, M, epi)
    dt = DTYPE[prec]
    if kind == "exact":
        x = torch.randint(-3, 4, (M, K), generator=g).float()
        w = torch.randint(-1, 2, (N, K), generator=g).float()
        bias = torch.randint(-4, 5, (N,), generator=g).float()
        resid = torch.randint(-8, 9, (M, N), generator=g).float()
    else:
        x = torch.randn(M, K, generator=g) + 0.3 * torch.linspace(-1, 1, M)[:, None]
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
        bias = torch.randn(N, generator=g) * 0.5
        resid = torch.randn(M, N, generator=g) + torch.linspace(-1, 1, N)
        if epi == EPI_BIAS_GELU:
            # Small activations under a bias spread over [-3.2, 1.5]: the pre-activations cover the left tail, where erf and tanh GELU
            # are 4.7e-4 apart (at -2.7) on values of size 0.01, and the accumulation term gamma_K sum |x||w| stays near 1e-4 at K = 768.
            x, bias = 0.15 * x, torch.linspace(-3.2, 1.5, N)[torch.randperm(N, generator=g)]
    if zero_bias:
        bias = torch.zeros(N)
    return dict(x=round_to(x, dt), w=round_to(w, dt), bias=bias, resid=resid if epi == EPI_BIAS_RESID else None)


def lin_out_dtype(epi, prec):
    return DTYPE[prec] if epi in (EPI_BIAS, EPI_BIAS_GELU) else torch.float32


def gelu64(y):
    return 0.5 * y * (1 + torch.erf(y / math.sqrt(2)))


def lin_finish(d, epi, acc, bias=None, resid_times=1, tanh=False):
    y = acc + (d["bias"].double() if bias is None else bias)
    if epi == EPI_BIAS_GELU:
        y = F.gelu(y, approximate="tanh") if tanh else gelu64(y)
    if epi == EPI_BIAS_RESID:
        y = y + resid_times * d["resid"].double()
    return y


def lin_ref(d, epi):
    return lin_finish(d, epi, d["x"].double() @ d["w"].double().T)


_FAST_C = [4.07419588e-08, -1.94481757e-06, 4.1060451e-05, -0.00051103633, 0.00423542528, -0.0251028568, 0.111079332, -0.375314877,
           1.12826843]                                          # common.hpp gelu_erf_fast: erf(z) ~ z P(z^2), z clamped to +-3


def erf_fast_abs_error():
    """max |z P(z^2) - erf(x / sqrt 2)| over x in [-6, 6], z = clamp(x / sqrt 2, +-3), in float64."""
    x = torch.linspace(-6, 6, 240001, dtype=torch.float64) / math.sqrt(2)
    z = x.clamp(-3, 3)
    t, p = z * z, torch.zeros_like(z)
    for c in _FAST_C:
        p = p * t + c
    return (z * p - torch.erf(x)).abs().max().item()


ERF_FAST_ABS = erf_fast_abs_error()


def lin_bound(d, epi, prec):
    x, w = d["x"].double(), d["w"].double()
    K = x.shape[1]
    acc = x @ w.T
    e = gamma(K) * (x.abs() @ w.abs().T)
    b = d["bias"].double()
    if epi == EPI_BIAS_RESID:                                   # acc + resid, then + bias
        t = acc + d["resid"].double()
        y = t + b
        e = e + U * t.abs() + U * y.abs()
    else:
        y = acc + b
        e = e + U * y.abs()
        if epi == EPI_BIAS_GELU:
            assert y.abs().max().item() + e.max().item() <= 6.0, "GELU case outside the range its erf constants hold for"
            erf_abs = 2 * ERF_F32_ABS if prec == "fp32" else ERF_FAST_ABS + 16 * U
            g = gelu64(y)
            y, e = g, GELU_LIP * e + 0.5 * y.abs() * erf_abs + 4 * U * g.abs()
    return stored(e, y, lin_out_dtype(epi, prec))


def lin_f32(d, epi, prec):
    y = d["x"] @ d["w"].T + d["bias"]
    if epi == EPI_BIAS_GELU:
        y = F.gelu(y)
    if epi == EPI_BIAS_RESID:
        y = y + d["resid"]
    return to_out(y, lin_out_dtype(epi, prec))


def lin_mutants(d, epi, prec):
    x, w = d["x"].double(), d["w"].double()
    M, K = x.shape
    N = w.shape[0]
    acc = x @ w.T
    out = {"bias_indexed_by_row": lin_finish(d, epi, acc, bias=d["bias"].double()[torch.arange(M) % N][:, None]),
           "last_k_chunk_dropped": lin_finish(d, epi, x[:, :K - K_CHUNK[prec]] @ w[:, :K - K_CHUNK[prec]].T)}
    if epi == EPI_BIAS_RESID:
        out["residual_added_twice"] = lin_finish(d, epi, acc, resid_times=2)
    if epi == EPI_BIAS_GELU:
        out["tanh_gelu"] = lin_finish(d, epi, acc, tanh=True)
    tile = ROW_TILE[prec]
    if M > tile:
        y = lin_finish(d, epi, acc).clone()
        t0 = (M - 1) // tile * tile
        y[t0:] = y[t0 - tile:M - tile]
        out["last_row_tile_duplicated"] = y
    return out
