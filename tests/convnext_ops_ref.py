"""Float64 restatements, test data, derived error bounds and mutants of the ConvNeXt operators: the four kernels of csrc/convnext.hip
(stem, depthwise 7x7 + LayerNorm, LayerNorm + space-to-depth, head) and the linears of convnext_forward (csrc/api.hip: `lin`), above all
the layer-scale epilogue EPI_BIAS_SCALE_RESID of gemm.hip / gemm2.hip, on caller-made tensors in the kernels' own layouts:

  stem weight [48 taps (c, ky, kx)][128]; depthwise weight [49 taps ky * 7 + kx][Cp]; activations [tokens][Cp]; space-to-depth rows
  [B H/2 W/2][4 C], quadrant (y & 1) * 2 + (x & 1), no pad columns.

tests/test_gpu_convnext_ops.py runs the kernels against them through libeffocr_convops.so (effocr_convops_cnx_*, effocr_convops_linear);
tests/test_convnext_ops_host.py proves on the CPU that every bound admits a float32 evaluation and rejects the mutants, and that the
references chained together are tests/convnext_ref.convnext_forward.  The LayerNorm, rounding, stem, head and linear machinery is
tests/swin_ops_ref.py's (its eps arguments carry ConvNeXt's 1e-6), the comparison functions tests/convops_ref.py's.

Every reference works on the REAL channels only; the GPU test fills the pad channels of its inputs with NaN and asserts the pad channels
of the outputs to be exactly 0 on its own.

Error model: the one at the head of swin_ops_ref.py.  What this file adds to it:
  * stem: the bias and 48 FMAs in a fixed order: gamma_49 (|x| * |w| + |b|), then `ln_bound`.
  * depthwise: the bias and 49 FMAs in (ky, kx) order: gamma_50 (conv(|x|, |w|) + |b|), then `ln_bound`, then the store.
  * seg_layernorm's summation tree is 2 levels in the thread, 5 in the 32-lane half and at most 6 halves in order (Cp = 768): 13 deep,
    inside swin_ops_ref.LN_DEPTH = 20.
  * head: HW adds in token order (gamma_HW sum |x|) and a division (2 u) in front of `ln_bound`; F.normalize as swin_ops_ref.l2_bound.
  * layer-scale epilogue: acc within gamma_K sum |x||w| (`lin_bound`'s accumulation term); t = acc + bias adds u |t|; out = fma(scale, t,
    resid) carries |scale| times that and one rounding u |out|.  The output is fp32 in every precision.
  * no measured constant but swin_ops_ref.ERF_F32_ABS (fp32 GELU, re-measured by tests/test_gpu_swin_ops.py).

Linears with epilogues 1 (bias + GELU) and 5 (bias, fp32 out): ConvNeXt's roles are fc1 (4C, Cp) and the downsample (Cp_next, 4C).  Both
libraries dispatch on (precision, N, K) alone (gemm2_supported ? gemm2_nt : gemm_nt), and swin_ops_ref.linear_roles() already holds every
one of them with the same epilogue — fc1 (384, 128), (768, 256), (1536, 384), (3072, 768) as s0..s3_fc1, the downsamples (256, 384),
(384, 768), (768, 1536) as s1..s3_reduction — so `extra_linear_roles()` is empty (asserted by the host test) and tests/test_gpu_swin_ops.py
is their operator test; the GPU test here runs one of each through effocr_convops_linear to cover the entry point itself."""
import torch
import torch.nn.functional as F

from tests import swin_ops_ref as S
from tests.convops_ref import U
from tests.swin_ops_ref import (DTYPE, EPI_BIAS_F32, EPI_BIAS_GELU, PRECS, ROW_TILE, TINY32, _affine, _gen, _tokens, gamma, ln64, ln_bound,
                                pad_cols, stored, to_out)

EPS = 1e-6
EPI_BIAS_SCALE_RESID = 4
STAGES = [(96, 128), (192, 256), (384, 384), (768, 768)]       # (C, Cp) of convnext_tiny
CROP_SCALE = [1.0, 0.01, 3.0]


def _stats_over(p):
    return p.mean(-1, keepdim=True), p.var(-1, unbiased=False, keepdim=True)


def _one_pass_fp32(x64):
    """(mean, E[x^2] - mean^2), both evaluated in fp32 on the fp32 rounding of x64."""
    x = x64.float()
    m = x.mean(-1, keepdim=True)
    return m.double(), ((x * x).mean(-1, keepdim=True) - m * m).double().clamp_min(0)


def _zeros(t):
    return torch.zeros_like(t, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------------------------------ stem
# (S, B, C0, kind): 64 tokens = whole blocks; crop borders inside the token stream; 256 tokens; no pad channels (the launcher accepts it);
# cancel: a bias near 100 standard deviations of the convolution
STEM_CASES = [(32, 1, 96, "real"), (32, 3, 96, "real"), (64, 1, 96, "real"), (32, 2, 128, "real"), (32, 3, 96, "cancel")]
STEM_REFUSALS = [(48, 96), (32, 132), (32, 98)]                 # (S, C0)


def stem_data(S_, B, C0, kind="real"):
    d = S.stem_data(S_, B, C0)
    if kind == "cancel":
        d["b"] = (100.0 * S._stem_conv(d["x"], d["w"], None).std().item() + d["b"]).float()
    return d


def stem_ref(d):
    return S.stem_ref(d, EPS)


def stem_bound(d):
    return S.stem_bound(d, EPS)


def stem_f32(d):
    return S.stem_f32(d, EPS)


def stem_mutants(d):
    return S.stem_mutants(d, EPS)


# ------------------------------------------------------------------------------------------------------------------------ depthwise + LayerNorm
# (B, H, W, C, Cp): one pixel (48 of 49 taps outside; one segment per block, 6 halves); odd H, W < 8, 12 strips on 8 segments (dead
# segments in the barriers); a strip seam at x = 8 with a 3-wide tail, odd H, H != W; Cq = 96 (3 halves, 192-thread blocks); 768 channels
# on a 4 x 4 map; one strip row with the seam at a strip boundary and both halos live
DW_CASES = [(2, 1, 1, 768, 768), (3, 7, 7, 96, 128), (2, 9, 11, 192, 256), (1, 14, 14, 384, 384), (2, 4, 4, 768, 768), (1, 2, 16, 96, 128)]
DW_RUNS = [(c, "real") for c in DW_CASES] + [((3, 7, 7, 96, 128), "cancel"), ((2, 9, 11, 192, 256), "cancel")]
DW_REFUSALS = [(96, 192), (1152, 1152), (98, 128), (256, 128)]  # (C, Cp)
DW_TH, DW_TW = 2, 8


def dw_data(case, kind="real"):
    """x [B, H, W, C], w [C, 7, 7], b, lnw, lnb [C].  A 7 x 7 window mixes its rows, so only a crop-wide scale reaches the LayerNorm: crop
    b is scaled by CROP_SCALE[b] (the second crop's rows have a variance where eps matters; the bias is small enough to leave it so).
    The last row of crop b is bright and the first row of crop b + 1 dark.  cancel: the bias is 100 standard deviations of the
    convolution's output (crop scales left out: one bias cannot be 100 deviations of all of them)."""
    B, H, W, C, Cp = case
    g = _gen(11, B, H, W, C, kind == "cancel")
    x = torch.randn(B, H, W, C, generator=g) + torch.linspace(-0.5, 0.5, C) + 0.3 * torch.linspace(-1, 1, W)[None, None, :, None]
    x[:, -1] += 1.5
    x[1:, 0] -= 1.5
    w = torch.randn(C, 7, 7, generator=g) / 7 + 0.05 * torch.linspace(-1, 1, 49).view(7, 7)
    b = torch.randn(C, generator=g) * 0.02
    lnw, lnb = _affine(C, g)
    if kind == "cancel":
        b = (100.0 * _dw_conv(x, w, None).std(-1).mean().item() + 25 * b).float()
    else:
        x = x * torch.tensor(CROP_SCALE)[torch.arange(B) % 3][:, None, None, None]
    return dict(x=x, w=w, b=b, lnw=lnw, lnb=lnb)


def pack_dw(d, Cp):
    """(w [49 taps ky * 7 + kx][Cp], b, lnw, lnb [Cp]) as pack_convnext lays them out: zeros beyond C."""
    C = d["w"].shape[0]
    return (pad_cols(d["w"].reshape(C, 49).T.contiguous(), Cp), pad_cols(d["b"], Cp), pad_cols(d["lnw"], Cp), pad_cols(d["lnb"], Cp))


def _dw_conv(x, w, b, pad="zeros"):
    """float64 depthwise 7x7 of x [B, H, W, C] -> [B*H*W, C]; pad: zeros (3 each side), replicate, or 'shift' (2 before, 4 after)."""
    C = x.shape[-1]
    t = x.double().permute(0, 3, 1, 2)
    if pad == "replicate":
        t = F.pad(t, (3, 3, 3, 3), mode="replicate")
    else:
        t = F.pad(t, (2, 4, 2, 4) if pad == "shift" else (3, 3, 3, 3))
    y = F.conv2d(t, w.double().view(C, 1, 7, 7), None if b is None else b.double(), groups=C)
    return y.permute(0, 2, 3, 1).reshape(-1, C)


def dw_ref(d):
    return ln64(_dw_conv(d["x"], d["w"], d["b"]), d["lnw"], d["lnb"], EPS)


def dw_bound(d, prec):
    ec = gamma(50) * _dw_conv(d["x"].abs(), d["w"].abs(), d["b"].abs())         # 49 FMAs on top of the bias
    y, ey = ln_bound(_dw_conv(d["x"], d["w"], d["b"]), ec, d["lnw"], d["lnb"], EPS)
    return stored(ey, y, DTYPE[prec])


def dw_f32(d, prec):
    C = d["w"].shape[0]
    y = F.conv2d(d["x"].permute(0, 3, 1, 2), d["w"].view(C, 1, 7, 7), d["b"], padding=3, groups=C).permute(0, 2, 3, 1).reshape(-1, C)
    return to_out(F.layer_norm(y, (C,), d["lnw"], d["lnb"], EPS), DTYPE[prec])


def dw_mutants(d, Cp, kind="real"):
    x, w, b, g, be = d["x"], d["w"], d["b"], d["lnw"], d["lnb"]
    B, H, W, C = x.shape
    conv = _dw_conv(x, w, b)
    ln = lambda c, **kw: ln64(c, g, be, kw.pop("eps", EPS), **kw)
    out = {"pad_2_one_pixel_shift": ln(_dw_conv(x, w, b, pad="shift")), "bias_after_norm": ln(_dw_conv(x, w, None)) + b.double(),
           "eps_1e-5": ln(conv, eps=1e-5)}
    if H * W > 1:                                               # (one pixel sees the centre tap only)
        out["correlation_flipped"] = ln(_dw_conv(x, w.flip(1, 2), b))
        out["ky_kx_swapped"] = ln(_dw_conv(x, w.transpose(1, 2), b))
        out["replicate_border"] = ln(_dw_conv(x, w, b, pad="replicate"))
    if H > DW_TH or W > DW_TW:
        iso = torch.empty(B, H, W, C, dtype=torch.float64)
        for y0 in range(0, H, DW_TH):
            for x0 in range(0, W, DW_TW):
                xs = torch.zeros_like(x)
                xs[:, y0:y0 + DW_TH, x0:x0 + DW_TW] = x[:, y0:y0 + DW_TH, x0:x0 + DW_TW]
                iso[:, y0:y0 + DW_TH, x0:x0 + DW_TW] = _dw_conv(xs, w, b).view(B, H, W, C)[:, y0:y0 + DW_TH, x0:x0 + DW_TW]
        out["strips_in_isolation"] = ln(iso.view(-1, C))
    if B > 1:
        out["halo_rows_from_neighbouring_crop"] = ln(_dw_conv(x.reshape(1, B * H, W, C), w, b))
    if C < Cp:
        out["norm_over_Cp"] = ln(conv, stats=_stats_over(pad_cols(conv, Cp)))
    if kind == "cancel":
        out["one_pass_variance_fp32"] = ln(conv, stats=_one_pass_fp32(conv))
    return out


# ------------------------------------------------------------------------------------------------------------------------ LayerNorm + space-to-depth
# (B, H, W, C, Cp): 12 tokens on 8 segments; 196 tokens; H != W; one 96-thread segment pair; one token per block
S2D_CASES = [(3, 2, 2, 96, 128), (1, 14, 14, 96, 128), (2, 4, 2, 192, 256), (1, 2, 2, 384, 384), (2, 2, 2, 768, 768)]
S2D_RUNS = [(c, "real") for c in S2D_CASES] + [((3, 2, 2, 96, 128), "cancel"), ((2, 2, 2, 768, 768), "cancel")]
S2D_REFUSALS = [(3, 2), (2, 3)]                                 # (H, W)


def s2d_data(case, kind="real"):
    B, H, W, C, Cp = case
    g = _gen(12, B, H, W, C, kind == "cancel")
    lnw, lnb = _affine(C, g)
    return dict(x=_tokens(B * H * W, C, g, kind).view(B, H, W, C), lnw=lnw, lnb=lnb)


def s2d_rows(t, x_major=False):
    """[B, H, W, C] -> [B H/2 W/2][4 C], quadrant (y & 1) * 2 + (x & 1) (x_major: (x & 1) * 2 + (y & 1))."""
    B, H, W, C = t.shape
    t = t.view(B, H // 2, 2, W // 2, 2, C)
    t = t.permute(0, 1, 3, 4, 2, 5) if x_major else t.permute(0, 1, 3, 2, 4, 5)
    return t.reshape(B * (H // 2) * (W // 2), 4 * C)


def s2d_ref(d):
    return s2d_rows(ln64(d["x"], d["lnw"], d["lnb"], EPS))


def s2d_bound(d, prec):
    y, ey = ln_bound(d["x"], _zeros(d["x"]), d["lnw"], d["lnb"], EPS)
    return s2d_rows(stored(ey, y, DTYPE[prec]))


def s2d_f32(d, prec):
    return s2d_rows(to_out(F.layer_norm(d["x"], d["x"].shape[-1:], d["lnw"], d["lnb"], EPS), DTYPE[prec]))


def s2d_mutants(d, Cp, kind="real"):
    x, g, b = d["x"].double(), d["lnw"], d["lnb"]
    C = x.shape[-1]
    out = {"quadrants_x_major": s2d_rows(ln64(x, g, b, EPS), x_major=True), "eps_1e-5": s2d_rows(ln64(x, g, b, 1e-5))}
    if C < Cp:
        out["norm_over_Cp"] = s2d_rows(ln64(x, g, b, EPS, stats=_stats_over(pad_cols(x, Cp))))
    if kind == "cancel":
        out["one_pass_variance_fp32"] = s2d_rows(ln64(x, g, b, EPS, stats=_one_pass_fp32(x)))
    return out


# ------------------------------------------------------------------------------------------------------------------------ head
# (B, HW, C, Cp, kind): one token; the 224^2 forward's shape; pad channels; cancel; const: every token of image b is the constant K_b in
# every channel and lnb = 0, so the pooled row is constant and its LayerNorm 0.  Image 0 (K = 0) is 0 in fp32 too, bit for bit, and
# F.normalize's clamp must make 0 / max(0, 1e-12) = 0 of it, not NaN.  Image 1 (K = -2): fl(1 / C) is inexact for C = 96, so the
# deviation v - s fl(1 / C) is a rounding residue near K 2^-25, which rstd = 1e3 (the variance is 0) carries to 1e-4 — inside `ln_bound`,
# whose rstd term is as large; behind F.normalize any finite vector is inside the bound there (the norm's own bound exceeds the norm).
HEAD_CASES = [(3, 1, 768, 768, "real"), (3, 49, 768, 768, "real"), (2, 4, 96, 128, "real"), (2, 4, 96, 128, "cancel"), (2, 4, 96, 128, "const")]
HEAD_CONST = [0.0, -2.0]


def head_data(B, HW, C, Cp, kind):
    g = _gen(13, B, HW, C, Cp, kind == "cancel")
    lnw, lnb = _affine(C, g)
    if kind == "const":
        x = torch.tensor(HEAD_CONST)[torch.arange(B) % 2][:, None, None].expand(B, HW, C).contiguous()
        return dict(x=x, lnw=lnw, lnb=torch.zeros(C))
    if kind == "cancel":                                        # the POOLED row has |mean| = 100 std: a per-image row, repeated with noise
        row = _tokens(B, C, g, "cancel")[:, None, :]
        return dict(x=row + 0.3 * row.std(-1, keepdim=True) * torch.randn(B, HW, C, generator=g), lnw=lnw, lnb=lnb)
    return dict(x=_tokens(B * HW, C, g).view(B, HW, C), lnw=lnw, lnb=lnb)


def head_ref(d, l2):
    m = ln64(d["x"].double().mean(1), d["lnw"], d["lnb"], EPS)
    return S._l2(m) if l2 else m


def head_bound(d, l2):
    x = d["x"].double()
    HW = x.shape[1]
    m = x.mean(1)
    em = gamma(HW) * x.abs().sum(1) / HW + 2 * U * m.abs()     # HW adds in token order, one division
    y, ey = ln_bound(m, em, d["lnw"], d["lnb"], EPS)
    return S.l2_bound(y, ey) if l2 else ey + TINY32


def head_f32(d, l2):
    C = d["x"].shape[-1]
    m = F.layer_norm(d["x"].mean(1), (C,), d["lnw"], d["lnb"], EPS)
    return F.normalize(m, dim=1) if l2 else m


def head_mutants(d, l2, Cp, kind="real"):
    x, g, b = d["x"].double(), d["lnw"], d["lnb"]
    B, HW, C = x.shape
    m = x.mean(1)
    fin = S._l2 if l2 else (lambda t: t)
    out = {"eps_1e-5": fin(ln64(m, g, b, 1e-5))}
    if HW > 1:
        out["mean_after_norm"] = fin(ln64(x, g, b, EPS).mean(1))
    if C < Cp:
        out["norm_over_Cp"] = fin(ln64(m, g, b, EPS, stats=_stats_over(pad_cols(m, Cp))))
    if l2 and kind == "const":
        out["clamp_left_out"] = S._l2(ln64(m, g, b, EPS), clamp=False)
    return out


# ------------------------------------------------------------------------------------------------------------------------ linear, layer scale
FC2_SHAPES = [(Cp, 4 * C) for C, Cp in STAGES]                  # (N, K): (128, 384), (256, 768), (384, 1536), (768, 3072)
LIN4_ROW_IDS = ["M1", "M49", "Mtile+1"]
LIN4_KINDS = ["real", "tiny", "pad"]                            # scale U(0.2, 1); scale 1e-6 (timm's init); Cp = 128, C = 96 with a zero pad


def lin4_rows(prec):
    return [1, 49, ROW_TILE[prec] + 1]


def lin4_data(N, K, M, prec, kind="real"):
    """x, w in the operand type's values, bias, resid [M, N], scale [N].  pad: rows 96 .. 127 of w, of bias and of scale and the residual's
    pad columns are zero, as pack_convnext and the kernels in front of fc2 leave them."""
    d = S.lin_data(N, K, M, S.EPI_BIAS_RESID, prec)
    g = _gen(14, N, K, M, LIN4_KINDS.index(kind))
    d["scale"] = torch.full((N,), 1e-6) if kind == "tiny" else torch.rand(N, generator=g) * 0.8 + 0.2
    if kind == "pad":
        assert (N, K) == (128, 384)
        for k in ("w", "bias", "scale"):
            d[k][96:] = 0
        d["resid"][:, 96:] = 0
    return d


def lin4_eval(d, scale_resid=False, bias_outside=False, scale_by_row=False, resid_times=1):
    acc = d["x"].double() @ d["w"].double().T
    M, N = acc.shape
    s, b, r = d["scale"].double(), d["bias"].double(), d["resid"].double()
    if scale_by_row:
        s = s[torch.arange(M) % N][:, None]
    if scale_resid:
        return s * (acc + b + r)
    if bias_outside:
        return r + s * acc + b
    return resid_times * r + s * (acc + b)


def lin4_ref(d):
    return lin4_eval(d)


def lin4_bound(d):
    x, w = d["x"].double(), d["w"].double()
    e = gamma(x.shape[1]) * (x.abs() @ w.abs().T)
    t = x @ w.T + d["bias"].double()
    e = e + U * t.abs()                                         # the bias add
    out = d["resid"].double() + d["scale"].double() * t
    return stored(d["scale"].double().abs() * e + U * out.abs(), out, torch.float32)   # one FMA


def lin4_f32(d):
    return d["resid"] + d["scale"] * (d["x"] @ d["w"].T + d["bias"])


def lin4_mutants(d, kind="real"):
    out = {"scale_on_residual_too": lin4_eval(d, scale_resid=True), "bias_outside_scale": lin4_eval(d, bias_outside=True),
           "residual_added_twice": lin4_eval(d, resid_times=2)}
    if kind != "tiny":                                          # (a constant scale has no index)
        out["scale_indexed_by_row"] = lin4_eval(d, scale_by_row=True)
    return out


def cnx_linear_roles():
    """(name, N, K, epilogue) of every linear of convnext_forward with epilogue 1 or 5."""
    out = []
    for i, (C, Cp) in enumerate(STAGES):
        if i:
            out.append((f"s{i}_downsample", Cp, 4 * STAGES[i - 1][0], EPI_BIAS_F32))
        out.append((f"s{i}_fc1", 4 * C, Cp, EPI_BIAS_GELU))
    return out


def extra_linear_roles():
    """The roles of cnx_linear_roles() whose (N, K, epilogue) tests/test_gpu_swin_ops.py::test_linear does not already run."""
    have = {(n, k, e) for _, n, k, e in S.linear_roles()}
    return [r for r in cnx_linear_roles() if r[1:] not in have]


# ------------------------------------------------------------------------------------------------------------------------ the network, op by op
def chain_parts(sd, arch="convnext_tiny"):
    """The state dict (timm key names) as the operators' data dictionaries: (stem, stages, head); a stage is (downsample or None, blocks),
    the downsample's weight [C][kh][kw][C_prev] flattened to [C, 4 C_prev] (the space-to-depth order), a block (dw, fc1, fc2)."""
    from effocr_amd.weights import CONVNEXT_CFG, strip_prefix
    depths, widths = CONVNEXT_CFG[arch]
    P = strip_prefix(sd)
    stem = dict(w=P["stem.0.weight"], b=P["stem.0.bias"], lnw=P["stem.1.weight"], lnb=P["stem.1.bias"])
    stages = []
    for i, (nb, C) in enumerate(zip(depths, widths)):
        p = f"stages.{i}."
        ds = None
        if i:
            ds = dict(lnw=P[p + "downsample.0.weight"], lnb=P[p + "downsample.0.bias"], bias=P[p + "downsample.1.bias"],
                      w=P[p + "downsample.1.weight"].permute(0, 2, 3, 1).reshape(C, 4 * widths[i - 1]).contiguous())
        blocks = []
        for j in range(nb):
            q = p + f"blocks.{j}."
            blocks.append((dict(w=P[q + "conv_dw.weight"].view(C, 7, 7), b=P[q + "conv_dw.bias"], lnw=P[q + "norm.weight"], lnb=P[q + "norm.bias"]),
                           dict(w=P[q + "mlp.fc1.weight"], bias=P[q + "mlp.fc1.bias"]),
                           dict(w=P[q + "mlp.fc2.weight"], bias=P[q + "mlp.fc2.bias"], scale=P[q + "gamma"])))
        stages.append((ds, blocks))
    return stem, stages, dict(lnw=P["head.norm.weight"], lnb=P["head.norm.bias"])


def chain64(sd, x, l2=0):
    """convnext_forward as a chain of this file's float64 operator references."""
    stem, stages, head = chain_parts(sd)
    B, H = x.shape[0], x.shape[-1] // 4
    t = stem_ref(dict(stem, x=x))                               # [B H H, C]
    for ds, blocks in stages:
        C = t.shape[-1]
        if ds is not None:
            rows = s2d_ref(dict(x=t.view(B, H, H, C), lnw=ds["lnw"], lnb=ds["lnb"]))
            H //= 2
            t = S.lin_ref(dict(x=rows, w=ds["w"], bias=ds["bias"]), EPI_BIAS_F32)
            C = t.shape[-1]
        for dw, fc1, fc2 in blocks:
            a = dw_ref(dict(dw, x=t.view(B, H, H, C)))
            h = S.lin_ref(dict(fc1, x=a), EPI_BIAS_GELU)
            t = lin4_ref(dict(fc2, x=h, resid=t))
    return head_ref(dict(head, x=t.view(B, H * H, t.shape[-1])), l2)
