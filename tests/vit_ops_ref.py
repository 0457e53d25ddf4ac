"""Float64 restatements, test data, derived error bounds and mutants of the non-GEMM operators of the main ViT path, in the kernels' own
layouts: the fused patch embedding (csrc/patch.hip), the unfused pair im2col16 + EPI_PATCH (csrc/vit_ops.hip; csrc/gemm.hip, csrc/gemm2.hip),
set_cls / gather_cls, the final class-token norm (csrc/vit_ops.hip) and the class-token form of the fused qkv + attention kernel
(csrc/qkvattn.hip).  tests/test_gpu_vit_ops.py runs the kernels against them through the effocr_convops_vit_* entry points of the test-only
library; tests/test_vit_ops_host.py proves on the CPU that every bound admits a float32 evaluation and rejects the mutants.  Comparison
functions and rounding constants are tests/convops_ref.py's, the error model and `lin_bound` / `ln_bound` / `l2_bound` tests/swin_ops_ref.py's.

Fragment-blocked layout (common.hpp blk_off): [rows / 32][cols / ch][32 rows][ch], ch = the elements of 16 bytes (`to_blocked`).

Patch embedding and EPI_PATCH, K = 768 = (c, py, px), tokens [B, 1 + P, D] with the class token at 0:
  * integer data (pixels -3..3, weights -1/0/1, bias and pos_embed integers in -8..8): every partial sum is an integer of at most
    768 * 3 + 16 < 2^24, so fp32 arithmetic in any order is exact and the kernel equals the float64 result cast to fp32 bit for bit.
  * real data, operands rounded to the mode's type (fp32 mode: as they are): `lin_bound`'s accumulation term gamma_768 sum |x||w|, then the
    two fp32 adds in the source's order — patch.hip (acc + bias) + pos, the GEMMs (acc + pos) + bias: u |first sum| + u |out|.
  * the class-token rows are a copy: bound 0.
im2col, set_cls, gather_cls: pure movement, bit equality.

Final norm (cls_norm_kernel<G, V>, ln.hpp ln_apply / group_sum): the mean's tree is ((v0 + v1) + (v2 + v3)) per float4, V <= 3 of them added in
order, then log2 G <= 6 xor-shuffle levels: depth <= 2 + 3 + 6 = 11.  The variance's and the L2 norm's are 4 V <= 12 squares added in order in
the thread, then the 6 shuffle levels: depth 18.  Both sit within swin_ops_ref's LN_DEPTH = 20, so `ln_bound` (eps 1e-6) and `l2_bound`
hold as they are.

Class-token attention: the restatement of tests/test_gpu_kernels.py::test_qkv_attn_fused_blocked (q, k, v rounded to the operand type, float64
softmax) on row img * T of every image, and that test's own tolerance, 1.5e-2 (bf16) / 2e-3 (fp16) of the largest reference element of
those rows."""
import math

import torch
import torch.nn.functional as F

from tests import swin_ops_ref as S
from tests.convops_ref import TINY, U, round_to
from tests.swin_ops_ref import DTYPE, gamma, l2_bound, ln64, ln_bound

EPS = 1e-6
PATCH_K = 768
TINY32 = TINY[torch.float32]
NAN = float("nan")
ATTN_TOL = {"bf16": 1.5e-2, "fp16": 2e-3}


# ------------------------------------------------------------------------------------------------------------------------ layouts
def to_blocked(t, rows_alloc):
    """[rows, cols] tensor -> flat buffer in the cell layout [rows_alloc/32][cols/ch][32][ch] (ch = 16 bytes)."""
    rows, cols = t.shape
    ch = 16 // t.element_size()
    buf = torch.zeros((rows_alloc, cols), dtype=t.dtype)
    buf[:rows] = t
    return buf.view(rows_alloc // 32, 32, cols // ch, ch).permute(0, 2, 1, 3).contiguous().view(-1)


def from_blocked(flat, rows, cols, rows_alloc):
    ch = 16 // flat.element_size()
    return flat.view(rows_alloc // 32, cols // ch, 32, ch).permute(0, 2, 1, 3).contiguous().view(rows_alloc, cols)[:rows]


def up32(n):
    return (n + 31) // 32 * 32


def perm32_rows(t):
    """P32 of include/effocr_hip.h along dim 0 (the v rows of the fused qkv weight and bias)."""
    p = torch.arange(32)
    hh, r = (p >> 2) & 1, (p & 3) + 4 * (p >> 3)
    src = 8 * (2 * (r >> 3) + hh) + (r & 7)
    idx = (torch.arange(t.shape[0] // 32)[:, None] * 32 + src[None, :]).reshape(-1)
    return t[idx].contiguous()


# ------------------------------------------------------------------------------------------------------------------------ patch embedding
def patch_slice_width(D, B, P, cus):
    """launch_patch (patch.hip): the output width of one workgroup."""
    panels = (B * P + 127) // 128
    if D == 384 and panels * 3 <= cus:
        return 128
    return 384 if D == 768 else D


def whole_panel_batch(cus):
    """Smallest batch of 32x32 crops (P = 4) whose panels no longer fit three slices each into one round of CUs: one crop past the last
    batch of whole panels that does, so the last panel is partial (256 CUs: 2721 crops, 86 panels)."""
    B = 1
    while ((B * 4 + 127) // 128) * 3 <= cus:
        B += 1
    return B


def patch_cases(cus):
    """(name, D, H, W, B, why)."""
    return [("three_slice_4_patches", 384, 32, 32, 1, "124 clamped lanes"),
            ("three_slice_wave_straddle", 384, 32, 48, 5, "images straddle a wave, non-square, PW = 3"),
            ("three_slice_partial_panel", 384, 224, 224, 1, "196 patches: the second panel is partial"),
            ("three_slice_image_boundary", 384, 224, 224, 3, "image boundary at patch 196 = 6 * 32 + 4 inside a wave"),
            ("d128", 128, 64, 64, 2, ""), ("d256", 256, 64, 64, 2, ""),
            ("d768_two_slices_small", 768, 32, 32, 1, ""), ("d768_two_slices", 768, 224, 224, 1, ""),
            ("whole_panels", 384, 32, 32, whole_panel_batch(cus), "panels * 3 > CUs: 384-wide panels, the last one partial")]


def patch_data(D, H, W, B, kind):
    g = S._gen(11, D, H, W, B, kind == "exact")
    P = (H // 16) * (W // 16)
    if kind == "exact":
        x = torch.randint(-3, 4, (B, 3, H, W), generator=g).float()
        w = torch.randint(-1, 2, (D, PATCH_K), generator=g).float()
        bias = torch.randint(-8, 9, (D,), generator=g).float()
        pos = torch.randint(-8, 9, (1 + P, D), generator=g).float()
        cls = torch.randint(-8, 9, (D,), generator=g).float()
    else:
        x = torch.randn(B, 3, H, W, generator=g) + 0.5 * torch.randn(B, 3, 1, 1, generator=g)
        w = torch.randn(D, PATCH_K, generator=g) / math.sqrt(PATCH_K)
        bias = torch.randn(D, generator=g) * 0.5
        pos = torch.randn(1 + P, D, generator=g)
        cls = torch.randn(D, generator=g)
    return dict(x=x, w=w, bias=bias, pos=pos, cls=cls, P=P, kind=kind)


def im2col(x, swap=False):
    """[B, 3, H, W] -> [B, P, 768], p = ty * PW + tx, k = (c, py, px); swap: k = (c, px, py)."""
    B = x.shape[0]
    u = x.unfold(2, 16, 16).unfold(3, 16, 16)                   # [B, 3, PH, PW, py, px]
    if swap:
        u = u.transpose(-1, -2)
    return u.permute(0, 2, 3, 1, 4, 5).reshape(B, u.shape[2] * u.shape[3], PATCH_K)


def _finish(acc, bias, pos, order):
    """The two adds in the source's order; returns (first sum, out)."""
    first = acc + (bias if order == "bias_pos" else pos)
    return first, first + (pos if order == "bias_pos" else bias)


def _tokens(d, patches, cls=None):
    """[B, 1 + P, D] float64: the class token in front of every image's patches."""
    B, P, D = patches.shape
    c = (d["cls"] if cls is None else cls).double()
    return torch.cat([c.view(1, 1, D).expand(B, 1, D), patches], 1)


def patch_ref(d, prec, order="bias_pos"):
    """float64 tokens [B, 1 + P, D] on operands rounded to prec's type."""
    dt = DTYPE[prec]
    acc = im2col(round_to(d["x"], dt)).double() @ round_to(d["w"], dt).double().T
    return _tokens(d, _finish(acc, d["bias"].double(), d["pos"][1:].double(), order)[1])


def patch_bound(d, prec, order="bias_pos"):
    dt = DTYPE[prec]
    rows, w = im2col(round_to(d["x"], dt)).double(), round_to(d["w"], dt).double()
    first, out = _finish(rows @ w.T, d["bias"].double(), d["pos"][1:].double(), order)
    e = gamma(PATCH_K) * (rows.abs() @ w.abs().T) + U * first.abs() + U * out.abs() + TINY32
    return torch.cat([torch.zeros_like(e[:, :1]), e], 1)         # the class-token row is a copy


def patch_exact_premise(d):
    top = (im2col(d["x"]).abs().double() @ d["w"].abs().double().T).max().item() + d["bias"].abs().max().item() + d["pos"].abs().max().item()
    assert top <= PATCH_K * 3 + 16 < 2 ** 24, top


def patch_f32(d, prec, order="bias_pos"):
    dt = DTYPE[prec]
    acc = im2col(round_to(d["x"], dt)) @ round_to(d["w"], dt).T
    return _tokens(d, _finish(acc, d["bias"], d["pos"][1:], order)[1].double()).float()


def patch_mutants(d, prec, dw, order="bias_pos"):
    """{name: float64 tokens of a wrong kernel}; dw: the output width of one workgroup (slices 1.. exist when dw < D)."""
    dt = DTYPE[prec]
    x, w = round_to(d["x"], dt), round_to(d["w"], dt).double()
    bias, pos, cls = d["bias"].double(), d["pos"].double(), d["cls"].double()
    B, _, H, W = x.shape
    PH, PW, P, D = H // 16, W // 16, d["P"], w.shape[0]
    acc = im2col(x).double() @ w.T
    fin = lambda a, b=bias, ps=pos[1:]: _finish(a, b, ps, order)[1]
    ref = fin(acc)
    out = {"pos_embed_row_p": _tokens(d, fin(acc, ps=pos[:P])),
           "py_px_swapped": _tokens(d, fin(im2col(x, swap=True).double() @ w.T)),
           "channels_bgr": _tokens(d, fin(im2col(x.flip(1)).double() @ w.T))}
    ps = pos[1:].clone()
    ps[0] = pos[0]
    out["class_pos_embed_on_patch_0"] = _tokens(d, fin(acc, ps=ps))
    if dw < D:
        f0 = torch.arange(D) % dw
        out["bias_of_slice_0"] = _tokens(d, fin(acc, b=bias[f0]))
        out["pos_embed_of_slice_0"] = _tokens(d, fin(acc, ps=pos[1:][:, f0]))
        out["class_row_from_slice_0"] = _tokens(d, ref, cls=cls[f0])
    if PH != PW:
        p = torch.arange(P)
        out["ty_tx_transposed"] = _tokens(d, fin(acc[:, (p % PH) * PW + p // PH]))
    if B * P >= 2:
        t = ref.reshape(B * P, D).clone()
        t[-1] = t[-2]
        out["last_patch_copied"] = _tokens(d, t.view(B, P, D))
    if B >= 2:
        a = acc.clone()
        a[1:, 0] = acc[:-1, 0]
        out["first_patch_from_previous_image"] = _tokens(d, fin(a))
    if dt != torch.float32:
        out["operand_rounding_left_out"] = _tokens(d, fin(im2col(d["x"]).double() @ d["w"].double().T))
    full = _tokens(d, ref)
    shifted = torch.full_like(full, NAN)                          # row img * T + p: the class row overwritten, the last row never written
    shifted[:, :P] = ref
    out["output_row_without_plus_1"] = shifted
    return out


# ------------------------------------------------------------------------------------------------------------------------ final norm
NORM_WG_IMAGES = {128: 8, 384: 8, 768: 4}                       # final_cls_norm: images per workgroup


def norm_data(D, T, B, kind="real"):
    """x [B * T, D] fp32 tokens; the class rows take the scales 0.01, 3, 0.3, 1 in turn (eps matters in the first).  'cancel': |mean| = 100
    std in the class rows; 'zero': image 0's class row is all zero and beta is zero, so its embedding is the zero vector."""
    g = S._gen(12, D, T, B, {"real": 0, "cancel": 1, "zero": 2}[kind])
    x = S._tokens(B * T, D, g)
    scale = torch.tensor([0.01, 3.0, 0.3, 1.0])[torch.arange(B) % 4][:, None]
    c = torch.randn(B, D, generator=g)
    x[::T] = scale * ((100.0 + c) if kind == "cancel" else (c + 0.4 + torch.linspace(-0.5, 0.5, D)))
    lnw, lnb = S._affine(D, g)
    if kind == "zero":
        x[0] = 0.0
        lnb = torch.zeros(D)
    return dict(x=x, lnw=lnw, lnb=lnb, T=T, B=B, kind=kind)


def _cls_rows(d):
    return d["x"][::d["T"]]


def _l2(m, clamp=True):
    n = m.norm(dim=1, keepdim=True)
    return m / (n.clamp_min(1e-12) if clamp else n)


def norm_ref(d, l2):
    y = ln64(_cls_rows(d), d["lnw"], d["lnb"], EPS)
    return _l2(y) if l2 else y


def norm_bound(d, l2):
    x = _cls_rows(d)
    y, ey = ln_bound(x, torch.zeros_like(x, dtype=torch.float64), d["lnw"], d["lnb"], EPS)
    return l2_bound(y, ey) if l2 else ey + TINY32


def norm_f32(d, l2):
    y = F.layer_norm(_cls_rows(d), d["x"].shape[-1:], d["lnw"], d["lnb"], EPS)
    return F.normalize(y, dim=1) if l2 else y


def norm_mutants(d, l2):
    x, T, B = _cls_rows(d).double(), d["T"], d["B"]
    D = x.shape[1]
    fin = (lambda y: _l2(y)) if l2 else (lambda y: y)
    out = {"eps_1e-5": fin(ln64(x, d["lnw"], d["lnb"], 1e-5))}
    ra = up32(B * T)
    out["row_major_offsets_on_a_blocked_buffer"] = fin(ln64(to_blocked(d["x"], ra).view(ra, D)[::T][:B], d["lnw"], d["lnb"], EPS))
    if T > 1:
        out["norm_of_token_1"] = fin(ln64(d["x"][1::T], d["lnw"], d["lnb"], EPS))
    if l2:
        out["l2_before_the_affine"] = _l2(ln64(x, torch.ones(D), torch.zeros(D), EPS)) * d["lnw"].double() + d["lnb"].double()
    if d["kind"] == "cancel":
        x32 = _cls_rows(d)
        m32 = x32.mean(-1, keepdim=True)
        v32 = (x32 * x32).mean(-1, keepdim=True) - m32 * m32      # E[x^2] - mean^2 in fp32
        out["one_pass_variance_fp32"] = fin(ln64(x, d["lnw"], d["lnb"], EPS, stats=(m32.double(), v32.double().clamp_min(0))))
    if l2 and d["kind"] == "zero":
        out["clamp_left_out"] = _l2(ln64(x, d["lnw"], d["lnb"], EPS), clamp=False)
    return out


# ------------------------------------------------------------------------------------------------------------------------ gather_cls
def gather_ref(x, att, T):
    return x[::T].clone(), att[::T].clone()


def gather_mutants(x, att, T):
    """{name: (xc, ac)}: row img * T + 1; the 16-bit half taken from image img - 1."""
    xc, ac = gather_ref(x, att, T)
    return {"row_img_T_plus_1": (x[1::T].clone(), att[1::T].clone()), "att_row_of_previous_image": (xc, torch.roll(ac, 1, 0))}


# ------------------------------------------------------------------------------------------------------------------------ class-token attention
def attn_data(B, T, D, prec):
    g = torch.Generator().manual_seed(B * 1000 + T + D)
    dt = DTYPE[prec]
    xn = torch.randn(B * T, D, generator=g).to(dt)
    w = (torch.randn(3 * D, D, generator=g) / math.sqrt(D)).to(dt)
    bias = 0.5 * torch.randn(3 * D, generator=g)
    return dict(xn=xn, w=w, bias=bias)


def cls_attn_ref(d, B, T, D, prec):
    """Row img * T of softmax(q k^T / 8) v, [B, D] float64: q, k, v rounded to the operand type, float64 softmax."""
    heads = D // 64
    qkv = (d["xn"].double() @ d["w"].double().T + d["bias"].double()).to(DTYPE[prec]).double()
    q, k, v = qkv.reshape(B, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
    att = ((q[:, :, :1] * 0.125) @ k.transpose(-2, -1)).softmax(-1)
    return (att @ v)[:, :, 0].reshape(B, D)
