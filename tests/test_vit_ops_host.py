"""-m "not gpu": the comparisons of tests/test_gpu_vit_ops.py judged on the CPU.  For every case the GPU test runs, a float32 torch evaluation
of the operator lies inside the derived bound everywhere, and every mutant the case names (the float64 restatement corrupted the way the kernel
could be wrong, tests/vit_ops_ref.py) lies outside it somewhere; for the integer data the float32 evaluation is bit-equal and `check_exact`
rejects the mutants.  The moved rows of gather_cls are judged by bit equality.  test_every_listed_mutant_is_rejected_somewhere holds the
list of mutants against what the cases named.

Which mutants a case names: every one that changes the reference for its geometry — slices 1.. exist only where a workgroup is narrower than
the embedding (three 128-wide slices at D = 384 on a small call, two 384-wide at D = 768), (ty, tx) can be transposed only on a non-square
image, a neighbouring image needs B >= 2, token 1 needs T >= 2, the clamp of F.normalize needs the all-zero row, the one-pass variance the
'cancel' rows (|mean| = 100 std)."""
import ctypes

import pytest
import torch

from tests import convops_lib as CL
from tests import vit_ops_ref as R
from tests.convops_ref import Mismatch, check_bound, check_exact
from tests.test_swin_ops_host import judge

CUS = 256                                                       # the MI355X's CU count, for the whole-panel case
DUMMY = ctypes.c_void_p(256)                                    # never dereferenced: every call below is refused before a launch
PATCH_CASES = R.patch_cases(CUS)

PATCH_LISTED = ["pos_embed_row_p", "class_pos_embed_on_patch_0", "bias_of_slice_0", "pos_embed_of_slice_0", "class_row_from_slice_0",
                "ty_tx_transposed", "py_px_swapped", "channels_bgr", "last_patch_copied", "first_patch_from_previous_image",
                "operand_rounding_left_out", "output_row_without_plus_1"]
GATHER_LISTED = ["row_img_T_plus_1", "att_row_of_previous_image"]
NORM_LISTED = ["eps_1e-5", "one_pass_variance_fp32", "norm_of_token_1", "l2_before_the_affine", "clamp_left_out",
               "row_major_offsets_on_a_blocked_buffer"]


def patch_required(D, H, W, B, prec, dw, kind):
    want = ["pos_embed_row_p", "class_pos_embed_on_patch_0", "py_px_swapped", "channels_bgr", "output_row_without_plus_1"]
    if dw < D:
        want += ["bias_of_slice_0", "pos_embed_of_slice_0", "class_row_from_slice_0"]
    if H != W:
        want.append("ty_tx_transposed")
    if B * (H // 16) * (W // 16) >= 2:
        want.append("last_patch_copied")
    if B >= 2:
        want.append("first_patch_from_previous_image")
    if prec != "fp32" and kind == "real":                       # (the integer data is representable in every operand type)
        want.append("operand_rounding_left_out")
    return want


def _judge_exact(ref, f32, mutants, want, what):
    assert set(want) <= set(mutants), f"{what}: mutants {sorted(set(want) - set(mutants))} do not apply"
    check_exact(f32, ref, what + " float32 evaluation")
    for name in want:
        with pytest.raises(Mismatch):
            check_exact(mutants[name].float(), ref, f"{what} {name}")


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("case", PATCH_CASES, ids=[c[0] for c in PATCH_CASES])
def test_patch_embed(case, prec, kind):
    name, D, H, W, B, _ = case
    d = R.patch_data(D, H, W, B, kind)
    dw = R.patch_slice_width(D, B, d["P"], CUS)
    want = patch_required(D, H, W, B, prec, dw, kind)
    ref, f32, mut = R.patch_ref(d, prec), R.patch_f32(d, prec), R.patch_mutants(d, prec, dw)
    what = f"patch_embed {name} {prec} {kind}"
    if kind == "exact":
        R.patch_exact_premise(d)
        _judge_exact(ref, f32, mut, want, what)
    else:
        r = judge(ref, R.patch_bound(d, prec), f32, mut, want, what)
        print(f"{what}: float32 evaluation at {r:.2f} of the bound; rejected {', '.join(want)}")


def test_patch_cases_reach_their_edges():
    by = {c[0]: c for c in PATCH_CASES}
    P = lambda c: (c[2] // 16) * (c[3] // 16)
    width = lambda c: R.patch_slice_width(c[1], c[4], P(c), CUS)
    assert P(by["three_slice_4_patches"]) == 4 and 128 - 4 == 124 and width(by["three_slice_4_patches"]) == 128
    c = by["three_slice_wave_straddle"]
    assert P(c) == 6 and c[3] // 16 == 3 and 32 % 6 and c[4] * 6 < 32 and width(c) == 128
    assert P(by["three_slice_partial_panel"]) == 196 and 196 % 128 and width(by["three_slice_partial_panel"]) == 128
    assert 196 == 6 * 32 + 4 and width(by["three_slice_image_boundary"]) == 128
    assert width(by["d128"]) == 128 and width(by["d256"]) == 256 and width(by["d768_two_slices"]) == 384 == width(by["d768_two_slices_small"])
    c = by["whole_panels"]
    panels = (c[4] * 4 + 127) // 128
    assert c[4] == 2721 and panels == 86 and panels * 3 > CUS >= (panels - 1) * 3 and (c[4] * 4) % 128 == 4 and width(c) == 384
    src = open(CL.ROOT + "/effocr_amd/csrc/patch.hip").read()
    assert "if (a.D == 384 && panels * 3 <= device_cus())" in src and "acc[t][4 * q] + bv[0] + pv[0]" in src      # dispatch and add order restated above
    for f in ("gemm.hip", "gemm2.hip"):                         # (acc + pos) + bias: the order patch_bound(..., "pos_bias") charges
        g = open(CL.ROOT + "/effocr_amd/csrc/" + f).read()
        assert g.index("acc[i][j][4 * q + e] += rv[i][j][q][e]") < g.index("float v0 = acc[i][j][4 * q + 0] + bv[i][q][0];")


EPI_CASES = [(4, 1), (196, 3)]                                  # (P, B): the smallest; M = 588 past both row tiles (128 fp32, 256 16-bit)


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("P,B", EPI_CASES)
def test_epi_patch(P, B, prec, kind):
    H, W = (32, 32) if P == 4 else (224, 224)
    d = R.patch_data(384, H, W, B, kind)
    want = [m for m in patch_required(384, H, W, B, prec, 384, kind) if m not in ("py_px_swapped", "channels_bgr")]   # (the rows are an input here)
    ref, f32, mut = R.patch_ref(d, prec, "pos_bias"), R.patch_f32(d, prec, "pos_bias"), R.patch_mutants(d, prec, 384, "pos_bias")
    what = f"EPI_PATCH P={P} B={B} {prec} {kind}"
    if kind == "exact":
        _judge_exact(ref, f32, mut, want, what)
    else:
        r = judge(ref, R.patch_bound(d, prec, "pos_bias"), f32, mut, want, what)
        print(f"{what}: float32 evaluation at {r:.2f} of the bound; rejected {', '.join(want)}")
    assert B * P == 4 or (B * P > 2 * 256 and 196 % 128 and 196 % 256)


def test_gather_cls_mutants():
    g = torch.Generator().manual_seed(5)
    x, att = torch.randn(3 * 5, 128, generator=g), torch.randint(-32768, 32767, (3 * 5, 128), generator=g, dtype=torch.int16)
    xc, ac = R.gather_ref(x, att, 5)
    mut = R.gather_mutants(x, att, 5)
    assert sorted(mut) == sorted(GATHER_LISTED)
    for name, (mx, ma) in mut.items():
        assert not (torch.equal(mx, xc) and torch.equal(ma, ac)), name
    b = R.to_blocked(x, 32)
    assert torch.equal(R.from_blocked(b, 15, 128, 32), x) and b[4 * 32 * 1 + 2 * 4 + 1] == x[2, 5]     # cell (chunk 1, row 2), element 1


NORM_HOST = ([(D, T, B, "real") for D in (128, 384, 768) for T in (1, 5, 197) for B in (1, R.NORM_WG_IMAGES[D] + 1)]
             + [(128, 5, 9, "cancel"), (384, 5, 9, "cancel"), (768, 5, 5, "cancel"), (128, 5, 9, "zero"), (384, 197, 9, "zero"), (768, 5, 5, "zero")])


def norm_required(T, l2, kind):
    want = ["row_major_offsets_on_a_blocked_buffer"] + (["norm_of_token_1"] if T > 1 else []) + (["l2_before_the_affine"] if l2 else [])
    if not (kind == "zero" and l2):                             # (beta = 0: rstd is a common factor of the row, which F.normalize removes)
        want.append("eps_1e-5")
    if kind == "cancel":
        want.append("one_pass_variance_fp32")
    if kind == "zero" and l2:
        want.append("clamp_left_out")
    return want


@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("D,T,B,kind", NORM_HOST)
def test_final_norm(D, T, B, kind, l2):
    d = R.norm_data(D, T, B, kind)
    want = norm_required(T, l2, kind)
    if kind == "cancel":
        rows = R._cls_rows(d).double()
        assert 50 < (rows.mean(-1).abs() / rows.std(-1)).median().item() < 200
    ref = R.norm_ref(d, l2)
    if kind == "zero" and l2:
        assert bool((ref[0] == 0).all())
    r = judge(ref, R.norm_bound(d, l2), R.norm_f32(d, l2), R.norm_mutants(d, l2), want, f"final_norm D={D} T={T} B={B} {kind} l2={l2}")
    print(f"final_norm D={D} T={T} B={B} {kind} l2={l2}: float32 evaluation at {r:.2f} of the bound; rejected {', '.join(want)}")


def test_norm_tree_depth_within_ln_depth():
    """ln.hpp as the module docstring of vit_ops_ref reads it: per float4 two levels, V float4 and 4 V squares added in order, log2 G shuffles."""
    src = open(CL.ROOT + "/effocr_amd/csrc/ln.hpp").read()
    assert "s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);" in src and "for (int o = G / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);" in src
    ops = open(CL.ROOT + "/effocr_amd/csrc/vit_ops.hip").read()
    for G, V in ((32, 3), (64, 3), (32, 1)):
        assert f"cls_norm_kernel<{G}, {V}>" in ops
        assert 2 + V + G.bit_length() - 1 <= 4 * V + G.bit_length() - 1 <= 18 <= R.S.LN_DEPTH


def test_class_attention_reference_is_the_all_token_one():
    """cls_attn_ref is row img * T of the restatement tests/test_gpu_kernels.py compares the all-token kernel with."""
    B, T, D = 2, 17, 128
    d = R.attn_data(B, T, D, "fp16")
    qkv = (d["xn"].double() @ d["w"].double().T + d["bias"].double()).to(torch.float16)
    q, k, v = qkv.double().reshape(B, T, 3, D // 64, 64).permute(2, 0, 3, 1, 4)
    full = (((q * 0.125) @ k.transpose(-2, -1)).softmax(-1) @ v).transpose(1, 2).reshape(B * T, D)
    assert torch.equal(R.cls_attn_ref(d, B, T, D, "fp16"), full[::T])
    w = torch.arange(64.)[:, None].expand(64, 8)
    assert R.perm32_rows(w)[:8, 0].tolist() == [0, 1, 2, 3, 8, 9, 10, 11]


def test_every_listed_mutant_is_rejected_somewhere():
    """The union of what the cases above name (and reject) is the whole list, operator by operator."""
    patch = set()
    for _, D, H, W, B, _ in PATCH_CASES:
        dw = R.patch_slice_width(D, B, (H // 16) * (W // 16), CUS)
        patch |= {m for prec in ("bf16", "fp16") for kind in ("exact", "real") for m in patch_required(D, H, W, B, prec, dw, kind)}
    assert patch == set(PATCH_LISTED)
    assert {m for _, T, _, kind in NORM_HOST for l2 in (0, 1) for m in norm_required(T, l2, kind)} == set(NORM_LISTED)
    assert set(R.gather_mutants(torch.zeros(4, 8), torch.zeros(4, 8, dtype=torch.int16), 2)) == set(GATHER_LISTED)


# ---------------------------------------------------------------------------------------------------- the entry points refuse before a launch
def test_refusals_before_any_launch():
    L = CL.lib()
    assert L.effocr_convops_abi_version() == CL.ABI_VERSION == 4
    pe = lambda prec=0, x=DUMMY, H=32, W=32, D=384, P=4, B=1: L.effocr_convops_vit_patch_embed(prec, x, 0, B, H, W, DUMMY, DUMMY, DUMMY, None, DUMMY, D, P, None)
    assert pe(x=None) == CL.EINVAL and pe(B=-1) == CL.EINVAL and "vit_patch_embed" in CL.last_error()
    assert pe(prec=2) == CL.EUNSUPPORTED and pe(D=512) == CL.EUNSUPPORTED and pe(H=40) == CL.EINVAL and pe(P=5) == CL.EINVAL
    assert pe(B=0) == CL.OK and CL.patch_last_dispatch() == (0, 0)
    im = lambda prec=0, x16=0, H=32, x=DUMMY: L.effocr_convops_vit_im2col16(prec, x, x16, 1, H, 32, DUMMY, None)
    assert im(x=None) == CL.EINVAL and im(H=40) == CL.EINVAL and im(prec=2, x16=1) == CL.EUNSUPPORTED and im(prec=5) == CL.EINVAL
    pg = lambda prec=0, D=384, blk=0, col=DUMMY, B=1: L.effocr_convops_vit_patch_gemm(prec, col, DUMMY, DUMMY, DUMMY, DUMMY, B, 4, D, blk, None)
    assert pg(col=None) == CL.EINVAL and pg(prec=3) == CL.EINVAL and pg(D=100) == CL.EUNSUPPORTED and pg(prec=2, blk=1) == CL.EUNSUPPORTED
    assert "fragment-blocked" in CL.last_error() and pg(B=0) == CL.OK
    assert L.effocr_convops_vit_set_cls(None, DUMMY, 1, 5, 128, 0, None, None) == CL.EINVAL
    assert L.effocr_convops_vit_set_cls(DUMMY, DUMMY, 1, 5, 130, 1, None, None) == CL.EINVAL
    assert L.effocr_convops_vit_gather_cls(DUMMY, None, 1, 5, 128, DUMMY, DUMMY, None) == CL.EINVAL
    assert L.effocr_convops_vit_gather_cls(DUMMY, DUMMY, 1, 5, 132, DUMMY, DUMMY, None) == CL.EINVAL
    qa = lambda prec=0, T=197, D=384, ra=224, xn=DUMMY, hs=0: L.effocr_convops_vit_qkv_attn(prec, xn, DUMMY, DUMMY, DUMMY, 1, T, D, ra, 1, hs, None)
    assert qa(xn=None) == CL.EINVAL and qa(hs=-1) == CL.EINVAL and qa(prec=2) == CL.EUNSUPPORTED and qa(T=100) == CL.EUNSUPPORTED
    assert qa(D=256) == CL.EUNSUPPORTED and qa(ra=192) == CL.EINVAL and qa(ra=200) == CL.EINVAL and CL.qkv_attn_last_dispatch() == []
    fn = lambda D=384, x=DUMMY, B=1: L.effocr_convops_vit_final_norm(x, B, 5, D, DUMMY, DUMMY, 1e-6, 1, 1, DUMMY, None, None)
    assert fn(x=None) == CL.EINVAL and fn(D=256) == CL.EUNSUPPORTED and "final norm" in CL.last_error() and fn(B=0) == CL.OK


def test_product_libraries_do_not_export_the_vit_operators():
    import os
    for so in sorted(f for f in os.listdir(os.path.join(CL.ROOT, "effocr_amd")) if f.endswith(".so") and f != "libeffocr_convops.so"):
        with open(os.path.join(CL.ROOT, "effocr_amd", so), "rb") as f:
            assert b"effocr_convops" not in f.read(), so
