"""-m "not gpu": the comparisons of tests/test_gpu_convnext_ops.py judged on the CPU.  For every case the GPU test runs and every
precision, a float32 torch evaluation of the operator lies inside the derived bound everywhere (computing the bound also runs
`ln_bound`'s conditioning assert on the case's data), and every mutant the case names (a float64 result corrupted the way the kernel
could be wrong, tests/convnext_ops_ref.py) lies outside it somewhere.  test_every_listed_mutant_is_rejected_somewhere holds the list of
mutants against what the cases named.

Which mutants a case names: every one that changes the reference for its geometry and data.  Not named are those that leave it
unchanged (a flipped or transposed kernel on a one-pixel map, which sees the centre tap only; isolated strips on a map of one strip;
a neighbouring crop's halo at B = 1; statistics over Cp when C = Cp; a scale indexed by row when the scale is constant; the clamp of
F.normalize on a non-zero embedding) and eps 1e-5 on a case without a row of small variance: at a variance near 1 it moves y by 4.5e-6
relative, inside the accumulation term of the bound.  The depthwise cases of two or more crops carry a crop scaled by 0.01, the
space-to-depth cases rows of standard deviation 0.01, the one-token and the 'cancel' head case an image of that scale.  The depthwise
operator's one-pass variance is named in fp32 and fp16 only: behind 50 roundings at |bias| = 100 std it moves y by some 1e-3 relative,
under bf16's half ulp (3.9e-3 |y|) wherever y does not happen to lie near 0.

The references are not merely self-consistent: chained together they are tests/convnext_ref.convnext_forward (test_chain_is_the_network),
which tests/test_convnext_host.py pins to transformers."""
import ctypes

import pytest
import torch

from effocr_amd import weights as W
from tests import convnext_ops_ref as R
from tests import convops_lib as CL
from tests import swin_ops_ref as S
from tests.convnext_ref import convnext_forward
from tests.convops_ref import Mismatch, check_bound
from tests.test_swin_ops_host import judge

DUMMY = ctypes.c_void_p(256)                                    # never dereferenced: every call below is refused before a launch


def _judge(op, ref, bound, f32, mutants, want, what):
    """test_swin_ops_host.judge, with the mutants rejected by name: the float32 evaluation inside, every mutant of `want` outside."""
    r = judge(ref, bound, f32, mutants, [], what)
    assert set(want) <= set(mutants), f"{what}: mutants {sorted(set(want) - set(mutants))} do not apply — change the case's data or shape"
    for name in want:
        outside = int(((mutants[name] - ref).abs() > bound).sum() + mutants[name].isnan().sum())
        assert outside, f"{what}: the bound admits the mutant {name}"
        with pytest.raises(Mismatch):
            check_bound(mutants[name], ref, bound, f"{what} {name}")
    print(f"{what}: float32 evaluation at {r:.2f} of the bound; rejected {', '.join(want)}")


def _cancel_ratio(rows):
    rows = rows.double()
    return (rows.mean(-1).abs() / rows.std(-1)).median().item()


def stem_required(C0):
    return ["ky_kx_swapped", "channel_major_taps", "bias_after_norm"] + (["norm_over_128"] if C0 < 128 else [])


@pytest.mark.parametrize("S_,B,C0,kind", R.STEM_CASES)
def test_stem(S_, B, C0, kind):
    d = R.stem_data(S_, B, C0, kind)
    _judge("stem", R.stem_ref(d), R.stem_bound(d), R.stem_f32(d), R.stem_mutants(d), stem_required(C0), f"stem S={S_} B={B} C0={C0} {kind}")
    if kind == "cancel":
        assert 50 < _cancel_ratio(S._stem_conv(d["x"], d["w"], d["b"])) < 200


def dw_required(case, kind, prec="fp32"):
    B, H, W, C, Cp = case
    want = ["pad_2_one_pixel_shift", "bias_after_norm"]
    if H * W > 1:
        want += ["ky_kx_swapped", "correlation_flipped", "replicate_border"]
    if H > R.DW_TH or W > R.DW_TW:
        want.append("strips_in_isolation")
    if B > 1:
        want.append("halo_rows_from_neighbouring_crop")
    if C < Cp:
        want.append("norm_over_Cp")
    if B > 1 and kind == "real":
        want.append("eps_1e-5")
    if kind == "cancel" and prec != "bf16":
        want.append("one_pass_variance_fp32")
    return want


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("case,kind", R.DW_RUNS, ids=lambda v: v if isinstance(v, str) else "B%d_%dx%d_C%d_Cp%d" % v)
def test_dwconv_ln(case, kind, prec):
    d = R.dw_data(case, kind)
    _judge("dwconv_ln", R.dw_ref(d), R.dw_bound(d, prec), R.dw_f32(d, prec), R.dw_mutants(d, case[4], kind), dw_required(case, kind, prec),
           f"dwconv_ln {case} {kind} {prec}")
    if kind == "cancel":
        assert 50 < _cancel_ratio(R._dw_conv(d["x"], d["w"], d["b"])) < 200
    wp, bp, _, _ = R.pack_dw(d, case[4])
    assert wp.shape == (49, case[4]) and wp[2 * 7 + 5, 3] == d["w"][3, 2, 5] and not wp[:, case[3]:].any() and not bp[case[3]:].any()


def test_dwconv_cases_reach_their_edges():
    segs = lambda Cp: 256 // (Cp // 4)                                          # convnext.hip: segs_for
    strips = lambda B, H, W: B * -(-H // R.DW_TH) * -(-W // R.DW_TW)
    assert strips(3, 7, 7) == 12 and segs(128) == 8 and 12 % 8                  # dead segments in the last block
    assert segs(768) == 1 and 768 // 4 // 32 == 6 and segs(384) == 2 and 2 * 96 == 192
    assert 11 % R.DW_TW == 3 and 9 % R.DW_TH and 16 % R.DW_TW == 0 and 2 == R.DW_TH
    src = open(CL.ROOT + "/effocr_amd/csrc/convnext.hip").read()
    assert f"constexpr int DW_TH = {R.DW_TH}, DW_TW = {R.DW_TW}" in src and "constexpr float CNX_EPS = 1e-6f" in src


def s2d_required(case, kind):
    return ["quadrants_x_major", "eps_1e-5"] + (["norm_over_Cp"] if case[3] < case[4] else []) + (["one_pass_variance_fp32"] if kind == "cancel" else [])


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("case,kind", R.S2D_RUNS, ids=lambda v: v if isinstance(v, str) else "B%d_%dx%d_C%d_Cp%d" % v)
def test_ln_s2d(case, kind, prec):
    d = R.s2d_data(case, kind)
    _judge("ln_s2d", R.s2d_ref(d), R.s2d_bound(d, prec), R.s2d_f32(d, prec), R.s2d_mutants(d, case[4], kind), s2d_required(case, kind),
           f"ln_s2d {case} {kind} {prec}")
    if kind == "cancel":
        assert 50 < _cancel_ratio(d["x"]) < 200


def test_s2d_rows_layout():
    B, H, W, C = 2, 4, 6, 3
    t = torch.arange(B * H * W * C, dtype=torch.float64).view(B, H, W, C)
    rows = R.s2d_rows(t)
    for b, y, x in [(0, 0, 0), (1, 3, 4), (0, 2, 5), (1, 1, 1)]:
        r = (b * (H // 2) + y // 2) * (W // 2) + x // 2
        q = (y & 1) * 2 + (x & 1)
        assert torch.equal(rows[r, q * C:(q + 1) * C], t[b, y, x])


def head_required(HW, C, Cp, kind, l2):
    if kind == "const":                                         # behind the clamp the bound is 1e-3 / 1e-12: only a NaN leaves it
        return ["clamp_left_out"] if l2 else ["norm_over_Cp"]
    return (["mean_after_norm"] if HW > 1 else []) + (["norm_over_Cp"] if C < Cp else []) + (["eps_1e-5"] if HW == 1 or kind == "cancel" else [])


@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("B,HW,C,Cp,kind", R.HEAD_CASES)
def test_head(B, HW, C, Cp, kind, l2):
    d = R.head_data(B, HW, C, Cp, kind)
    ref, muts = R.head_ref(d, l2), R.head_mutants(d, l2, Cp, kind)
    if kind == "const":
        assert not ref.any()
        assert not l2 or muts["clamp_left_out"].isnan().all()
    _judge("head", ref, R.head_bound(d, l2), R.head_f32(d, l2), muts, head_required(HW, C, Cp, kind, l2),
           f"head B={B} HW={HW} C={C} Cp={Cp} {kind} l2={l2}")
    if kind == "cancel":
        assert 50 < _cancel_ratio(d["x"].mean(1)) < 200


def lin4_required(kind):
    return ["scale_on_residual_too", "bias_outside_scale", "residual_added_twice"] + (["scale_indexed_by_row"] if kind != "tiny" else [])


LIN4_RUNS = ([(N, K, mi, "real") for N, K in R.FC2_SHAPES for mi in range(3)] + [(256, 768, 1, "tiny"), (128, 384, 1, "pad")])


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("N,K,mi,kind", LIN4_RUNS, ids=[f"N{n}_K{k}-{R.LIN4_ROW_IDS[m]}-{kd}" for n, k, m, kd in LIN4_RUNS])
def test_linear_scale_resid(N, K, mi, kind, prec):
    M = R.lin4_rows(prec)[mi]
    d = R.lin4_data(N, K, M, prec, kind)
    want = lin4_required(kind)
    ref, bound = R.lin4_ref(d), R.lin4_bound(d)
    _judge("linear4", ref, bound, R.lin4_f32(d), R.lin4_mutants(d, kind), want, f"linear scale+resid N={N} K={K} M={M} {kind} {prec}")
    if kind == "pad":
        assert not ref[:, 96:].any()
    if kind == "tiny":                                          # the result is the residual to within the bound
        assert bool(((ref - d["resid"].double()).abs() <= 1e-5).all()) and bound.max().item() < 1e-6


def test_linear_roles_of_epilogues_1_and_5_are_swins():
    roles = R.cnx_linear_roles()
    assert len(roles) == 7 and R.extra_linear_roles() == []
    have = {(n, k, e): name for name, n, k, e in S.linear_roles()}
    assert [have[r[1:]] for r in roles] == ["s0_fc1", "s1_reduction", "s1_fc1", "s2_reduction", "s2_fc1", "s3_reduction", "s3_fc1"]
    assert R.FC2_SHAPES == [(128, 384), (256, 768), (384, 1536), (768, 3072)]
    assert "gemm2_supported(prec, N, K) ? gemm2_nt(prec, epi, g, s) : gemm_nt(prec, epi, g, s)" in open(CL.ROOT + "/effocr_amd/csrc/api.hip").read()


LISTED = {"stem": {"ky_kx_swapped", "channel_major_taps", "bias_after_norm", "norm_over_128"},
          "dwconv_ln": {"ky_kx_swapped", "correlation_flipped", "pad_2_one_pixel_shift", "replicate_border", "strips_in_isolation",
                        "halo_rows_from_neighbouring_crop", "bias_after_norm", "norm_over_Cp", "one_pass_variance_fp32", "eps_1e-5"},
          "ln_s2d": {"quadrants_x_major", "norm_over_Cp", "eps_1e-5", "one_pass_variance_fp32"},
          "head": {"mean_after_norm", "norm_over_Cp", "clamp_left_out", "eps_1e-5"},
          "linear4": {"scale_on_residual_too", "bias_outside_scale", "scale_indexed_by_row", "residual_added_twice"}}


def test_every_listed_mutant_is_rejected_somewhere():
    """The union of what the cases above name (and reject) is the whole list, operator by operator."""
    named = {"stem": set().union(*(stem_required(c[2]) for c in R.STEM_CASES)),
             "dwconv_ln": set().union(*(dw_required(c, k) for c, k in R.DW_RUNS)),
             "ln_s2d": set().union(*(s2d_required(c, k) for c, k in R.S2D_RUNS)),
             "head": set().union(*(head_required(HW, C, Cp, k, l2) for _, HW, C, Cp, k in R.HEAD_CASES for l2 in (0, 1))),
             "linear4": set().union(*(lin4_required(k) for _, _, _, k in LIN4_RUNS))}
    assert named == LISTED


# ---------------------------------------------------------------------------------------------------- the references are the network
def test_chain_is_the_network():
    """stem -> [ln_s2d -> downsample] -> [dwconv_ln -> fc1 + GELU -> fc2 * gamma + residual] -> head in float64 is convnext_forward: the tap
    order, the quadrant order and the [C][kh][kw][C_prev] downsample permutation are the network's."""
    sd = W.init_state_dict("convnext_tiny", seed=3, img_size=32)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(5)).double()
    want = convnext_forward("convnext_tiny", sd, x)
    got = R.chain64(sd, x)
    assert got.dtype == torch.float64 and got.shape == want.shape == (2, 768)
    rel = ((got - want).abs().max() / want.abs().max()).item()
    print(f"chain of operator references vs convnext_forward, float64: {rel:.2e} relative")
    assert rel <= 1e-10
    n = torch.nn.functional.normalize(want, dim=1)
    assert ((R.chain64(sd, x, l2=1) - n).abs().max() / n.abs().max()).item() <= 1e-10


# ---------------------------------------------------------------------------------------------------- the entry points refuse before a launch
def test_refusals_before_any_launch():
    L = CL.lib()
    assert L.effocr_convops_abi_version() == CL.ABI_VERSION == 4
    stem = lambda S_, C0, x=DUMMY: L.effocr_convops_cnx_stem(x, 1, S_, DUMMY, DUMMY, DUMMY, DUMMY, C0, DUMMY, None)
    for S_, C0 in R.STEM_REFUSALS:
        assert stem(S_, C0) == CL.EUNSUPPORTED and "cnx_stem" in CL.last_error(), (S_, C0)
    assert stem(32, 96, None) == CL.EINVAL and stem(-32, 96) == CL.EINVAL and "cnx_stem" in CL.last_error()
    dw = lambda C, Cp, prec=CL.PREC_FP32, B=1, x=DUMMY: L.effocr_convops_cnx_dwconv_ln(prec, x, B, 4, 4, C, Cp, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, None)
    for C, Cp in R.DW_REFUSALS:
        assert dw(C, Cp) == CL.EUNSUPPORTED and "cnx_dwconv_ln" in CL.last_error(), (C, Cp)
    assert dw(96, 128, prec=7) == CL.EINVAL and dw(96, 128, B=-1) == CL.EINVAL and dw(96, 128, x=None) == CL.EINVAL
    s2d = lambda H, W_, x=DUMMY: L.effocr_convops_cnx_ln_s2d(CL.PREC_FP16, x, 1, H, W_, 96, 128, DUMMY, DUMMY, DUMMY, None)
    for H, W_ in R.S2D_REFUSALS:
        assert s2d(H, W_) == CL.EUNSUPPORTED and "cnx_ln_s2d" in CL.last_error(), (H, W_)
    assert s2d(2, 2, None) == CL.EINVAL and s2d(-2, 2) == CL.EINVAL
    head = lambda C, Cp, HW=4, x=DUMMY: L.effocr_convops_cnx_head(x, 1, HW, C, Cp, DUMMY, DUMMY, 0, DUMMY, None, None)
    assert head(96, 192) == CL.EUNSUPPORTED and "cnx_head" in CL.last_error() and head(96, 128, HW=0) == CL.EUNSUPPORTED
    assert head(96, 128, x=None) == CL.EINVAL and head(96, 128, HW=-1) == CL.EINVAL
    lin = lambda epi, resid=DUMMY, scale=DUMMY, prec=CL.PREC_FP16, n=128, k=384, m=4, x=DUMMY: L.effocr_convops_linear(
        prec, epi, x, DUMMY, DUMMY, resid, scale, DUMMY, m, n, k, None)
    for epi in (0, 2, 3, 6, -1):
        assert lin(epi) == CL.EINVAL and "epilogue" in CL.last_error(), epi
    assert lin(4, resid=None) == CL.EINVAL and lin(4, scale=None) == CL.EINVAL and "convops_linear" in CL.last_error()
    assert lin(1, x=None) == CL.EINVAL and lin(5, m=-1) == CL.EINVAL and lin(4, prec=3) == CL.EINVAL
    assert lin(4, n=96) == CL.EUNSUPPORTED and lin(4, prec=CL.PREC_FP32, n=96) == CL.EUNSUPPORTED      # the launchers' own refusals
    assert lin(4, k=100) == CL.EUNSUPPORTED
