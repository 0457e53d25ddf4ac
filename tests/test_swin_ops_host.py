"""-m "not gpu": the comparisons of tests/test_gpu_swin_ops.py judged on the CPU.  For every case the GPU test runs and every precision,
a float32 torch evaluation of the operator lies inside the derived bound everywhere, and every mutant the case names (a float64 result
corrupted the way the kernel could be wrong, tests/swin_ops_ref.py) lies outside it somewhere.

Which mutants a case names: every one that changes the reference for its geometry.  Not named are those that leave it unchanged
(statistics over Cp when C = Cp, a roll or a mask when shift = 0, a neighbouring token when M = 1, the mean before the norm at HW = 1,
a mean over HW + 1 in front of F.normalize, which removes the common factor), and eps 1e-6 in the 16-bit modes on a case without a row
of small variance: there it moves y by 4.5e-6 relative, a hundredth of an f16 half ulp.  Every LayerNorm case of more than one row
carries rows of standard deviation 0.01, where eps 1e-6 moves y by 4 % and is named in every precision.

One mutant of the issue's list cannot be rejected by any data: a mask whose regions are split at H - shift only.  H - 7 is a window
border, no window holds positions from both sides of it, so inside every window that mask equals the reference's
(test_mask_split_at_h_minus_shift_only_is_the_same_mask)."""
import os
import re

import pytest
import torch

from tests import swin_ops_ref as R
from tests.convops_ref import Mismatch, assert_exact_premise, check_bound, check_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def judge(ref, bound, f32, mutants, expected, what):
    """The named mutants outside, the float32 evaluation inside.  `expected`: the mutant names the case must have and reject."""
    assert set(expected) <= set(mutants), f"{what}: mutants {sorted(set(expected) - set(mutants))} do not apply — change the case's data or shape"
    assert torch.isfinite(ref).all() and torch.isfinite(bound).all() and (bound >= 0).all()
    ratio = check_bound(f32.double(), ref, bound, what + " float32 evaluation")
    for name in expected:
        with pytest.raises(Mismatch):
            check_bound(mutants[name], ref, bound, f"{what} {name}")
    return ratio


@pytest.mark.parametrize("S,B,C0", R.STEM_CASES)
def test_stem(S, B, C0):
    d = R.stem_data(S, B, C0)
    want = ["ky_kx_swapped", "channel_major_taps", "bias_after_norm"] + (["norm_over_128"] if C0 < 128 else [])
    r = judge(R.stem_ref(d), R.stem_bound(d), R.stem_f32(d), R.stem_mutants(d), want, f"stem {S} {B} {C0}")
    print(f"stem S={S} B={B} C0={C0}: float32 evaluation at {r:.2f} of the bound")
    wt, b, lnw, lnb = R.pack_stem(d)
    assert wt.shape == (48, 128) and not wt[:, C0:].any() and not b[C0:].any()
    assert wt[1 * 16 + 2 * 4 + 3, 5] == d["w"][5, 1, 2, 3]                     # tap (c, ky, kx) major


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("C,Cp,M,kind", R.LN_CASES)
def test_layernorm(C, Cp, M, kind, prec):
    d = R.ln_data(C, Cp, M, kind)
    want = (["unbiased_variance"] + (["statistics_over_Cp"] if C < Cp else []) + (["neighbouring_token_statistics"] if M > 1 else [])
            + (["eps_1e-6"] if prec == "fp32" or (M > 1 and kind == "real") else [])
            + (["one_pass_variance_fp32"] if kind == "cancel" else []))
    r = judge(R.ln_ref(d), R.ln_op_bound(d, prec), R.ln_f32(d, prec), R.ln_mutants(d, Cp, kind), want, f"layernorm {C} {Cp} {M} {kind} {prec}")
    print(f"layernorm C={C} Cp={Cp} M={M} {kind} {prec}: float32 evaluation at {r:.2f} of the bound")
    if kind == "cancel":
        x = d["x"].double()
        assert torch.allclose(x.mean(-1).abs() / x.std(-1), torch.full((M,), 100.0, dtype=torch.float64), rtol=0.3)


def test_layernorm_cases_reach_their_edges():
    for C, Cp in R.LN_GEOM:
        segs = 1 if Cp >= 1024 else 256 // (Cp // 4)                              # swin_layernorm
        assert segs == R.LN_SEGS[Cp]
        assert (C, Cp, 1, "real") in R.LN_CASES and (C, Cp, 2 * segs + 1, "real") in R.LN_CASES
    assert 37 % 8 and 17 % 8


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("B,H,C,Cp", R.MERGE_CASES)
def test_merge(B, H, C, Cp, prec):
    d = R.merge_data(B, H, C, Cp)
    want = ["quadrants_row_major", "norm_per_quadrant", "last_row_from_next_crop", "unbiased_variance"] + (["row_stride_C_for_Cp"] if C < Cp else [])
    r = judge(R.merge_ref(d), R.merge_bound(d, prec), R.merge_f32(d, prec), R.merge_mutants(d, Cp), want, f"merge {B} {H} {C} {Cp} {prec}")
    print(f"merge B={B} H={H} C={C} Cp={Cp} {prec}: float32 evaluation at {r:.2f} of the bound")


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("case,kind", R.WA_RUNS, ids=lambda v: v if isinstance(v, str) else "B%d_H%d_s%d_C%d_Cp%d" % v)
def test_window_attention(case, kind, prec):
    d = R.wa_data(case, kind, prec)
    ref, bound = R.wa_ref(case, d), R.wa_bound(case, d, prec)
    r = judge(ref, bound, R.wa_f32(case, d, prec), R.wa_mutants(case, d), R.wa_required(case, kind), f"window attention {case} {kind} {prec}")
    print(f"window attention {case} {kind} {prec}: float32 evaluation at {r:.2f} of the bound")
    if kind == "leak":
        # the leak premise in the operand type: the masked pairs' scores exceed the query's in-region scores by 100 .. 200
        qq, kk, vv, bias, m = R._wa_parts(case, d, torch.float64)
        s = qq @ kk.transpose(-2, -1) + bias
        lq = (qq[..., 0] == R.LEAK * R.SCALE) & (qq[..., 1] == R.LEAK * R.SCALE)
        masked = (m != 0) & lq[..., None]
        inreg = (m == 0) & lq[..., None]
        assert bool(masked.any())
        top_in = torch.where(inreg, s, torch.full_like(s, -1e9)).amax(-1, keepdim=True)
        leak = (kk[..., 0] == R.LEAK) & (kk[..., 1] == R.LEAK)
        gap = (s - top_in)[masked & leak[..., None, :]]
        assert gap.numel() and 100 < gap.min().item() and gap.max().item() < 200, (gap.min().item(), gap.max().item())
        hard = R.wa_mutants(case, d)["mask_hard"]
        assert bool(((hard - ref).abs() > bound).any())


@pytest.mark.parametrize("case", [c for c in R.WA_CASES if c[2]], ids=lambda c: "B%d_H%d_s%d_C%d_Cp%d" % c)
def test_mask_split_at_h_minus_shift_only_is_the_same_mask(case):
    B, H, shift, C, Cp = case
    ours = R._mask_of(R.region_ids(H, shift, cuts=(H - shift,)))
    assert torch.equal(ours, R.region_mask(H, H, R.WS, shift, torch.float64))
    assert torch.equal(R._mask_of(R.region_ids(H, shift)), R.region_mask(H, H, R.WS, shift, torch.float64))
    assert not R._mask_of(R.region_ids(H, shift, cuts=(H - R.WS,))).any()        # a split at H - 7 only is no mask at all


def test_window_attention_cases_reach_their_edges():
    patterns = {c: len({tuple(w.flatten().tolist()) for w in R.region_mask(c[1], c[1], 7, c[2], torch.float64)}) for c in R.WA_CASES if c[2]}
    assert patterns[(3, 14, 3, 96, 128)] == 4
    ids = R.windows(R.region_ids(14, 3).double().view(1, 14, 14, 1), 7).squeeze(-1)
    assert len(set(ids[3].tolist())) == 4 and len(set(ids[0].tolist())) == 1
    m21 = R.region_mask(21, 21, 7, 3, torch.float64)
    assert not m21[4].any() and m21[5].any() and m21[8].any()                     # an interior unmasked window beside masked ones


@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("B,HW,C,Cp,kind", R.HEAD_CASES)
def test_head(B, HW, C, Cp, kind, l2):
    d = R.head_data(B, HW, C, Cp, kind)
    ref = R.head_ref(d, l2)
    if kind == "zero":
        assert not ref.any()
        want = ["clamp_left_out"] if l2 else []
        m = R.head_mutants(d, l2, Cp, kind)
        assert not l2 or m["clamp_left_out"].isnan().all()
        judge(ref, R.head_bound(d, l2), R.head_f32(d, l2), m, want, f"head zero {l2}")
        return
    want = ["mean_over_HW_plus_1", "unbiased_variance"] + (["mean_before_norm"] if HW > 1 else []) + (["l2_norm_over_Cp"] if l2 and C < Cp else [])
    if l2:
        want.remove("mean_over_HW_plus_1")                                        # a common factor: F.normalize removes it
    r = judge(ref, R.head_bound(d, l2), R.head_f32(d, l2), R.head_mutants(d, l2, Cp, kind), want, f"head {B} {HW} {C} {Cp} {l2}")
    print(f"head B={B} HW={HW} C={C} Cp={Cp} l2={l2}: float32 evaluation at {r:.2f} of the bound")


ROLES = R.linear_roles()


def lin_required(epi, prec, M):
    want = ["bias_indexed_by_row", "last_k_chunk_dropped"]
    if epi == R.EPI_BIAS_RESID:
        want.append("residual_added_twice")
    if epi == R.EPI_BIAS_GELU:
        want.append("tanh_gelu")
    if M > R.ROW_TILE[prec]:
        want.append("last_row_tile_duplicated")
    return want


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("mi", range(4), ids=R.LINEAR_ROW_IDS)
@pytest.mark.parametrize("name,N,K,epi", ROLES, ids=[r[0] for r in ROLES])
def test_linear(name, N, K, epi, mi, prec):
    M = R.linear_rows(prec)[mi]
    for zero_bias in ([True, False] if epi == R.EPI_BIAS_F32 else [False]):
        d = R.lin_data(N, K, M, epi, prec, zero_bias=zero_bias)
        want = lin_required(epi, prec, M)
        if zero_bias:
            want.remove("bias_indexed_by_row")
        r = judge(R.lin_ref(d, epi), R.lin_bound(d, epi, prec), R.lin_f32(d, epi, prec), R.lin_mutants(d, epi, prec), want,
                  f"{name} M={M} {prec}")
        print(f"linear {name} N={N} K={K} M={M} {prec}{' zero bias' if zero_bias else ''}: float32 evaluation at {r:.2f} of the bound")


def test_linear_roles_and_tiles_are_the_sources():
    """17 distinct (N, K) over 19 roles, as build_swin lays them out; the row tiles and K-stages read from the GEMM sources; every
    16-bit pair dispatches to gemm2 (N % 128 == 0, K % 64 == 0, K >= 128), every fp32 pair to gemm_nt."""
    assert len(ROLES) == 19 and len({(n, k) for _, n, k, _ in ROLES}) == 17
    assert {k for _, _, k, _ in ROLES} >= {256, 768, 3072}
    src = lambda f: open(os.path.join(ROOT, "effocr_amd", "csrc", f)).read()
    assert int(re.search(r"constexpr int G2M = (\d+)", src("gemm2.hip")).group(1)) == R.ROW_TILE["bf16"] == R.ROW_TILE["fp16"]
    t = src("tile128.hpp")
    assert int(re.search(r"constexpr int BM = (\d+)", t).group(1)) == R.ROW_TILE["fp32"]
    assert int(re.search(r"constexpr int ROWB = (\d+)", t).group(1)) == 4 * R.K_CHUNK["fp32"] == 2 * R.K_CHUNK["bf16"]
    assert "N % G2N == 0 && K >= 128 && K % 64 == 0" in src("gemm2.hip")
    assert all(n % 128 == 0 and k % 64 == 0 and k >= 128 for _, n, k, _ in ROLES)
    body = src("common.hpp").split("float gelu_erf_fast(float x)")[1].split("const float h")[0].split("z * z;")[1]
    coef = re.findall(r"(-?\d[0-9.]*(?:e[+-]?\d+)?)f\b", body)
    assert [float(c) for c in coef] == R._FAST_C
    assert 1.0e-5 < R.ERF_FAST_ABS <= 2.3e-5                                    # common.hpp: |abs err| <= 2.3e-5


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("epi", [R.EPI_BIAS, R.EPI_BIAS_RESID, R.EPI_BIAS_F32])
def test_linear_exact_data_premise(epi, prec):
    d = R.lin_data(384, 128, 130, epi, prec, kind="exact")
    assert_exact_premise(d["x"].abs().double() @ d["w"].abs().double().T, d["bias"], d["resid"])
    assert torch.equal(R.round_to(d["x"], R.DTYPE[prec]), d["x"]) and torch.equal(R.round_to(d["w"], R.DTYPE[prec]), d["w"])
    check_exact(R.lin_f32(d, epi, prec), R.lin_ref(d, epi))
