"""-m "not gpu": the comparisons of tests/test_gpu_mobilenetv3_ops.py judged on the CPU.  For every case the GPU test runs, every
applicable mutant of tests/mobilenetv3_ops_ref.py (a float64 result corrupted the way a kernel could be wrong) lies outside the derived
bound somewhere, and a float32 torch evaluation of the same operator lies inside it everywhere.  Also: the packing the GPU test hands
mg_pw, and the restatement's round_pw path."""
import ctypes

import pytest
import torch

from effocr_amd import _lib
from tests import mobilenetv3_ops_ref as R
from tests.convops_ref import Mismatch, check_bound, check_exact

PRECS = ["fp32", "fp16", "bf16"]


def judge(ref, bound, f32, mutants, expected, what):
    """Mutants outside, the float32 evaluation inside.  `expected`: the mutant names the case must have."""
    assert set(expected) <= set(mutants), f"{what}: mutants {sorted(set(expected) - set(mutants))} do not apply — change the case's data or shape"
    assert torch.isfinite(ref).all() and torch.isfinite(bound).all() and (bound >= 0).all()
    ratio = check_bound(f32.double(), ref, bound, what + " float32 evaluation")
    for name, y in mutants.items():
        with pytest.raises(Mismatch):
            check_bound(y, ref, bound, f"{what} {name}")
    return ratio


@pytest.mark.parametrize("S,B", R.STEM_CASES)
def test_stem(S, B):
    d = R.stem_data(S, B)
    r = judge(R.stem_ref(d), R.stem_bound(d), R.stem_f32(d), R.stem_mutants(d),
              ["taps_transposed", "pad_off_by_one", "window_one_pixel_late"], f"stem {S} {B}")
    print(f"mg_stem S={S} B={B}: float32 evaluation at {r:.2f} of the bound")


@pytest.mark.parametrize("case", R.DW_CASES, ids=lambda c: c.name)
def test_dw(case):
    d = R.dw_data(case)
    want = ["pad_off_by_one"] + (["taps_transposed"] if case.H > 1 else []) + (["window_one_pixel_late"] if case.stride == 2 else [])
    r = judge(R.dw_ref(case, d), R.dw_bound(case, d), R.dw_f32(case, d), R.dw_mutants(case, d), want, case.name)
    print(f"mg_dw {case.name}: float32 evaluation at {r:.2f} of the bound")
    # the last workgroup is partly idle in every case but the first (768 threads: three full workgroups, the only full last one)
    assert (case.B * case.Ho * case.Ho * case.C // 4) % 256 or case == R.DW_CASES[0]


@pytest.mark.parametrize("B,C,Rr,HW", R.SE_CASES)
def test_se_gate(B, C, Rr, HW):
    d = R.se_data(B, C, Rr, HW)
    want = ["mean_drops_last_pixel", "reduce_weight_transposed", "expand_weight_transposed"] + (["mean_of_neighbouring_crop"] if B > 1 else [])
    ref = R.se_ref(d)
    r = judge(ref, R.se_bound(d), R.se_f32(d), R.se_mutants(d), want, f"se {B} {C} {Rr} {HW}")
    live = ((ref > 0.02) & (ref < 0.98)).float().mean().item()
    print(f"mg_se_gate B={B} C={C} R={Rr} HW={HW}: float32 evaluation at {r:.2f} of the bound; {live:.0%} of the gates off the clamps")
    assert live > 0.5                                                           # the hard-sigmoid does not hide the FC layers


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", R.PW_CASES, ids=lambda c: c.name)
def test_pw(case, prec):
    d = R.pw_data(case, prec)
    want = ((["last_k_quad_dropped"] if case.K % 16 else []) + (["last_n_tile_shifted_4"] if case.N % 16 else [])
            + (["gate_left_out"] if case.gate else []) + (["gate_of_neighbouring_crop"] if case.gate and case.crops > 1 else [])
            + (["residual_left_out"] if case.resid else [])
            + (["activation_after_residual"] if case.resid and case.act != R.ACT_NONE else [])
            + (["lo_part_dropped"] if prec != "fp32" else []))
    r = judge(R.pw_ref(case, d), R.pw_bound(case, d, prec), R.pw_f32(case, d), R.pw_mutants(case, d, prec), want, f"{case.name} {prec}")
    print(f"mg_pw {case.name} {prec}: float32 evaluation at {r:.2f} of the bound")
    w = R.pack_pw_w(d["w"], prec)
    if prec != "fp32":
        assert w.shape == ((case.N + 15) // 16 * 16, (case.K + 15) // 16 * 16) and w.dtype == R.DTYPE[prec]
        assert not w[case.N:].any() and not w[:, case.K:].any()


def test_pw_cases_reach_their_edges():
    """What the issue's table says each shape reaches, from the kernel's tiling: 64 rows per workgroup, 16 per wave, 4 n-tiles of 16 per
    block column, 16 k per MFMA step."""
    c = {x.name: x for x in R.PW_CASES}
    a, b, _, h, e, f = R.PW_CASES
    assert a.K == 8 and (a.K + 15) // 16 * 16 == 16                             # three of four k-quads outside K
    assert b.crops == 3 and b.M % 64 == 19 and b.HW % 16 and b.N % 16 == 8 and (b.N + 15) // 16 == 3
    assert (h.N + 15) // 16 // 4 == 20
    assert e.M == 65 and (e.N + 15) // 16 == 6 and e.N % 16 == 8                 # block column 1 holds tiles 4, 5; tiles 6, 7 absent
    assert f.act == R.ACT_SILU and f.gate
    assert sum(1 for x in R.PW_CASES if x.K % 16) >= 3 and len(c) == len(R.PW_CASES)


def test_split_premise_is_checked():
    case = R.PW_CASES[1]
    d = R.pw_data(case, "fp16")
    d["a"][5, 3] = 0.01
    with pytest.raises(AssertionError, match="2\\^-3"):
        R.pw_bound(case, d, "fp16")
    R.pw_bound(case, d, "bf16")


@pytest.mark.parametrize("B,HW,C", R.POOL_CASES)
def test_pool(B, HW, C):
    d = R.pool_data(B, HW, C)
    want = ["divided_by_wrong_count", "neighbouring_crop"] + (["last_pixel_dropped"] if HW > 1 else [])
    m = R.pool_mutants(d)
    r = judge(R.pool_ref(d), R.pool_bound(d), R.pool_f32(d), m, want, f"pool {B} {HW} {C}")
    print(f"mg_pool B={B} HW={HW} C={C}: float32 evaluation at {r:.2f} of the bound")


@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("D", R.FINISH_DIMS)
def test_finish(D, l2):
    d = R.finish_data(D)
    ref, bound = R.finish_ref(d, l2), R.finish_bound(d, l2)
    want = ["norm_misses_last_column", "norm_not_rooted", "norm_of_neighbouring_row"] if l2 else []
    r = judge(ref, bound + (0 if l2 else 1e-300), R.finish_f32(d, l2), R.finish_mutants(d, l2), want, f"finish {D} {l2}")
    assert not ref[1].any()                                                     # the all-zero row stays 0
    if l2:
        assert torch.allclose(ref[[0, 2, 3]].norm(dim=1), torch.ones(3, dtype=torch.float64), atol=1e-12)
        print(f"mg_finish D={D}: float32 evaluation at {r:.2f} of the bound")
    else:
        check_exact(R.finish_f32(d, l2), ref)


def test_nonfinite_comparison_rejects_a_fmaxf_relu():
    """check_nonfinite sees what the kernels did before the fix: a NaN turned into 0 by a maximum that drops it."""
    x = torch.tensor([[1.0, float("nan"), -2.0, float("inf"), float("-inf")]])
    want = torch.relu(x.double())
    assert R.check_nonfinite(torch.relu(x), want) == 2
    with pytest.raises(Mismatch, match="got 0.0, want nan"):
        R.check_nonfinite(torch.nan_to_num(torch.relu(x), nan=0.0, posinf=float("inf")), want)
    with pytest.raises(Mismatch):
        R.check_nonfinite(torch.tensor([[1.0, float("nan"), 0.0, float("nan"), 0.0]]), want)      # an inf that came out as NaN


def test_entry_points_check_their_arguments():
    """Every effocr_mnv3_op_* call below is refused on the host, before any launch: NULL -> -1, what the kernel cannot do -> -2."""
    L = _lib.mnv3_lib()
    p, s = ctypes.c_void_p(4096), None                                           # (never dereferenced)
    assert L.effocr_mnv3_op_stem(None, 1, 32, p, p, p, s) == -1
    assert L.effocr_mnv3_op_stem(p, 1, 31, p, p, p, s) == -2                      # odd S
    assert L.effocr_mnv3_op_dw(p, 1, 8, 16, 3, 1, p, p, 1, None, s) == -1
    assert L.effocr_mnv3_op_dw(p, 1, 8, 18, 3, 1, p, p, 1, p, s) == -2            # C % 4
    assert L.effocr_mnv3_op_dw(p, 1, 8, 16, 7, 1, p, p, 1, p, s) == -2            # k not 3 / 5
    assert L.effocr_mnv3_op_dw(p, 1, 8, 16, 4, 1, p, p, 1, p, s) == -2
    assert L.effocr_mnv3_op_dw(p, 1, 8, 16, 3, 3, p, p, 1, p, s) == -2            # stride not 1 / 2
    assert L.effocr_mnv3_op_se_gate(p, 1, 4, 16, 8, p, None, p, p, p, s) == -1
    for B, C, Rr, HW in R.SE_REFUSED:
        assert L.effocr_mnv3_op_se_gate(p, B, HW, C, Rr, p, p, p, p, p, s) == -2  # C = 1028, R = 260: beyond the LDS tables
        assert b"LDS" in L.effocr_mnv3_last_error()
    assert L.effocr_mnv3_op_pw(2, p, 4, 16, None, 16, p, None, 1, 0, None, p, s) == -1
    assert L.effocr_mnv3_op_pw(3, p, 4, 16, p, 16, p, None, 1, 0, None, p, s) == -1
    assert L.effocr_mnv3_op_pw(2, p, 4, 18, p, 16, p, None, 1, 0, None, p, s) == -2   # K % 4
    assert L.effocr_mnv3_op_pw(1, p, 4, 16, p, 18, p, None, 1, 0, None, p, s) == -2   # N % 4
    assert L.effocr_mnv3_op_pool(p, 1, 4, 16, None, s) == -1
    assert L.effocr_mnv3_op_pool(p, 0, 4, 16, p, s) == -1
    assert L.effocr_mnv3_op_finish(p, 1, 1024, 1, None, s) == -1
    assert L.effocr_mnv3_op_finish(None, 1, 1024, 1, p, s) == -1
