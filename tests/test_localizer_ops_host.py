"""-m "not gpu": the comparisons of tests/test_gpu_localizer_ops.py judged on the CPU.  For every operator of tests/localizer_ops_ref.py a
float32 torch evaluation lies inside the derived bound on every case the GPU test runs, and every mutant (the float64 result corrupted
the way a kernel could be wrong) is rejected on at least one case — on every case it applies to, but for the ones whose damage needs
particular data (`NEEDS`).  Also: the header / export / argument checks of the new test entry points."""
import ctypes
import os
import re

import pytest
import torch

from effocr_amd import _lib
from tests import convops_lib as CL
from tests import localizer_ops_ref as R
from tests.convops_ref import Mismatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rejected(fn):
    try:
        fn()
    except Mismatch:
        return True
    return False


# ------------------------------------------------------------------------------------------------------------------- YOLOv8 decode
# The data kinds on which a mutant must show; every other mutant shows on every kind.  A missing max-subtraction shows only where fp32's
# expf leaves its range; with all logits equal every distance is 7.5, the middle of the bins, and the four sides are alike.
_UNEQUAL = ("normal", "peaked", "shift+100", "shift-100")
NEEDS = {"no_max_subtraction": ("shift+100", "shift-100"), "bins_reversed": _UNEQUAL, "left_right_swapped": _UNEQUAL, "top_bottom_swapped": _UNEQUAL}


@pytest.mark.parametrize("kind", R.V8_KINDS)
@pytest.mark.parametrize("case", R.V8_CASES, ids=lambda c: c.name)
def test_v8_decode(case, kind):
    d = R.v8_data(case, kind)
    ref, bound, own = R.v8_ref(case, d), R.v8_bound(case, d), R.v8_own(case)
    assert torch.isfinite(bound[own]).all() and (bound[own] > 0).all()
    R.check_owned(R.v8_variant(case, d), ref, torch.full_like(ref, 1e-9), own, "the step-by-step restatement against yolov8_ref.decode")
    r = R.check_owned(R.v8_f32(case, d).double(), ref, bound, own, f"{case.name} {kind} float32 evaluation")
    split = R.column_ratios(R.v8_f32(case, d), ref, bound, own, R.ROW_GROUPS)
    print(f"yolov8_decode {case.name} {kind}: float32 evaluation at {r:.2f} of the bound (box {split['box']:.2f}, scores {split['scores']:.2f})")
    for m in R.V8_MUTANTS:
        if R.v8_applies(case, m) and kind in NEEDS.get(m, R.V8_KINDS):
            assert rejected(lambda: R.check_owned(R.v8_variant(case, d, m), ref, bound, own, m)), f"{case.name} {kind}: mutant {m} passes"


def test_v8_every_mutant_is_rejected_somewhere_and_the_cases_reach_their_edges():
    seen = set()
    for case in R.V8_CASES:
        for kind in R.V8_KINDS:
            d = R.v8_data(case, kind)
            ref, bound, own = R.v8_ref(case, d), R.v8_bound(case, d), R.v8_own(case)
            seen |= {m for m in R.V8_MUTANTS if R.v8_applies(case, m) and rejected(lambda: R.check_owned(R.v8_variant(case, d, m), ref, bound, own, m))}
    assert seen == set(R.V8_MUTANTS), sorted(set(R.V8_MUTANTS) - seen)
    a, b, c, e, f, g = R.V8_CASES
    assert a.B * a.A == 1 and b.before and b.after and c.box_ld > 64 and c.cls_ld > c.nc > 4
    assert e.A == 63 and f.A == 65 and g.B * g.A * 4 == 512 and g.nc == 80
    peak = R.v8_data(c, "peaked")["box"][:, :64].reshape(-1, 16).argmax(1)
    assert {0, 15} <= set(peak.tolist())
    # the premise of the issue: the peaked distances are the peak's bin, the equal ones 7.5
    assert torch.allclose(R.v8_ref(a, R.v8_data(a, "equal"))[0, 0, 2:4], torch.tensor([15.0, 15.0], dtype=torch.float64) * a.stride)


@pytest.mark.parametrize("kind", R.V8_NONFINITE)
def test_v8_nonfinite_reference(kind):
    """One NaN / +inf logit poisons its side: cx and w (the left side) of that point are NaN in float64 and in float32, nothing else is."""
    case = R.V8_CASES[2]
    d = R.v8_data(case, kind)
    ref, own = R.v8_ref(case, d), R.v8_own(case)
    bad = (~torch.isfinite(ref) & own).nonzero().tolist()
    P = case.B * case.A // 2
    assert bad == [[P // case.A, case.before + P % case.A, 0], [P // case.A, case.before + P % case.A, 2]]
    clean = R.v8_bound(case, R.v8_data(case, "normal"))
    r = R.check_owned(R.v8_f32(case, d).double(), ref, clean, own, f"{kind} float32", nonfinite=True)
    assert r < 1
    with pytest.raises(Mismatch, match="non-finite"):
        got = R.v8_f32(case, d).double()
        got[own] = torch.nan_to_num(got[own], nan=3.0)                                       # a maximum that drops the NaN, say
        R.check_owned(got, ref, clean, own, kind, nonfinite=True)


# ------------------------------------------------------------------------------------------------------------------- YOLOv5 decode
@pytest.mark.parametrize("case", R.V5_CASES, ids=lambda c: c.name)
def test_v5_decode(case):
    d = R.v5_data(case)
    ref, bound, own = R.v5_ref(case, d), R.v5_bound(case, d), R.v5_own(case)
    assert torch.isfinite(bound[own]).all() and (bound[own] > 0).all()
    R.check_owned(R.v5_variant(case, d), ref, torch.full_like(ref, 1e-9), own, "the element-by-element restatement against Detect")
    r = R.check_owned(R.v5_f32(case, d).double(), ref, bound, own, f"{case.name} float32 evaluation")
    print(f"yolo_decode {case.name}: float32 evaluation at {r:.2f} of the bound")
    for m in R.V5_MUTANTS:
        if R.v5_applies(case, m) and case.kind == "normal":
            assert rejected(lambda: R.check_owned(R.v5_variant(case, d, m), ref, bound, own, m)), f"{case.name}: mutant {m} passes"


def test_v5_every_mutant_is_rejected_somewhere_and_the_cases_reach_their_edges():
    seen = set()
    for case in R.V5_CASES:
        d = R.v5_data(case)
        ref, bound, own = R.v5_ref(case, d), R.v5_bound(case, d), R.v5_own(case)
        seen |= {m for m in R.V5_MUTANTS if R.v5_applies(case, m) and rejected(lambda: R.check_owned(R.v5_variant(case, d, m), ref, bound, own, m))}
    assert seen == set(R.V5_MUTANTS), sorted(set(R.V5_MUTANTS) - seen)
    assert {c.no for c in R.V5_CASES} == {6, 7, 10} and all(c.ny != c.nx for c in R.V5_CASES)
    assert {c.raw_ld == 3 * c.no for c in R.V5_CASES} == {True, False} and all(c.raw_ld % 32 == 0 for c in R.V5_CASES if c.padded)
    assert any(c.before and c.after for c in R.V5_CASES) and all(c.B * c.A * c.no % 256 for c in R.V5_CASES)
    assert len(set(R.ANCHORS_PX)) == 3 and all(w != h for w, h in R.ANCHORS_PX)
    sat = R.v5_data(R.V5_CASES[-1])["raw"]
    assert {90.0, -90.0, 200.0, -200.0} <= set(sat[~sat.isnan()].tolist())


# ------------------------------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("case", R.STEM_CASES, ids=lambda c: c.name)
def test_stem(case):
    d = R.stem_data(case)
    ref, bound = R.stem_ref(case, d), R.stem_bound(case, d)
    R.check_stem(case, R.stem_variant(case, d).float(), ref, bound + 1e-6, "the padded restatement against conv_reference")
    r = R.check_stem(case, R.stem_f32(case, d), ref, bound, f"{case.name} float32 evaluation")
    print(f"stem3x3s2 {case.name}: float32 evaluation at {r:.2f} of the bound")
    for m in R.STEM_MUTANTS:
        if R.stem_applies(case, m):
            assert rejected(lambda: R.check_stem(case, R.stem_variant(case, d, m).float(), ref, bound, m)), f"{case.name}: mutant {m} passes"
    wt, b = R.pack_stem(case, d)
    assert wt.shape == (27, case.wt_ld) and not wt[:, :case.cout].isnan().any() and not b[case.cout:].any()
    assert torch.equal(wt[(1 * 3 + 2) * 3 + 1, :case.cout], d["w"][:, 1, 1, 2])           # row (ky 3 + kx) 3 + c


def test_stem_cases_and_nonfinite_reference():
    assert {m for c in R.STEM_CASES for m in R.STEM_MUTANTS if R.stem_applies(c, m)} == set(R.STEM_MUTANTS)
    a, b, c, e, f = R.STEM_CASES
    assert a.H % 2 and a.W % 2 and a.cout_st - a.cout == 16 and b.out_off and b.out_ld > b.cout_st
    assert c.OH == 1 and c.wt_ld > c.cout_st and e.cout_st // 16 > 1 and f.M // 4 > 256 and all(x.OW % 4 == 0 for x in R.STEM_CASES)
    d, clean = R.stem_data(a, nonfinite=True), R.stem_data(a)
    ref, bound = R.stem_ref(a, d), R.stem_bound(a, clean)
    nf = ~torch.isfinite(ref) & R.stem_own(a)
    assert nf.any() and ref[nf].isnan().any() and torch.isinf(ref[nf]).any()               # NaN from the NaN pixel and from SiLU(-inf); +inf
    assert nf.reshape(a.B, a.OH, a.OW, -1)[0, 0, 0, :a.cout].all() and nf.reshape(a.B, a.OH, a.OW, -1)[-1, -1, -1, :a.cout].all()
    assert int(nf.sum()) == 2 * a.cout                                                     # one window each
    R.check_stem(a, R.stem_f32(a, d), ref, bound, "nonfinite float32", nonfinite=True)


# ------------------------------------------------------------------------------------------------------------------- box stage
BOX_FORMS = [(False, 0), (True, 1), (True, 0)]                                             # (vertical, axis)


@pytest.mark.parametrize("L", R.BOX_LINES)
@pytest.mark.parametrize("max_det", R.BOX_MAX_DETS)
def test_box_stage_two_statements_agree(max_det, L):
    """The plain-Python restatement of the driver and the ATen expression (on CPU tensors) give the same boxes, counts and crops."""
    vertical, axis = BOX_FORMS[(max_det + L) % 3]
    rows, counts = R.boxes_data(max_det, L)
    want = R.boxes_ref(rows, counts, max_det, R.BOX_H, R.BOX_W, axis, vertical)
    R.check_boxes(R.boxes_torch(rows, counts, max_det, R.BOX_H, R.BOX_W, axis, vertical), want, f"max_det {max_det} L {L}")
    assert want[3] == int(want[1].sum()) and (want[2][want[3]:] == R.SENTINEL).all() and (want[2][:want[3]] != R.SENTINEL).all()
    if L == 40:
        n = want[1].tolist()
        assert n[3] == 0 and n[5] == 0 and n[6] == 0 and n[4] == max_det and n[2] <= max_det


@pytest.mark.parametrize("vertical,axis", BOX_FORMS)
def test_box_stage_mutants(vertical, axis):
    seen = set()
    for max_det in (5, 65):
        rows, counts = R.boxes_data(max_det, 40)
        want = R.boxes_ref(rows, counts, max_det, R.BOX_H, R.BOX_W, axis, vertical)
        for m in R.BOX_MUTANTS:
            if rejected(lambda: R.check_boxes(R.boxes_ref(rows, counts, max_det, R.BOX_H, R.BOX_W, axis, vertical, fault=m), want, m)):
                seen.add(m)
    assert seen == set(R.BOX_MUTANTS), sorted(set(R.BOX_MUTANTS) - seen)


def test_box_stage_nan_keys():
    """NaN in the sort-key column only (axis 1 of horizontal lines): torch.sort's order — behind every number and behind the rows that
    are no characters — is the reference; ranking them first is rejected."""
    for max_det in (5, 65):
        rows, counts = R.boxes_data(max_det, 40, nan_keys=True)
        assert rows[..., 1].isnan().any() and torch.isfinite(rows[..., [0, 2, 3, 4, 5]]).all()
        want = R.boxes_torch(rows, counts, max_det, R.BOX_H, R.BOX_W, 1, False)
        assert want[0].isnan().any()
        with pytest.raises(Mismatch):
            R.check_boxes(R.boxes_torch(rows, counts, max_det, R.BOX_H, R.BOX_W, 1, False, nan_first=True), want, "nan first")
        # the NaN rows are a permutation's: every input row appears once in the sorted boxes
        for l in (0, 7):
            key = lambda t: sorted(map(str, t.tolist()))
            assert key(want[0][l]) == key(rows[l, :, :4])


# ------------------------------------------------------------------------------------------------------------------- entry points
def test_entry_points_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "effocr_yolov8.h")).read()
    declared = set(re.findall(r"\b(effocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    assert {"effocr_yolov8_op_decode", "effocr_yolov8_op_stem"} <= declared and declared == set(_lib.YOLOV8_EXPORTS)
    L = _lib.yolov8_lib()
    assert L.effocr_yolov8_op_decode.argtypes[9] is ctypes.c_float and L.effocr_yolov8_op_decode.argtypes[10] is ctypes.c_int64
    assert not any("_op_decode" in k or "_op_stem" in k for k in _lib.YOLO11_EXPORTS)       # one library under test is enough
    api = open(os.path.join(ROOT, "effocr_amd", "csrc", "convops_api.hip")).read()
    assert int(re.search(r"#define\s+EFFOCR_CONVOPS_ABI_VERSION\s+(\d+)", api).group(1)) == CL.ABI_VERSION == CL.lib().effocr_convops_abi_version() == 4
    assert "effocr_convops_yolo_decode" in CL.EXPORTS
    _lib.lib()
    assert "effocr_parse_char_boxes" in _lib.EXPORTS


def test_entry_points_check_their_arguments():
    """Refused on the host, before any launch: NULL and bad geometry -> -1, what the launcher cannot do -> its own code and message."""
    L, C = _lib.yolov8_lib(), CL.lib()
    p, s = ctypes.c_void_p(4096), None                                                       # (never dereferenced)
    dec = L.effocr_yolov8_op_decode
    assert dec(None, 64, p, 4, p, 1, 2, 2, 1, 8.0, 4, 0, s) == -1 and b"NULL" in L.effocr_yolov8_last_error()
    assert dec(p, 64, None, 4, p, 1, 2, 2, 1, 8.0, 4, 0, s) == -1
    assert dec(p, 64, p, 4, None, 1, 2, 2, 1, 8.0, 4, 0, s) == -1
    assert dec(p, 60, p, 4, p, 1, 2, 2, 1, 8.0, 4, 0, s) == -1                              # box_ld < 64
    assert dec(p, 64, p, 4, p, 1, 2, 2, 5, 8.0, 4, 0, s) == -1                              # cls_ld < nc
    assert dec(p, 64, p, 4, p, 1, 0, 2, 1, 8.0, 4, 0, s) == -1
    assert dec(p, 64, p, 4, p, -1, 2, 2, 1, 8.0, 4, 0, s) == -1
    assert dec(p, 66, p, 4, p, 1, 2, 2, 1, 8.0, 4, 0, s) == -1 and b"multiple of 4" in L.effocr_yolov8_last_error()   # the launcher's
    assert dec(p, 64, p, 4, p, 1, 2, 2, 1, 8.0, 4, 1, s) == -1 and b"do not fit" in L.effocr_yolov8_last_error()
    assert dec(p, 64, p, 4, p, 1, 2, 2, 1, 8.0, 4, -1, s) == -1
    assert dec(p, 64, p, 4, p, 0, 2, 2, 1, 8.0, 4, 0, s) == 0                               # an empty batch launches nothing
    stem = L.effocr_yolov8_op_stem
    ok = dict(x=p, wt=p, wt_ld=32, bias=p, out=p, B=1, H=8, W=8, OH=4, OW=4, out_ld=32, out_off=0, cout=16, cout_st=32)
    call = lambda **kw: stem(*{**ok, **kw}.values(), s)
    for k in ("x", "wt", "bias", "out"):
        assert call(**{k: None}) == -1 and b"NULL" in L.effocr_yolov8_last_error()
    assert call(wt_ld=34) == -1 and call(H=0) == -1 and call(out_off=-4) == -1 and call(B=-1) == -1
    assert call(OH=5) == -1 and b"ceil(input / 2)" in L.effocr_yolov8_last_error()
    assert call(B=0) == 0
    for c0 in R.STEM_CASES[:1]:
        base = dict(wt_ld=c0.wt_ld, B=c0.B, H=c0.H, W=c0.W, OH=c0.OH, OW=c0.OW, out_ld=c0.out_ld, out_off=c0.out_off, cout=c0.cout, cout_st=c0.cout_st)
        for over, msg in R.STEM_REFUSED:
            kw = {**base, **over}
            kw["OH"], kw["OW"] = (kw["H"] - 1) // 2 + 1, (kw["W"] - 1) // 2 + 1
            assert call(**kw) == -2 and msg.encode() in L.effocr_yolov8_last_error(), over
    v5 = C.effocr_convops_yolo_decode
    anc = (ctypes.c_float * 6)(*[v for a in R.ANCHORS_PX for v in a])
    assert v5(None, 18, p, 1, 2, 3, 3, 6, 8.0, anc, 18, 0, s) == -1 and "NULL" in CL.last_error()
    assert v5(p, 18, None, 1, 2, 3, 3, 6, 8.0, anc, 18, 0, s) == -1
    assert v5(p, 18, p, 1, 2, 3, 3, 6, 8.0, None, 18, 0, s) == -1
    assert v5(p, 17, p, 1, 2, 3, 3, 6, 8.0, anc, 18, 0, s) == -1                            # raw_ld < na * no
    assert v5(p, 18, p, 1, 2, 3, 3, 4, 8.0, anc, 18, 0, s) == -1
    assert v5(p, 18, p, 1, 2, 3, 3, 6, 8.0, anc, 17, 0, s) == -1 and "do not fit" in CL.last_error()
    assert v5(p, 18, p, 1, 2, 3, 3, 6, 8.0, anc, 18, 1, s) == -1
    assert v5(p, 12, p, 1, 2, 3, 2, 6, 8.0, anc, 12, 0, s) == -2 and "three anchors per level" in CL.last_error()
    assert v5(p, 18, p, 0, 2, 3, 3, 6, 8.0, anc, 18, 0, s) == 0
    H = _lib.lib()
    assert H.effocr_parse_char_boxes(p, p, 1, 4097, 32, 32, 0, 0, p, p, p, p, s) == -2
    assert H.effocr_parse_char_boxes(p, p, 1, 64, 32, 32, 2, 0, p, p, p, p, s) == -1
