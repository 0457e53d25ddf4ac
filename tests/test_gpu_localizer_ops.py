"""The localizer tail on the MI355X (-m gpu), one launch per case: both Detect decodes, the YOLOv8 stem and the box stage against the
float64 / plain-Python restatements of tests/localizer_ops_ref.py, within bounds derived from the arithmetic
(tests/test_localizer_ops_host.py shows on the CPU that each bound rejects every mutant of its operator).  Output buffers are pre-filled
with NaN (the integer ones with a sentinel): every element the operator owns must be written, every other one must still be NaN.

yolov8_decode_kernel and stem3x3s2_g16_kernel run through libeffocr_yolov8.so's effocr_yolov8_op_decode / _op_stem.
libeffocr_yolo11.so links the same yolov8.fam.o — the same object file, so the same kernels — and is not run a second time here.
yolo_decode_kernel runs through the test library's effocr_convops_yolo_decode, the box stage through the product library's
effocr_parse_char_boxes.

Non-finite data.  A NaN or +inf logit makes its side's distance NaN in the kernel as in torch (the kernel's fmaxf drops a NaN from the
maximum, but expf(NaN - max) brings it back; inf - inf is NaN in both), and a NaN / inf pixel gives the stem torch's values (SiLU(-inf)
is NaN in both): no difference from torch was found, none is allowed for.

Box stage.  Every coordinate boxes_compact_kernel reads is finite: the conversion of a non-finite float to `long long` is not defined,
and the driver never produces one (NMS rows are products and sums of finite sigmoids).  NaN appears in the sort-key column only, on
horizontal lines sorted along axis 1, whose slices never read that column."""
import ctypes

import pytest
import torch

from effocr_amd import _lib
from tests import convops_lib as CL
from tests import localizer_ops_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _nanbuf(dev, *shape):
    return torch.full(shape, NAN, device=dev)


def _ratio(name, what, r, split=None):
    """Prints the largest error / bound of a case (`split`: per column group as well — the scores' ratio alone would hide the boxes')."""
    assert r < 1
    more = "" if split is None else "  (" + ", ".join(f"{k} {v:.3f}" for k, v in split.items()) + ")"
    print(f"{name} {what}: error / bound {r:.3f}{more}")


# ------------------------------------------------------------------------------------------------------------------- YOLOv8 decode
def run_v8(dev, c, d):
    L = _lib.yolov8_lib()
    box, cls = d["box"].to(dev), d["cls"].to(dev)
    pred = _nanbuf(dev, c.B, c.total, c.no)
    rc = L.effocr_yolov8_op_decode(_lib.ptr(box), c.box_ld, _lib.ptr(cls), c.cls_ld, _lib.ptr(pred), c.B, c.ny, c.nx, c.nc, c.stride, c.total, c.before,
                                   _lib.current_stream(dev))
    assert rc == 0, L.effocr_yolov8_last_error()
    torch.cuda.synchronize(dev)
    return pred.cpu()


@pytest.mark.parametrize("kind", R.V8_KINDS)
@pytest.mark.parametrize("case", R.V8_CASES, ids=lambda c: c.name)
def test_v8_decode(dev, case, kind):
    d = R.v8_data(case, kind)
    got = run_v8(dev, case, d)
    own = R.v8_own(case)
    assert bool((got[own].reshape(-1, case.no)[:, 4] == 1.0).all())
    ref, bound = R.v8_ref(case, d), R.v8_bound(case, d)
    _ratio("yolov8_decode", f"{case.name} {kind}", R.check_owned(got.double(), ref, bound, own, f"yolov8_decode {case.name} {kind}"),
           R.column_ratios(got, ref, bound, own, R.ROW_GROUPS))


@pytest.mark.parametrize("kind", R.V8_NONFINITE)
@pytest.mark.parametrize("case", R.V8_CASES[1:4], ids=lambda c: c.name)
def test_v8_decode_nonfinite(dev, case, kind):
    """A NaN / +inf logit in the left side of one point: exactly the reference's outputs (that row's cx and w) are NaN; every other
    element stays within the bound of the clean data, which it shares with this data."""
    d = R.v8_data(case, kind)
    ref, own = R.v8_ref(case, d), R.v8_own(case)
    assert int((~torch.isfinite(ref) & own).sum()) == 2
    bound = R.v8_bound(case, R.v8_data(case, "normal"))
    _ratio("yolov8_decode", f"{case.name} {kind}", R.check_owned(run_v8(dev, case, d).double(), ref, bound, own, f"yolov8_decode {case.name} {kind}", nonfinite=True))


# ------------------------------------------------------------------------------------------------------------------- YOLOv5 decode
def _v5_call(dev, c, raw, pred, na=3):
    anc = (ctypes.c_float * 6)(*[v for a in R.ANCHORS_PX for v in a])
    return CL.lib().effocr_convops_yolo_decode(CL.ptr(raw), c.raw_ld, CL.ptr(pred), c.B, c.ny, c.nx, na, c.no, c.stride, anc, c.total, c.before,
                                               _lib.current_stream(dev))


@pytest.mark.parametrize("case", R.V5_CASES, ids=lambda c: c.name)
def test_v5_decode(dev, case):
    d = R.v5_data(case)
    raw, pred = d["raw"].to(dev), _nanbuf(dev, case.B, case.total, case.no)
    assert _v5_call(dev, case, raw, pred) == 0, CL.last_error()
    torch.cuda.synchronize(dev)
    got, ref, bound, own = pred.cpu(), R.v5_ref(case, d), R.v5_bound(case, d), R.v5_own(case)
    _ratio("yolo_decode", case.name, R.check_owned(got.double(), ref, bound, own, f"yolo_decode {case.name}"), R.column_ratios(got, ref, bound, own, R.ROW_GROUPS))


def test_v5_decode_refuses_two_anchors(dev):
    case = R.V5_CASES[0]
    raw, pred = R.v5_data(case)["raw"].to(dev), _nanbuf(dev, case.B, case.total, case.no)
    assert _v5_call(dev, case, raw, pred, na=2) == CL.EUNSUPPORTED and "yolo_decode: three anchors per level" in CL.last_error()
    torch.cuda.synchronize(dev)
    assert bool(pred.isnan().all())


# ------------------------------------------------------------------------------------------------------------------- stem
def _stem_call(dev, c, x, wt, b, out, **over):
    a = dict(wt_ld=c.wt_ld, B=c.B, H=c.H, W=c.W, OH=c.OH, OW=c.OW, out_ld=c.out_ld, out_off=c.out_off, cout=c.cout, cout_st=c.cout_st)
    a.update(over)
    return _lib.yolov8_lib().effocr_yolov8_op_stem(_lib.ptr(x), _lib.ptr(wt), a["wt_ld"], _lib.ptr(b), _lib.ptr(out), a["B"], a["H"], a["W"], a["OH"], a["OW"],
                                                   a["out_ld"], a["out_off"], a["cout"], a["cout_st"], _lib.current_stream(dev))


def run_stem(dev, c, d):
    wt, b = R.pack_stem(c, d)
    x, wt, b = d["x"].to(dev), wt.to(dev), b.to(dev)
    out = _nanbuf(dev, c.M, c.out_ld)
    assert _stem_call(dev, c, x, wt, b, out) == 0, _lib.yolov8_lib().effocr_yolov8_last_error()
    torch.cuda.synchronize(dev)
    assert torch.equal(x.cpu().view(torch.int32), d["x"].view(torch.int32)), "the input was modified by the call"
    return out.cpu()


@pytest.mark.parametrize("case", R.STEM_CASES, ids=lambda c: c.name)
def test_stem(dev, case):
    d = R.stem_data(case)
    _ratio("stem3x3s2", case.name, R.check_stem(case, run_stem(dev, case, d), R.stem_ref(case, d), R.stem_bound(case, d), f"stem3x3s2 {case.name}"))


@pytest.mark.parametrize("case", [R.STEM_CASES[0], R.STEM_CASES[2]], ids=lambda c: c.name)
def test_stem_nonfinite(dev, case):
    """One NaN pixel (top-left of the first image) and one inf pixel (bottom-right of the last): the windows that hold them give the
    reference's NaN / +inf / NaN = SiLU(-inf), every other output stays within the clean data's bound."""
    d, clean = R.stem_data(case, nonfinite=True), R.stem_data(case)
    ref = R.stem_ref(case, d)
    assert int((~torch.isfinite(ref) & R.stem_own(case)).sum()) >= 2 * case.cout
    _ratio("stem3x3s2", f"{case.name} nonfinite", R.check_stem(case, run_stem(dev, case, d), ref, R.stem_bound(case, clean), f"stem3x3s2 {case.name} nonfinite",
                                                               nonfinite=True))


def test_stem_refusals(dev):
    c = R.STEM_CASES[0]
    d = R.stem_data(c)
    wt, b = R.pack_stem(c, d)
    x, wt, b, out = d["x"].to(dev), wt.to(dev), b.to(dev), _nanbuf(dev, c.M, c.out_ld)
    L = _lib.yolov8_lib()
    for over, msg in R.STEM_REFUSED:
        a = dict(H=c.H, W=c.W)
        a.update(over)
        a["OH"], a["OW"] = (a["H"] - 1) // 2 + 1, (a["W"] - 1) // 2 + 1
        assert _stem_call(dev, c, x, wt, b, out, **a) == -2 and msg.encode() in L.effocr_yolov8_last_error(), over
    torch.cuda.synchronize(dev)
    assert bool(out.isnan().all())


# ------------------------------------------------------------------------------------------------------------------- box stage
BOX_FORMS = [(False, 0), (True, 1), (True, 0)]                                             # (vertical, axis)


def run_boxes(dev, rows, counts, max_det, H, W, axis, vertical):
    Lh = _lib.lib()
    L = rows.shape[0]
    d_rows, d_counts = rows.to(dev).contiguous(), counts.to(dev)
    srt = _nanbuf(dev, L, max_det, 4)
    n = torch.full((max(L, 1),), R.SENTINEL, dtype=torch.int32, device=dev)
    b5 = torch.full((max(L * max_det, 1), 5), R.SENTINEL, dtype=torch.int32, device=dev)
    total = torch.full((1,), R.SENTINEL, dtype=torch.int32, device=dev)
    rc = Lh.effocr_parse_char_boxes(_lib.ptr(d_rows), _lib.ptr(d_counts), L, max_det, H, W, axis, 1 if vertical else 0, _lib.ptr(srt), _lib.ptr(n), _lib.ptr(b5),
                                    _lib.ptr(total), _lib.current_stream(dev))
    _lib.check(rc, "effocr_parse_char_boxes", Lh)
    torch.cuda.synchronize(dev)
    assert torch.equal(d_rows.cpu().view(torch.int32), rows.view(torch.int32))
    return srt.cpu(), n.cpu()[:L], b5.cpu()[:L * max_det], int(total.item())


@pytest.mark.parametrize("L", R.BOX_LINES)
@pytest.mark.parametrize("max_det", R.BOX_MAX_DETS)
def test_box_stage(dev, max_det, L):
    """Exact: the sorted boxes of every line, the character counts, the compact crop slices and the total, against the plain-Python
    restatement of the driver; crop rows from the total on are untouched."""
    vertical, axis = BOX_FORMS[(max_det + L) % 3]
    rows, counts = R.boxes_data(max_det, L)
    want = R.boxes_ref(rows, counts, max_det, R.BOX_H, R.BOX_W, axis, vertical)
    R.check_boxes(run_boxes(dev, rows, counts, max_det, R.BOX_H, R.BOX_W, axis, vertical), want, f"box stage max_det {max_det} L {L}")
    print(f"box stage max_det={max_det} L={L} vertical={vertical} axis={axis}: {want[3]} crops, exact")


@pytest.mark.parametrize("vertical,axis", BOX_FORMS)
def test_box_stage_forms(dev, vertical, axis):
    rows, counts = R.boxes_data(65, 40)
    want = R.boxes_ref(rows, counts, 65, R.BOX_H, R.BOX_W, axis, vertical)
    R.check_boxes(run_boxes(dev, rows, counts, 65, R.BOX_H, R.BOX_W, axis, vertical), want, f"box stage vertical {vertical} axis {axis}")


@pytest.mark.parametrize("max_det", [5, 64, 65, 1000])
def test_box_stage_nan_keys(dev, max_det):
    """NaN sort keys rank as in torch.sort: behind every number and behind the rows that are no characters (key +inf).  Below a power of
    two (or below the 64-entry floor) the bitonic network's padding entries must rank behind them as well: every sorted row is a row
    of its own line."""
    rows, counts = R.boxes_data(max_det, 40, nan_keys=True)
    want = R.boxes_torch(rows, counts, max_det, R.BOX_H, R.BOX_W, 1, False)
    R.check_boxes(run_boxes(dev, rows, counts, max_det, R.BOX_H, R.BOX_W, 1, False), want, f"box stage NaN keys max_det {max_det}")
    print(f"box stage NaN keys max_det={max_det}: {int(rows[..., 1].isnan().sum())} NaN keys, {want[3]} crops, exact")


def test_box_stage_refusals(dev):
    Lh = _lib.lib()
    t = torch.zeros(64, device=dev)
    p = _lib.ptr(t)
    assert Lh.effocr_parse_char_boxes(p, p, 1, 4097, 32, 32, 0, 0, p, p, p, p, None) == -2 and b"max_det must be in 1..4096" in Lh.effocr_last_error()
    assert Lh.effocr_parse_char_boxes(p, p, 1, 2, 32, 32, 2, 0, p, p, p, p, None) == -1 and b"axis" in Lh.effocr_last_error()
    torch.cuda.synchronize(dev)
    assert not t.any()
