"""Float64 restatements, test data, derived error bounds and mutants of the localizer tail: the two Detect decodes (csrc/yolov8.hip
yolov8_decode_kernel, csrc/yolo.hip yolo_decode_kernel), the YOLOv8 stem (csrc/yolov8.hip stem3x3s2_g16_kernel) and the box stage
(csrc/boxes.hip boxes_sort_kernel + boxes_compact_kernel), on caller-made tensors in the kernels' own layouts.
tests/test_gpu_localizer_ops.py runs the kernels against them, one launch per case, through effocr_yolov8_op_decode / _op_stem
(libeffocr_yolov8.so), effocr_convops_yolo_decode (the test library) and effocr_parse_char_boxes (the product library);
tests/test_localizer_ops_host.py proves on the CPU that every bound admits a float32 evaluation and rejects every mutant.

Every reference returns the WHOLE buffer the operator writes into, NaN (a sentinel for the integer outputs) wherever the operator owns
nothing: the comparison (`check_owned`) wants every owned element written and inside its bound and every other element untouched.
Comparison functions and the rounding constants are tests/convops_ref.py's.

Error model (convops_ref's), u = 2^-24, gamma_n = n u / (1 - n u):
  * an fp32 sum of n terms errs by at most gamma_n sum |terms| (the issue's 16-term sums: gamma_16); every further fp32 add or multiply
    adds u |its result|; expf and a division 1 ulp = 2 u relative (the constant tests/swin_ops_ref.py uses for a division, v_rcp and
    v_exp; HIP's math documentation states 1 ulp for expf); a result below the smallest normal (flushed, or kept as a subnormal) errs by
    at most TINYN = 2^-126 absolute.
  * sigmoid 1 / (1 + expf(-v)): e = expf(-v) is off by 2 u e (the negation is exact); 1 + e by e / (1 + e) 2 u + u <= 3 u relative; the
    division adds 2 u: SIG_RHO = 5 u relative (6 u with the second-order terms) plus TINYN where expf or the quotient leaves the normal
    range (an overflowed expf gives 1 / inf = 0 for a true value below 2^-126).
  * YOLOv8 decode, one side: a_k = v_k - max v is off by u |a_k|, so e_k = expf(a_k) by the relative rho_k = expm1(u |a_k|) (1 + 2 u)
    + 2 u, plus TINYN absolute.  den = sum e_k, num = sum k e_k (one more rounding per product), both over 16 terms: every term of den
    carries beta_k = rho_k + gamma_16 (1 + rho_k), of num alpha_k = rho_k + gamma_17 (1 + rho_k).  With p = softmax and d = sum k p_k:
        |num / den - d| <= (sum k p_k alpha_k + d sum p_k beta_k + 136 TINYN) / (1 - sum p_k beta_k - 16 TINYN)     (den >= 1: e_max = 1)
    and the division adds 2 u |d|.  x1 = ax - d_l, x2 = ax + d_r add u |x1|, u |x2| (ax = px + 0.5 is exact); cx = (x1 + x2) 0.5 stride:
    (e_x1 + e_x2 + u |x1 + x2|) 0.5 stride + u |cx|; w = (x2 - x1) stride: (e_x1 + e_x2 + u |x2 - x1|) stride + u |w|; likewise cy, h.
    The objectness column is the constant 1: no error allowed.
  * YOLOv5 decode with s = sigmoid(v) known to within e_s: xy = (2 s + g) stride (2 s exact): stride (2 e_s + u |2 s + g|) + u |xy|;
    wh = (2 s)^2 a: a (8 s e_s + 4 e_s^2) + 2 u (1 + u) |wh| (the square and the product with the anchor); every other column e_s.
  * stem: tests/convops_ref.py's conv_bound with K = 27 and the SiLU epilogue (silu_fast's constants are derived there).
  * box stage: integers and copies — exact."""
import dataclasses
import math

import torch
import torch.nn.functional as F

from tests import convops_ref as CR
from tests import yolov8_ref
from tests.convops_ref import Mismatch, U, check_bound

NAN = float("nan")
TINY32 = CR.TINY[torch.float32]
TINYN = 2.0 ** -126
SIG_RHO = 6 * U


def gamma(n):
    return n * U / (1 - n * U)


def _gen(*key):
    return torch.Generator().manual_seed(4241 + sum((i + 3) * int(k) for i, k in enumerate(key)))


def check_owned(got, ref, bound, own, what="", nonfinite=False):
    """`got`, `ref`, `bound`, `own`: the whole buffer.  Outside `own` every element is still NaN; inside it every element is written and
    within `bound` of `ref` — or, with `nonfinite`, where `ref` is not finite, the same non-finite value.  Returns max error / bound."""
    assert got.shape == ref.shape == bound.shape == own.shape, f"{what}: shapes {tuple(got.shape)} {tuple(ref.shape)}"
    out = ~own
    if not bool(got[out].isnan().all()):
        i = tuple((out & ~got.isnan()).nonzero()[0].tolist())
        raise Mismatch(f"{what}: {int((out & ~got.isnan()).sum())} elements written outside the operator's rows / slice; first at {i}: {got[i].item()!r}")
    fin = own & torch.isfinite(ref)
    if not nonfinite and not bool(fin[own].all()):
        raise AssertionError(f"{what}: the reference is not finite")
    if nonfinite:
        nf = own & ~torch.isfinite(ref)
        want = ref.to(got.dtype)
        same = (got == want) | (got.isnan() & want.isnan())
        if not bool(same[nf].all()):
            i = tuple((nf & ~same).nonzero()[0].tolist())
            raise Mismatch(f"{what}: {int((nf & ~same).sum())} of {int(nf.sum())} non-finite outputs differ from the reference; first at {i}: "
                           f"got {got[i].item()!r}, want {want[i].item()!r}")
    return check_bound(got[fin], ref[fin], bound[fin], what)


def column_ratios(got, ref, bound, own, groups):
    """Largest error / bound over the owned, finite elements of each group of last-axis columns: {name: ratio}."""
    ok = own & torch.isfinite(ref)
    r = torch.where(ok, (got.double() - ref).abs() / bound, torch.zeros((), dtype=torch.float64))
    return {name: r[..., cols].max().item() for name, cols in groups.items()}


ROW_GROUPS = {"box": slice(0, 4), "scores": slice(4, None)}


# ------------------------------------------------------------------------------------------------------------------- YOLOv8 decode
@dataclasses.dataclass(frozen=True)
class V8Case:
    B: int
    ny: int
    nx: int
    nc: int
    box_ld: int
    cls_ld: int
    before: int
    after: int
    why: str = ""

    @property
    def name(self):
        return f"B{self.B}_{self.ny}x{self.nx}_nc{self.nc}_ld{self.box_ld}_{self.cls_ld}_r{self.before}_{self.after}"

    @property
    def A(self):
        return self.ny * self.nx

    @property
    def total(self):
        return self.before + self.A + self.after

    @property
    def no(self):
        return self.nc + 5

    @property
    def stride(self):
        return (8.0, 16.0, 32.0)[(self.ny + self.nc) % 3]


V8_CASES = [
    V8Case(1, 1, 1, 1, 64, 4, 0, 0, "single anchor point"),
    V8Case(2, 3, 5, 2, 64, 4, 4, 3, "row offsets before and after the level"),
    V8Case(3, 5, 3, 5, 96, 8, 0, 7, "box_ld wider than 64, cls_ld wider than nc, second class-loop iteration"),
    V8Case(1, 9, 7, 9, 64, 12, 0, 0, "63 points: the tail quad sits inside a block"),
    V8Case(1, 13, 5, 3, 64, 4, 2, 0, "65 points: the second block holds one live quad"),
    V8Case(2, 8, 8, 80, 64, 80, 0, 0, "exactly two full blocks, twenty class iterations"),
]
V8_KINDS = ["normal", "peaked", "shift+100", "shift-100", "equal"]
V8_NONFINITE = ["nan", "inf"]


def v8_data(c, kind):
    """box [B * A][box_ld], cls [B * A][cls_ld] fp32; the columns no kernel may read (64 .. box_ld, nc .. cls_ld) hold NaN."""
    g = _gen(1, c.B, c.ny, c.nx, c.nc)
    P = c.B * c.A
    t = torch.randn(P, 4, 16, generator=g) * 2.0
    if kind == "peaked":                                    # one bin at +30, the rest at -30: bins 0 and 15 are the peak somewhere
        peak = (torch.arange(P)[:, None] * 5 + torch.arange(4)[None, :] * 15) % 16
        assert P < 4 or {0, 15} <= set(peak.reshape(-1).tolist())
        t = torch.full((P, 4, 16), -30.0)
        t.scatter_(2, peak[..., None], 30.0)
    elif kind == "shift+100":
        t = t + 100.0
    elif kind == "shift-100":
        t = t - 100.0
    elif kind == "equal":
        t = torch.full((P, 4, 16), 1.25)
    elif kind in ("nan", "inf"):                            # one side of one point: the left side of the middle point, bin 6
        t[P // 2, 0, 6] = NAN if kind == "nan" else float("inf")
    box = torch.full((P, c.box_ld), NAN)
    box[:, :64] = t.reshape(P, 64)
    cls = torch.full((P, c.cls_ld), NAN)
    cls[:, :c.nc] = torch.randn(P, c.nc, generator=g) * 3.0
    return dict(box=box, cls=cls)


def _v8_place(c, rows, dtype=torch.float64):
    """rows [B, A, no] -> the prediction tensor [B, total, no], NaN outside the level's rows."""
    out = torch.full((c.B, c.total, c.no), NAN, dtype=dtype)
    out[:, c.before:c.before + c.A] = rows
    return out


def v8_own(c):
    own = torch.zeros(c.B, c.total, c.no, dtype=torch.bool)
    own[:, c.before:c.before + c.A] = True
    return own


def _v8_nchw(c, d, dtype):
    box = d["box"][:, :64].to(dtype).reshape(c.B, c.ny, c.nx, 64).permute(0, 3, 1, 2).contiguous()
    cls = d["cls"][:, :c.nc].to(dtype).reshape(c.B, c.ny, c.nx, c.nc).permute(0, 3, 1, 2).contiguous()
    return box, cls


def v8_ref(c, d):
    """tests/yolov8_ref.py's decode (Detect inference + DFL + dist2bbox) in float64, placed at the level's rows."""
    return _v8_place(c, yolov8_ref.decode(*_v8_nchw(c, d, torch.float64), c.stride))


def v8_f32(c, d):
    return _v8_place(c, yolov8_ref.decode(*_v8_nchw(c, d, torch.float32), c.stride), torch.float32)


def v8_bound(c, d):
    t = d["box"][:, :64].double().reshape(c.B, c.A, 4, 16)
    a = t - t.max(3, keepdim=True).values
    p = a.softmax(3)
    k = torch.arange(16, dtype=torch.float64)
    dist = (p * k).sum(3)                                                         # [B, A, 4]
    rho = torch.expm1(U * a.abs()) * (1 + 2 * U) + 2 * U
    beta, alpha = rho + gamma(16) * (1 + rho), rho + gamma(17) * (1 + rho)
    sb = (p * beta).sum(3) + 16 * TINYN
    ed = ((k * p * alpha).sum(3) + dist * sb + 136 * TINYN) / (1 - sb)
    ed = ed + 2 * U * (dist + ed)
    ys, xs = torch.meshgrid(torch.arange(c.ny, dtype=torch.float64) + 0.5, torch.arange(c.nx, dtype=torch.float64) + 0.5, indexing="ij")
    ax, ay = xs.reshape(-1), ys.reshape(-1)
    x1, y1, x2, y2 = ax - dist[..., 0], ay - dist[..., 1], ax + dist[..., 2], ay + dist[..., 3]
    e1 = [ed[..., 0] + U * x1.abs(), ed[..., 1] + U * y1.abs(), ed[..., 2] + U * x2.abs(), ed[..., 3] + U * y2.abs()]
    s = c.stride
    ref = v8_ref(c, d)[:, c.before:c.before + c.A]
    e = torch.zeros(c.B, c.A, c.no, dtype=torch.float64)
    e[..., 0] = (e1[0] + e1[2] + U * (x1 + x2).abs()) * 0.5 * s + U * ref[..., 0].abs()
    e[..., 1] = (e1[1] + e1[3] + U * (y1 + y2).abs()) * 0.5 * s + U * ref[..., 1].abs()
    e[..., 2] = (e1[0] + e1[2] + U * (x2 - x1).abs()) * s + U * ref[..., 2].abs()
    e[..., 3] = (e1[1] + e1[3] + U * (y2 - y1).abs()) * s + U * ref[..., 3].abs()
    e[..., 5:] = SIG_RHO * ref[..., 5:] + TINYN
    return _v8_place(c, e + TINY32)


V8_MUTANTS = ["no_max_subtraction", "bins_weighted_k_plus_1", "bins_reversed", "left_right_swapped", "top_bottom_swapped", "anchor_offset_0",
              "px_py_swapped", "stride_on_centre_only", "w_is_x2_plus_x1", "classes_from_4_dropped", "class_from_channel_c_mod_4", "box_ld_taken_as_64",
              "cls_ld_taken_as_nc", "row0_ignored", "batch_stride_ny_nx", "objectness_not_written"]


def v8_variant(c, d, fault=None):
    """The decode written out step by step with one switchable fault; fault=None restates v8_ref (the host test holds the two together).
    float64, but for `no_max_subtraction`, whose damage is fp32's overflow and underflow: that one runs in float32."""
    dt = torch.float32 if fault == "no_max_subtraction" else torch.float64
    P = c.B * c.A
    box = d["box"].reshape(-1)[:P * 64].reshape(P, 64) if fault == "box_ld_taken_as_64" else d["box"][:, :64]
    cls = d["cls"].reshape(-1)[:P * c.nc].reshape(P, c.nc) if fault == "cls_ld_taken_as_nc" else d["cls"][:, :c.nc]
    t = box.to(dt).reshape(c.B, c.A, 4, 16)
    e = torch.exp(t if fault == "no_max_subtraction" else t - t.max(3, keepdim=True).values)
    k = torch.arange(16, dtype=dt)
    wk = k + 1 if fault == "bins_weighted_k_plus_1" else (15 - k if fault == "bins_reversed" else k)
    dist = (e * wk).sum(3) / e.sum(3)
    dl, dtop, dr, db = dist.unbind(2)
    if fault == "left_right_swapped":
        dl, dr = dr, dl
    if fault == "top_bottom_swapped":
        dtop, db = db, dtop
    pix = torch.arange(c.A)
    px, py = (pix % c.nx).to(dt), (pix // c.nx).to(dt)
    if fault == "px_py_swapped":
        px, py = py, px
    off = 0.0 if fault == "anchor_offset_0" else 0.5
    ax, ay = px + off, py + off
    x1, y1, x2, y2 = ax - dl, ay - dtop, ax + dr, ay + db
    s = c.stride
    sw = 1.0 if fault == "stride_on_centre_only" else s
    w = (x2 + x1) if fault == "w_is_x2_plus_x1" else (x2 - x1)
    rows = torch.full((c.B, c.A, c.no), NAN, dtype=dt)
    rows[..., 0], rows[..., 1], rows[..., 2], rows[..., 3] = (x1 + x2) * 0.5 * s, (y1 + y2) * 0.5 * s, w * sw, (y2 - y1) * sw
    if fault != "objectness_not_written":
        rows[..., 4] = 1.0
    sc = torch.sigmoid(cls.to(dt)).reshape(c.B, c.A, c.nc)
    if fault == "class_from_channel_c_mod_4":
        sc = sc[..., torch.arange(c.nc) % 4]
    nlive = min(c.nc, 4) if fault == "classes_from_4_dropped" else c.nc
    rows[..., 5:5 + nlive] = sc[..., :nlive]
    flat = torch.full((c.B * c.total, c.no), NAN, dtype=dt)
    r0 = 0 if fault == "row0_ignored" else c.before
    bs = c.A if fault == "batch_stride_ny_nx" else c.total
    for b in range(c.B):
        flat[b * bs + r0: b * bs + r0 + c.A] = rows[b]
    return flat.reshape(c.B, c.total, c.no).double()


def v8_applies(c, fault):
    """Whether a fault changes anything at this geometry (the data decides the rest)."""
    return {"px_py_swapped": c.A > 1, "classes_from_4_dropped": c.nc > 4, "class_from_channel_c_mod_4": c.nc > 4, "box_ld_taken_as_64": c.box_ld != 64,
            "cls_ld_taken_as_nc": c.cls_ld != c.nc and c.B * c.A > 1, "row0_ignored": c.before > 0,
            "batch_stride_ny_nx": c.B > 1 and c.total != c.A}.get(fault, True)


# ------------------------------------------------------------------------------------------------------------------- YOLOv5 decode
ANCHORS_PX = ((10.0, 13.0), (16.0, 30.0), (33.0, 23.0))      # three distinct non-square anchors, input pixels


@dataclasses.dataclass(frozen=True)
class V5Case:
    B: int
    ny: int
    nx: int
    no: int
    padded: bool
    before: int
    after: int
    kind: str

    @property
    def name(self):
        return f"B{self.B}_{self.ny}x{self.nx}_no{self.no}_{'pad' if self.padded else 'dense'}_r{self.before}_{self.after}_{self.kind}"

    @property
    def raw_ld(self):
        return (3 * self.no + 31) // 32 * 32 if self.padded else 3 * self.no

    @property
    def A(self):
        return 3 * self.ny * self.nx

    @property
    def total(self):
        return self.before + self.A + self.after

    @property
    def stride(self):
        return (8.0, 16.0, 32.0)[self.no % 3]


V5_CASES = [V5Case(2, 3, 5, 6, False, 0, 0, "normal"), V5Case(2, 5, 3, 7, True, 6, 2, "normal"), V5Case(1, 4, 7, 10, True, 0, 5, "normal"),
            V5Case(3, 2, 3, 10, False, 1, 0, "normal"), V5Case(1, 3, 2, 6, True, 2, 1, "saturated"), V5Case(2, 5, 3, 7, False, 0, 3, "saturated")]


def v5_data(c):
    """raw [B * ny * nx][raw_ld] fp32, channel an * no + o; the columns past 3 no hold NaN."""
    g = _gen(2, c.B, c.ny, c.nx, c.no, c.padded)
    P = c.B * c.ny * c.nx
    v = torch.randn(P, 3 * c.no, generator=g) * 2.0
    if c.kind == "saturated":
        v = torch.tensor([90.0, -90.0, 200.0, -200.0])[torch.randint(0, 4, (P, 3 * c.no), generator=g)]
        v[::3] = torch.randn(v[::3].shape, generator=g)      # (every third point stays ordinary)
    raw = torch.full((P, c.raw_ld), NAN)
    raw[:, :3 * c.no] = v
    return dict(raw=raw)


def v5_own(c):
    own = torch.zeros(c.B, c.total, c.no, dtype=torch.bool)
    own[:, c.before:c.before + c.A] = True
    return own


def _v5_detect(c, d, dtype):
    """oracle/yolo_ref.py's Detect, inference branch, for one level: (bs, na no, ny, nx) -> (bs, na, ny, nx, no) -> sigmoid ->
    xy = (y 2 + grid) stride, grid = index - 0.5; wh = (y 2)^2 anchor (pixels) -> (bs, na ny nx, no)."""
    r = d["raw"][:, :3 * c.no].to(dtype).reshape(c.B, c.ny, c.nx, 3 * c.no).permute(0, 3, 1, 2)
    y = r.reshape(c.B, 3, c.no, c.ny, c.nx).permute(0, 1, 3, 4, 2).contiguous().sigmoid()
    yv, xv = torch.meshgrid(torch.arange(c.ny, dtype=dtype), torch.arange(c.nx, dtype=dtype), indexing="ij")
    grid = torch.stack((xv, yv), 2).expand(1, 3, c.ny, c.nx, 2) - 0.5
    anchor_grid = torch.tensor(ANCHORS_PX, dtype=dtype).view(1, 3, 1, 1, 2).expand(1, 3, c.ny, c.nx, 2)
    xy = (y[..., 0:2] * 2 + grid) * c.stride
    wh = (y[..., 2:4] * 2) ** 2 * anchor_grid
    return torch.cat((xy, wh, y[..., 4:]), -1), y, grid, anchor_grid


def _v5_place(c, rows, dtype=torch.float64):
    out = torch.full((c.B, c.total, c.no), NAN, dtype=dtype)
    out[:, c.before:c.before + c.A] = rows.reshape(c.B, c.A, c.no)
    return out


def v5_ref(c, d):
    return _v5_place(c, _v5_detect(c, d, torch.float64)[0])


def v5_f32(c, d):
    return _v5_place(c, _v5_detect(c, d, torch.float32)[0], torch.float32)


def v5_bound(c, d):
    z, s, grid, anchor = _v5_detect(c, d, torch.float64)
    es = SIG_RHO * s + TINYN
    e = es.clone()
    e[..., 0:2] = c.stride * (2 * es[..., 0:2] + U * (2 * s[..., 0:2] + grid).abs()) + U * z[..., 0:2].abs()
    e[..., 2:4] = anchor * (8 * s[..., 2:4] * es[..., 2:4] + 4 * es[..., 2:4] ** 2) + 2 * U * (1 + U) * z[..., 2:4].abs()
    return _v5_place(c, e + TINY32)


V5_MUTANTS = ["grid_without_half", "x_y_swapped", "anchor_w_h_swapped", "anchor_of_wrong_index", "two_sigma_not_squared", "rows_y_x_anchor",
              "channel_o_na_plus_an", "raw_ld_taken_as_3_no", "row0_ignored", "batch_stride_without_total"]


def v5_variant(c, d, fault=None):
    """Detect element by element, with one switchable fault; fault=None restates v5_ref."""
    P = c.B * c.ny * c.nx
    raw = d["raw"].reshape(-1)[:P * 3 * c.no].reshape(P, 3 * c.no) if fault == "raw_ld_taken_as_3_no" else d["raw"][:, :3 * c.no]
    raw = raw.double().reshape(c.B, c.ny, c.nx, 3 * c.no)
    rows = torch.full((c.B, 3, c.ny, c.nx, c.no), NAN, dtype=torch.float64)
    gy, gx = torch.meshgrid(torch.arange(c.ny, dtype=torch.float64), torch.arange(c.nx, dtype=torch.float64), indexing="ij")
    half = 0.0 if fault == "grid_without_half" else 0.5
    if fault == "x_y_swapped":
        gx, gy = gy, gx
    for an in range(3):
        aw, ah = ANCHORS_PX[(an + 1) % 3 if fault == "anchor_of_wrong_index" else an]
        if fault == "anchor_w_h_swapped":
            aw, ah = ah, aw
        for o in range(c.no):
            s = torch.sigmoid(raw[..., o * 3 + an if fault == "channel_o_na_plus_an" else an * c.no + o])
            if o == 0:
                s = (s * 2 + (gx - half)) * c.stride
            elif o == 1:
                s = (s * 2 + (gy - half)) * c.stride
            elif o in (2, 3):
                s = (s * 2 if fault == "two_sigma_not_squared" else (s * 2) ** 2) * (aw if o == 2 else ah)
            rows[:, an, :, :, o] = s
    if fault == "rows_y_x_anchor":
        rows = rows.permute(0, 2, 3, 1, 4)
    rows = rows.reshape(c.B, c.A, c.no)
    flat = torch.full((c.B * c.total, c.no), NAN, dtype=torch.float64)
    r0 = 0 if fault == "row0_ignored" else c.before
    bs = c.A if fault == "batch_stride_without_total" else c.total
    for b in range(c.B):
        flat[b * bs + r0: b * bs + r0 + c.A] = rows[b]
    return flat.reshape(c.B, c.total, c.no)


def v5_applies(c, fault):
    return {"raw_ld_taken_as_3_no": c.padded and c.raw_ld != 3 * c.no, "row0_ignored": c.before > 0,
            "batch_stride_without_total": c.B > 1 and c.total != c.A}.get(fault, True)


# ------------------------------------------------------------------------------------------------------------------- YOLOv8 stem
@dataclasses.dataclass(frozen=True)
class StemCase:
    B: int
    H: int
    W: int
    cout: int
    cout_st: int
    wt_ld: int
    out_ld: int
    out_off: int
    why: str = ""

    @property
    def name(self):
        return f"B{self.B}_{self.H}x{self.W}_c{self.cout}_{self.cout_st}_wt{self.wt_ld}_ld{self.out_ld}_{self.out_off}"

    @property
    def conv(self):
        return CR.ConvCase("v8stem_" + self.name, self.B, self.H, self.W, 3, self.cout, 3, 2, 1, "silu")

    @property
    def OH(self):
        return (self.H - 1) // 2 + 1

    @property
    def OW(self):
        return (self.W - 1) // 2 + 1

    @property
    def M(self):
        return self.B * self.OH * self.OW


STEM_CASES = [
    StemCase(2, 5, 7, 16, 32, 32, 32, 0, "odd H and W, one padding group"),
    StemCase(1, 8, 8, 48, 64, 64, 96, 32, "a slice inside a wider buffer"),
    StemCase(3, 2, 24, 80, 96, 128, 96, 0, "OH = 1, wt_ld wider than cout_st"),
    StemCase(1, 33, 40, 64, 64, 64, 64, 0, "more than one block (four channel groups)"),
    StemCase(2, 33, 71, 16, 16, 16, 16, 0, "306 pixel quads: two blocks along the pixels, odd W"),
]
# (case, argument overrides, message): what the launcher refuses
STEM_REFUSED = [(dict(W=10), "output width must be a multiple of 4"), (dict(cout=40, cout_st=48, wt_ld=64, out_ld=64), "channel counts of 16"),
                (dict(out_off=16), "the slice inside its buffer")]


def stem_data(c, nonfinite=False):
    """convops_ref's conv_data (the last row of image b bright, the first row of image b + 1 dark).  `nonfinite`: one NaN pixel and one
    inf pixel, in different images where there are two, far enough apart that no window holds both."""
    x, w, bias, _ = CR.conv_data(c.conv, "real")
    if nonfinite:
        x = x.clone()
        x[0, 1, 0, 0] = NAN
        x[-1, 2, c.H - 1, c.W - 1] = float("inf")
    return dict(x=x, w=w, bias=bias)


def pack_stem(c, d):
    """wt [27][wt_ld], row (ky 3 + kx) 3 + ci; the columns from cout on, which the kernel never reads, hold NaN.  bias [cout_st], 0 from cout on."""
    wt = torch.full((27, c.wt_ld), NAN)
    wt[:, :c.cout] = CR.pack_w(d["w"]).t()
    b = torch.zeros(c.cout_st)
    b[:c.cout] = d["bias"]
    return wt, b


def _stem_place(c, y, dtype=torch.float64):
    """y [B, cout, OH, OW] -> the output buffer [M, out_ld]: the slice's live channels, exact zeros up to cout_st, NaN elsewhere."""
    out = torch.full((c.M, c.out_ld), NAN, dtype=dtype)
    out[:, c.out_off:c.out_off + c.cout_st] = 0.0
    out[:, c.out_off:c.out_off + c.cout] = CR.to_nhwc(y).reshape(c.M, c.cout).to(dtype)
    return out


def stem_own(c):
    own = torch.zeros(c.M, c.out_ld, dtype=torch.bool)
    own[:, c.out_off:c.out_off + c.cout_st] = True
    return own


def stem_ref(c, d):
    return _stem_place(c, CR.conv_reference(c.conv, d["x"], d["w"], d["bias"], None)[0])


def stem_bound(c, d):
    """conv_bound (K = 27, SiLU) on the live channels; 0 on the padding groups, which must be exactly 0."""
    out = torch.zeros(c.M, c.out_ld, dtype=torch.float64)
    out[:, c.out_off:c.out_off + c.cout] = CR.to_nhwc(CR.conv_bound(c.conv, d["x"], d["w"], d["bias"], None)).reshape(c.M, c.cout)
    return out


def stem_f32(c, d):
    return _stem_place(c, F.silu(F.conv2d(d["x"], d["w"], d["bias"], stride=2, padding=1)), torch.float32)


def check_stem(c, got, ref, bound, what="", nonfinite=False):
    """check_owned on the live channels; the padding groups exactly +0; everything outside the slice untouched."""
    live = torch.zeros(c.M, c.out_ld, dtype=torch.bool)
    live[:, c.out_off:c.out_off + c.cout] = True
    pad = stem_own(c) & ~live
    if not bool((got[pad] == 0).all()) or bool(torch.signbit(got[pad]).any()):
        raise Mismatch(f"{what}: the padding groups {c.cout} .. {c.cout_st} are not exactly +0")
    g = got.clone()
    g[pad] = NAN
    return check_owned(g, ref, bound, live, what, nonfinite)


STEM_MUTANTS = ["pad_0", "window_crosses_planes", "taps_kx_ky", "stride_1", "padding_group_not_zero", "slice_offset_ignored", "relu_for_silu"]


def stem_variant(c, d, fault=None):
    x, w, b = d["x"].double(), d["w"].double(), d["bias"].double()
    if fault == "taps_kx_ky":
        w = w.transpose(2, 3)
    if fault == "window_crosses_planes":                     # the rows above and below a plane are its neighbours in memory, not zeros
        flat = F.pad(x.reshape(-1, c.W), (0, 0, 1, 1))
        top = flat[torch.arange(c.B * 3) * c.H].reshape(c.B, 3, 1, c.W)
        bot = flat[torch.arange(c.B * 3) * c.H + c.H + 1].reshape(c.B, 3, 1, c.W)
        xp = F.pad(torch.cat((top, x, bot), 2), (1, 1, 0, 0))
    elif fault == "pad_0":                                   # every window starts one pixel late
        xp = F.pad(x, (0, 3, 0, 3))
    else:
        xp = F.pad(x, (1, 2, 1, 2))
    if fault == "stride_1":
        xp = F.pad(xp, (0, c.OW, 0, c.OH))
    y = F.conv2d(xp, w, b, stride=1 if fault == "stride_1" else 2)[:, :, :c.OH, :c.OW]
    y = F.relu(y) if fault == "relu_for_silu" else y * torch.sigmoid(y)
    if fault == "slice_offset_ignored":
        c = dataclasses.replace(c, out_off=0)
    out = _stem_place(c, y)
    if fault == "padding_group_not_zero":                    # the taps run on the padding group's stale weights: a small non-zero value
        out[:, c.out_off + c.cout:c.out_off + c.cout_st] = 2.0 ** -20
    return out


def stem_applies(c, fault):
    return {"padding_group_not_zero": c.cout_st > c.cout, "slice_offset_ignored": c.out_off > 0}.get(fault, True)


# ------------------------------------------------------------------------------------------------------------------- box stage
BOX_MAX_DETS = [1, 5, 64, 65, 1000, 4096]
BOX_LINES = [0, 1, 40]
BOX_H, BOX_W = 320, 960                                       # size / 640 = 0.5 and 1.5: odd rounded bounds land on .5 at the second rounding
SENTINEL = -777


def boxes_data(max_det, L, nan_keys=False):
    """rows [L, max_det, 6] = (x0, y0, x1, y1, conf, label) and counts [L].  Lines cycle through: heavy key ties; x.5 coordinates (half-way
    at torch.round); odd integers (half-way at the second rounding, both sizes); coordinates whose scaled bounds are negative or beyond the
    line; labels -0.0, 1 and 2; counts that are negative, zero, max_det and above max_det.  Every coordinate is finite; `nan_keys` puts
    NaN into column 1 of some characters — the sort key of axis 1, which a horizontal line's slices never read."""
    g = _gen(3, max_det, L)
    rows = torch.zeros(L, max_det, 6)
    rows[..., 0] = torch.rand(L, max_det, generator=g) * 700 - 30
    rows[..., 1] = torch.rand(L, max_det, generator=g) * 700 - 30
    rows[..., 2] = rows[..., 0] + torch.rand(L, max_det, generator=g) * 80
    rows[..., 3] = rows[..., 1] + torch.rand(L, max_det, generator=g) * 80
    rows[..., 4] = torch.rand(L, max_det, generator=g)
    rows[..., 5] = torch.tensor([0.0, 0.0, -0.0, 1.0, 2.0, 0.0])[torch.randint(0, 6, (L, max_det), generator=g)]
    counts = torch.randint(0, max_det + 1, (L,), generator=g).to(torch.int32)
    for l in range(L):
        m = l % 8
        if m == 0:
            rows[l, :, :2] = torch.randint(0, 4, (max_det, 2), generator=g).float() * 3      # four distinct keys: stability
        elif m == 1:
            rows[l, :, :4] = torch.round(rows[l, :, :4]) + 0.5
        elif m == 2:
            rows[l, :, :4] = torch.round(rows[l, :, :4] / 2) * 2 + 1
        elif m == 3:
            rows[l, :, 5] = 1.0                                                              # a line without characters
        elif m == 4:
            rows[l, :, 5] = -0.0                                                             # every row a character, all labelled -0.0
        counts[l] = (max_det, max_det, max_det + 7, max_det, max_det, -3, 0, int(counts[l]))[m]
    if nan_keys:
        rows[..., 1] = torch.where(torch.rand(L, max_det, generator=g) < 0.3, torch.full((), NAN), rows[..., 1])
    return rows, counts


def _round_half_away(v):
    return math.floor(abs(v) + 0.5) * (1 if v >= 0 else -1)


def boxes_ref(rows, counts, max_det, H, W, axis, vertical, fault=None):
    """The driver's box stage in plain Python (infer_effocr_onnx_multi.py, the lines csrc/boxes.hip cites), line by line:
    characters = the first counts[l] rows whose label equals 0; sorted(key = the reading axis) (stable); per character torch.round on the
    fp32 box, Python round() of the scaled bound, numpy's slice resolution (slice.indices) along the reading direction and the whole line
    across it.  -> sorted [L, max_det, 4] (characters first, every other row behind them in row order), n_chars [L], the crop buffer
    [L max_det, 5] (rows from the total on untouched: SENTINEL), total.  `fault`: one of BOX_MUTANTS."""
    L = rows.shape[0]
    fl = rows.reshape(-1, 6).tolist()
    r1 = torch.round(rows.reshape(-1, 6)[:, :4]).tolist()    # torch.round on the fp32 boxes: half to even
    size = H if vertical else W
    lo_i, hi_i = (1, 3) if vertical else (0, 2)
    sorted_rows = torch.full((L, max_det, 4), NAN)
    crops, n_chars = [], []
    for l in range(L):
        cnt = max(int(counts[l]), 0)
        if fault != "count_not_clamped":
            cnt = min(cnt, max_det)
        base = l * max_det                                   # (an unclamped count runs on into the next line's rows)
        line = [fl[base + j] if base + j < len(fl) else [0.0] * 6 for j in range(cnt)]
        if fault == "minus_zero_label_not_a_character":
            chars = [j for j in range(cnt) if line[j][5] == 0 and math.copysign(1.0, line[j][5]) > 0]
        else:
            chars = [j for j in range(cnt) if line[j][5] == 0]
        order = sorted(chars, key=(lambda j: (line[j][axis], -j)) if fault == "unstable_sort" else (lambda j: line[j][axis]))
        inside = [j for j in order if j < max_det]
        perm = (inside + sorted(set(range(max_det)) - set(inside)))[:max_det]
        sorted_rows[l] = rows[l, perm, :4]
        n_chars.append(len(chars))
        mine = []
        for j in order:
            if fault == "first_round_half_away":
                box = [_round_half_away(v) for v in line[j][:4]]
            else:
                box = r1[base + j] if base + j < len(r1) else [0.0] * 4
            rnd = _round_half_away if fault == "second_round_half_away" else round
            lo, hi = int(rnd(box[lo_i] * size / 640)), int(rnd(box[hi_i] * size / 640))
            if fault == "slice_not_from_the_end":
                a0, a1 = min(max(lo, 0), size), min(max(hi, 0), size)
            else:
                a0, a1, _ = slice(lo, hi).indices(size)      # numpy's im[lo:hi] along one axis
            mine.append([0, a0, W, a1, l] if vertical else [a0, 0, a1, H, l])
        crops.append(mine)
    buf = [[SENTINEL] * 5] * (L * max_det)
    pos = 0
    for l in range(L):
        if fault == "line_offset_off_by_one_line":           # the line's own count added to its offset
            pos += n_chars[l]
        for k, row in enumerate(crops[l]):
            if pos + k < L * max_det:
                buf[pos + k] = row
        if fault != "line_offset_off_by_one_line":
            pos += n_chars[l]
    b5 = torch.tensor(buf, dtype=torch.int32).reshape(L * max_det, 5)
    return sorted_rows, torch.tensor(n_chars, dtype=torch.int32).reshape(L), b5, sum(n_chars)


BOX_MUTANTS = ["unstable_sort", "first_round_half_away", "second_round_half_away", "count_not_clamped", "line_offset_off_by_one_line",
               "minus_zero_label_not_a_character", "slice_not_from_the_end"]


def boxes_torch(rows, counts, max_det, H, W, axis, vertical, nan_first=False):
    """effocr_amd.pipeline._char_boxes_torch on CPU tensors, in boxes_ref's output form: the reference where NaN keys leave Python's
    sorted() undefined (torch.sort ranks a NaN behind every number), and the second, independent statement everywhere else.
    `nan_first`: the mutant that ranks a NaN key in front."""
    from effocr_amd.pipeline import _char_boxes_torch
    L = rows.shape[0]
    r = rows
    if nan_first:
        r = rows.clone()
        r[..., axis] = torch.where(rows[..., axis].isnan(), torch.full((), -float("inf")), rows[..., axis])
    srt, n, x = _char_boxes_torch(r, counts, max_det, H, W, axis, vertical)
    if nan_first:                                            # (the boxes themselves keep their NaN)
        order = torch.sort(torch.where((torch.arange(max_det)[None] < counts[:, None]) & (rows[..., 5] == 0), r[..., axis],
                                       torch.full((), float("inf"))), dim=1, stable=True).indices
        srt = torch.gather(rows[..., :4], 1, order[..., None].expand(-1, -1, 4))
    b5 = torch.full((L * max_det, 5), SENTINEL, dtype=torch.int32)
    b5[:x.shape[0]] = x
    return srt, n.reshape(L), b5, int(x.shape[0])


def check_boxes(got, want, what=""):
    """(sorted, n_chars, crop buffer, total) equal, NaN-aware on the float boxes."""
    (s0, n0, b0, t0), (s1, n1, b1, t1) = got, want
    if t0 != t1 or not torch.equal(n0, n1):
        raise Mismatch(f"{what}: character counts differ: total {t0} vs {t1}; lines {(n0 != n1).nonzero().reshape(-1).tolist()[:8]}")
    same = (s0 == s1) | (s0.isnan() & s1.isnan())
    if not bool(same.all()):
        raise Mismatch(f"{what}: {int((~same).sum())} sorted box elements differ; first at {tuple((~same).nonzero()[0].tolist())}")
    if not torch.equal(b0, b1):
        i = (b0 != b1).any(1).nonzero().reshape(-1)
        raise Mismatch(f"{what}: {i.numel()} crop rows differ; first {int(i[0])}: {b0[i[0]].tolist()} vs {b1[i[0]].tolist()}")
