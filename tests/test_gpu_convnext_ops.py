"""The four kernels of csrc/convnext.hip and the layer-scale linear of convnext_forward on the MI355X (-m gpu), one launch each through
the test-only libeffocr_convops.so (effocr_convops_cnx_*, effocr_convops_linear), against the float64 restatements of
tests/convnext_ops_ref.py within bounds derived from the arithmetic (tests/test_convnext_ops_host.py shows on the CPU that each bound
rejects the mutants of its operator, and that the restatements chained together are the network).  No tolerance here is measured.

Asymmetric data; output buffers pre-filled with NaN (an unwritten element fails); the pad channels C .. Cp-1 of every activation hold
NaN on input (the kernels must not read them) and must be exactly 0 on output.  Every element of every output is compared.

Non-finite data (the semantics of tests/test_gpu_swin_ops.py's LayerNorm-type kernels): a NaN or inf input element makes every real
output of the tokens whose 7x7 window (depthwise) or whose own row (stem, ln_s2d) contains it non-finite — inf times a tap is inf and
inf - mean is NaN — no other token changes by a bit, and the pad outputs stay 0.  Head: the pooled sum carries a NaN or inf token into
its image's row, LayerNorm makes the whole row NaN, F.normalize keeps it; the status word is 1 then and 0 on finite input, only that
image's embedding is non-finite and only word 0 of the status buffer changes.

test_chain_equals_the_product runs the whole network through the operator entry points on weights packed in Python and expects the
product library's embedding bit for bit."""
import functools

import pytest
import torch

from effocr_amd import _lib
from effocr_amd import weights as W
from tests import convnext_ops_ref as R
from tests import convops_lib as CL
from tests import swin_ops_ref as S
from tests.convops_ref import check_bound
from tests.mobilenetv3_ops_ref import NONFINITE

pytestmark = pytest.mark.gpu

NAN = float("nan")
CASE_ID = lambda v: "B%d_%dx%d_C%d_Cp%d" % v if isinstance(v, tuple) else str(v)


def _call(dev, name, *args):
    rc = getattr(CL.lib(), "effocr_convops_" + name)(*args, _lib.current_stream(dev))
    torch.cuda.synchronize(dev)
    return rc


def _run(dev, name, *args):
    rc = _call(dev, name, *args)
    assert rc == 0, f"rc {rc}: {CL.last_error()}"


def _nanbuf(dev, shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _real(out, C):
    """The real channels of an output [M, Cp] as float32; the pad channels must be exactly 0."""
    out = out.float().cpu()
    assert bool((out[:, C:] == 0).all()), "pad channels of the output are not 0"
    return out[:, :C]


def run_stem(dev, d):
    B, _, S_, _ = d["x"].shape
    C0 = d["w"].shape[0]
    x = d["x"].contiguous().to(dev)
    wt, b, lnw, lnb = (t.contiguous().to(dev) for t in S.pack_stem(d))
    out = _nanbuf(dev, (B * (S_ // 4) ** 2, 128))
    _run(dev, "cnx_stem", CL.ptr(x), B, S_, CL.ptr(wt), CL.ptr(b), CL.ptr(lnw), CL.ptr(lnb), C0, CL.ptr(out))
    return _real(out, C0)


def run_dw(dev, d, Cp, prec):
    B, H, W_, C = d["x"].shape
    x = S.pad_cols(d["x"], Cp, NAN).to(dev)
    w, b, lnw, lnb = (t.contiguous().to(dev) for t in R.pack_dw(d, Cp))
    out = _nanbuf(dev, (B * H * W_, Cp), R.DTYPE[prec])
    _run(dev, "cnx_dwconv_ln", CL.PREC[prec], CL.ptr(x), B, H, W_, C, Cp, CL.ptr(w), CL.ptr(b), CL.ptr(lnw), CL.ptr(lnb), CL.ptr(out))
    return _real(out, C)


def run_s2d(dev, d, Cp, prec):
    B, H, W_, C = d["x"].shape
    x = S.pad_cols(d["x"], Cp, NAN).to(dev)
    lnw, lnb = S.pad_cols(d["lnw"], Cp).to(dev), S.pad_cols(d["lnb"], Cp).to(dev)
    out = _nanbuf(dev, (B * (H // 2) * (W_ // 2), 4 * C), R.DTYPE[prec])
    _run(dev, "cnx_ln_s2d", CL.PREC[prec], CL.ptr(x), B, H, W_, C, Cp, CL.ptr(lnw), CL.ptr(lnb), CL.ptr(out))
    return out.float().cpu()


def run_head(dev, d, Cp, l2):
    B, HW, C = d["x"].shape
    x = S.pad_cols(d["x"], Cp, NAN).to(dev)
    lnw, lnb = S.pad_cols(d["lnw"], Cp).to(dev), S.pad_cols(d["lnb"], Cp).to(dev)
    emb = _nanbuf(dev, (B, C))
    status = torch.zeros(64, dtype=torch.int32, device=dev)
    _run(dev, "cnx_head", CL.ptr(x), B, HW, C, Cp, CL.ptr(lnw), CL.ptr(lnb), l2, CL.ptr(emb), CL.ptr(status))
    assert not status[1:].any() and int(status[0]) in (0, 1)                    # only word 0 may change
    return emb.cpu(), int(status[0])


def run_linear(dev, d, epi, prec, in_place=False):
    M, K = d["x"].shape
    N = d["w"].shape[0]
    dt = R.DTYPE[prec]
    x, w, bias = d["x"].to(dt).to(dev), d["w"].to(dt).to(dev), d["bias"].to(dev)
    resid = scale = None
    if epi == R.EPI_BIAS_SCALE_RESID:
        resid, scale = d["resid"].to(dev).clone(), d["scale"].to(dev)
    out = resid if in_place else _nanbuf(dev, (M, N), dt if epi == R.EPI_BIAS_GELU else torch.float32)
    _run(dev, "linear", CL.PREC[prec], epi, CL.ptr(x), CL.ptr(w), CL.ptr(bias), CL.ptr(resid), CL.ptr(scale), CL.ptr(out), M, N, K)
    if resid is not None and not in_place:
        assert torch.equal(resid.cpu(), d["resid"]), "the residual was modified by an out-of-place call"
    return out.float().cpu()


# ---------------------------------------------------------------------------------------------------- parity within the derived bounds
@pytest.mark.parametrize("S_,B,C0,kind", R.STEM_CASES)
def test_stem(dev, S_, B, C0, kind):
    d = R.stem_data(S_, B, C0, kind)
    what = f"cnx_stem S={S_} B={B} C0={C0} {kind}"
    r = check_bound(run_stem(dev, d), R.stem_ref(d), R.stem_bound(d), what)
    print(f"{what}: error / bound {r:.3f}")


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("case,kind", R.DW_RUNS, ids=CASE_ID)
def test_dwconv_ln(dev, case, kind, prec):
    d = R.dw_data(case, kind)
    what = f"cnx_dwconv_ln {CASE_ID(case)} {kind} {prec}"
    r = check_bound(run_dw(dev, d, case[4], prec), R.dw_ref(d), R.dw_bound(d, prec), what)
    print(f"{what}: error / bound {r:.3f}")


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("case,kind", R.S2D_RUNS, ids=CASE_ID)
def test_ln_s2d(dev, case, kind, prec):
    d = R.s2d_data(case, kind)
    what = f"cnx_ln_s2d {CASE_ID(case)} {kind} {prec}"
    r = check_bound(run_s2d(dev, d, case[4], prec), R.s2d_ref(d), R.s2d_bound(d, prec), what)
    print(f"{what}: error / bound {r:.3f}")


@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("B,HW,C,Cp,kind", R.HEAD_CASES)
def test_head(dev, B, HW, C, Cp, kind, l2):
    d = R.head_data(B, HW, C, Cp, kind)
    got, status = run_head(dev, d, Cp, l2)
    assert status == 0
    if kind == "const":
        assert bool((got[0] == 0).all())                                        # 0 / max(0, 1e-12): the zero vector, not NaN
    what = f"cnx_head B={B} HW={HW} C={C} Cp={Cp} {kind} l2={l2}"
    r = check_bound(got, R.head_ref(d, l2), R.head_bound(d, l2), what)
    print(f"{what}: error / bound {r:.3f}")


LIN4_RUNS = ([(N, K, mi, "real", prec, v) for N, K in R.FC2_SHAPES for mi in range(3) for prec in R.PRECS for v in ("in place", "out of place")]
             + [(256, 768, 1, "tiny", prec, "in place") for prec in R.PRECS] + [(128, 384, 1, "pad", prec, "in place") for prec in R.PRECS])


@functools.lru_cache(maxsize=4)
def _lin4_case(N, K, M, prec, kind):
    """(data, float64 reference, bound), shared by the in-place and the out-of-place run."""
    d = R.lin4_data(N, K, M, prec, kind)
    return d, R.lin4_ref(d), R.lin4_bound(d)


@pytest.mark.parametrize("N,K,mi,kind,prec,variant", LIN4_RUNS,
                         ids=[f"N{r[0]}_K{r[1]}-{R.LIN4_ROW_IDS[r[2]]}-{r[3]}-{r[4]}-{r[5].replace(' ', '_')}" for r in LIN4_RUNS])
def test_linear_scale_resid(dev, N, K, mi, kind, prec, variant):
    M = R.lin4_rows(prec)[mi]
    d, ref, bound = _lin4_case(N, K, M, prec, kind)
    what = f"linear scale+resid N={N} K={K} M={M} {kind} {prec} {variant}"
    got = run_linear(dev, d, R.EPI_BIAS_SCALE_RESID, prec, variant == "in place")
    if kind == "pad":
        assert bool((got[:, 96:] == 0).all()), "pad channels of the residual stream are not 0"
    r = check_bound(got, ref, bound, what)
    print(f"{what}: error / bound {r:.3f}")


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("name,N,K,epi", [r for r in R.cnx_linear_roles() if r[0] in ("s0_fc1", "s1_downsample")], ids=lambda v: v if isinstance(v, str) else None)
def test_linear_entry_point_epilogues_1_and_5(dev, name, N, K, epi, prec):
    """The entry point itself on one role of each epilogue; every role's operator test is tests/test_gpu_swin_ops.py::test_linear."""
    assert R.extra_linear_roles() == []
    d = S.lin_data(N, K, 49, epi, prec)
    what = f"linear {name} N={N} K={K} {S.EPI_NAME[epi]} M=49 {prec}"
    r = check_bound(run_linear(dev, d, epi, prec), S.lin_ref(d, epi), S.lin_bound(d, epi, prec), what)
    print(f"{what}: error / bound {r:.3f}")


# ---------------------------------------------------------------------------------------------------- invariance, bit for bit
def _crop(d, b, keys=("x",)):
    """The data of crop b (or of the rows of a slice) alone."""
    sl = b if isinstance(b, slice) else slice(b, b + 1)
    return {k: (v[sl] if k in keys else v) for k, v in d.items()}


def test_stem_is_crop_by_crop(dev):
    d = R.stem_data(32, 3, 96)
    assert torch.equal(run_stem(dev, d), torch.cat([run_stem(dev, _crop(d, b)) for b in range(3)]))


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("case", [(3, 7, 7, 96, 128), (2, 9, 11, 192, 256), (2, 4, 4, 768, 768)], ids=CASE_ID)
def test_dwconv_ln_is_crop_by_crop_and_ignores_its_neighbours(dev, case, prec):
    B, H, W_, C, Cp = case
    d = R.dw_data(case)
    whole = run_dw(dev, d, Cp, prec)
    assert torch.equal(whole, torch.cat([run_dw(dev, _crop(d, b), Cp, prec) for b in range(B)]))
    g = torch.Generator().manual_seed(1)
    for pos, n in ((2, 5), (0, 3), (3, 4)):                                     # crop 1 of the case inside batches of other crops
        big = dict(d, x=3 * torch.randn(n, H, W_, C, generator=g) + 2)
        big["x"][pos] = d["x"][1]
        assert torch.equal(run_dw(dev, big, Cp, prec).view(n, H * W_, C)[pos], whole.view(B, H * W_, C)[1]), (pos, n)


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("case", [(3, 2, 2, 96, 128), (2, 4, 2, 192, 256)], ids=CASE_ID)
def test_ln_s2d_is_crop_by_crop(dev, case, prec):
    d = R.s2d_data(case)
    assert torch.equal(run_s2d(dev, d, case[4], prec), torch.cat([run_s2d(dev, _crop(d, b), case[4], prec) for b in range(case[0])]))


@pytest.mark.parametrize("l2", [0, 1])
def test_head_is_crop_by_crop(dev, l2):
    d = R.head_data(3, 49, 768, 768, "real")
    assert torch.equal(run_head(dev, d, 768, l2)[0], torch.cat([run_head(dev, _crop(d, b), 768, l2)[0] for b in range(3)]))


@pytest.mark.parametrize("prec", R.PRECS)
def test_linear_scale_resid_is_row_by_row(dev, prec):
    """A crop is 49 rows here: the rows of two crops in one call equal the two calls on their own rows (no split-K, no M-dependent path)."""
    d = R.lin4_data(256, 768, 98, prec)
    whole = run_linear(dev, d, R.EPI_BIAS_SCALE_RESID, prec, True)
    parts = [run_linear(dev, _crop(d, slice(a, a + 49), ("x", "resid")), R.EPI_BIAS_SCALE_RESID, prec, True) for a in (0, 49)]
    assert torch.equal(whole, torch.cat(parts))


# ---------------------------------------------------------------------------------------------------- non-finite data
def _planted(got, clean, rows):
    """Every output of `rows` non-finite, every other row unchanged bit for bit."""
    keep = torch.ones(got.shape[0], dtype=torch.bool)
    keep[rows] = False
    assert torch.equal(got[keep], clean[keep]), "an output outside the planted element's reach changed"
    assert not torch.isfinite(got[~keep]).any(), "a finite output inside the planted element's reach"


@pytest.mark.parametrize("bad", list(NONFINITE))
def test_nonfinite_stem(dev, bad):
    d = R.stem_data(32, 3, 96)
    clean = run_stem(dev, d)
    d["x"][1, 2, 6, 9] = NONFINITE[bad]                                         # crop 1, patch (1, 2)
    _planted(run_stem(dev, d), clean, [1 * 64 + 1 * 8 + 2])                     # (run_stem asserts the pad outputs to be 0)


@pytest.mark.parametrize("bad", list(NONFINITE))
@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("case,y,x", [((2, 9, 11, 192, 256), 7, 8), ((3, 7, 7, 96, 128), 0, 6)], ids=CASE_ID)
def test_nonfinite_dwconv_ln(dev, case, y, x, prec, bad):
    B, H, W_, C, Cp = case
    d = R.dw_data(case)
    clean = run_dw(dev, d, Cp, prec)
    b = B - 2
    d["x"][b, y, x, C - 3] = NONFINITE[bad]
    rows = [(b * H + yy) * W_ + xx for yy in range(max(0, y - 3), min(H, y + 4)) for xx in range(max(0, x - 3), min(W_, x + 4))]
    _planted(run_dw(dev, d, Cp, prec), clean, rows)


@pytest.mark.parametrize("bad", list(NONFINITE))
@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("case", [(3, 2, 2, 96, 128), (2, 4, 2, 192, 256)], ids=CASE_ID)
def test_nonfinite_ln_s2d(dev, case, prec, bad):
    B, H, W_, C, Cp = case
    d = R.s2d_data(case)
    clean = run_s2d(dev, d, Cp, prec)
    b, y, x = 1, H - 1, 0
    d["x"][b, y, x, 7] = NONFINITE[bad]
    got = run_s2d(dev, d, Cp, prec)
    row, q = (b * (H // 2) + y // 2) * (W_ // 2) + x // 2, (y & 1) * 2 + (x & 1)
    got4, clean4 = got.view(-1, 4, C), clean.view(-1, 4, C)                     # [row][quadrant] = one token each
    _planted(got4.reshape(-1, C), clean4.reshape(-1, C), [row * 4 + q])


@pytest.mark.parametrize("bad", list(NONFINITE))
@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("B,HW,C,Cp", [(3, 49, 768, 768), (2, 4, 96, 128)])
def test_nonfinite_head_rows_and_status(dev, B, HW, C, Cp, l2, bad):
    d = R.head_data(B, HW, C, Cp, "real")
    clean, status = run_head(dev, d, Cp, l2)
    assert status == 0
    d["x"][1, HW // 2, C - 5] = NONFINITE[bad]
    got, status = run_head(dev, d, Cp, l2)                                      # (run_head: only word 0 of the status buffer may change)
    assert status == 1
    _planted(got, clean, [1])


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_output_untouched(dev):
    """Each refused shape returns the negative code, names its operator in last_error and writes nothing."""
    L = CL.lib()
    s = _lib.current_stream(dev)
    buf = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=dev)
    out = _nanbuf(dev, (1 << 16,))
    x, v = buf(1 << 16), buf(4096)

    def refused(rc, code, word):
        torch.cuda.synchronize(dev)
        assert rc == code and word in CL.last_error(), (rc, CL.last_error())
        assert bool(out.isnan().all()), f"{word}: a refused call wrote to its output"

    for S_, C0 in R.STEM_REFUSALS:
        refused(L.effocr_convops_cnx_stem(CL.ptr(x), 1, S_, CL.ptr(x), CL.ptr(v), CL.ptr(v), CL.ptr(v), C0, CL.ptr(out), s), CL.EUNSUPPORTED, "cnx_stem")
    for C, Cp in R.DW_REFUSALS:
        refused(L.effocr_convops_cnx_dwconv_ln(CL.PREC_FP32, CL.ptr(x), 1, 2, 2, C, Cp, CL.ptr(x), CL.ptr(v), CL.ptr(v), CL.ptr(v), CL.ptr(out), s),
                CL.EUNSUPPORTED, "cnx_dwconv_ln")
    for H, W_ in R.S2D_REFUSALS:
        refused(L.effocr_convops_cnx_ln_s2d(CL.PREC_FP32, CL.ptr(x), 1, H, W_, 96, 128, CL.ptr(v), CL.ptr(v), CL.ptr(out), s), CL.EUNSUPPORTED, "cnx_ln_s2d")
    refused(L.effocr_convops_cnx_head(CL.ptr(x), 1, 4, 96, 192, CL.ptr(v), CL.ptr(v), 0, CL.ptr(out), None, s), CL.EUNSUPPORTED, "cnx_head")
    lin = lambda epi, resid, scale, n=128: L.effocr_convops_linear(CL.PREC_FP32, epi, CL.ptr(x), CL.ptr(x), CL.ptr(v), resid, scale, CL.ptr(out), 4, n, 128, s)
    for epi in (0, 2, 3, 6):
        refused(lin(epi, CL.ptr(x), CL.ptr(v)), CL.EINVAL, "convops_linear")
    refused(lin(4, None, CL.ptr(v)), CL.EINVAL, "convops_linear")
    refused(lin(4, CL.ptr(x), None), CL.EINVAL, "convops_linear")
    refused(lin(4, CL.ptr(x), CL.ptr(v), n=96), CL.EUNSUPPORTED, "gemm_nt")


# ---------------------------------------------------------------------------------------------------- the chain is the product
def _pack_chain(sd, prec, dev):
    """The state dict in the operators' layouts, as csrc/api.hip: pack_convnext lays them out, restated in Python: vectors zero-padded to
    Cp, fc1 [4C][Cp] with zero columns, fc2 [Cp][4C] with zero rows, the downsample [Cp][kh][kw][C_prev]; linear weights in the operand type."""
    dt = R.DTYPE[prec]
    stem, stages, head = R.chain_parts(sd)
    up = lambda t: t.contiguous().to(dev)
    vec = lambda t, Cp: up(S.pad_cols(t, Cp))
    rows = lambda w, Np: up(torch.cat([w, torch.zeros(Np - w.shape[0], w.shape[1])]).to(dt))
    out = dict(stem=[up(t) for t in S.pack_stem(stem)], stages=[])
    for (C, Cp), (ds, blocks) in zip(R.STAGES, stages):
        pds = None if ds is None else dict(lnw=up(ds["lnw"]), lnb=up(ds["lnb"]), w=rows(ds["w"], Cp), bias=vec(ds["bias"], Cp))
        pb = [dict(dw=[up(t) for t in R.pack_dw(dw, Cp)], w1=up(S.pad_cols(fc1["w"], Cp).to(dt)), b1=up(fc1["bias"]), w2=rows(fc2["w"], Cp),
                   b2=vec(fc2["bias"], Cp), gamma=vec(fc2["scale"], Cp)) for dw, fc1, fc2 in blocks]
        out["stages"].append((pds, pb))
    out["head"] = (vec(head["lnw"], 768), vec(head["lnb"], 768))
    return out


def _chain_gpu(dev, P, x, prec, l2=0):
    dt, pr = R.DTYPE[prec], CL.PREC[prec]
    B, H = x.shape[0], x.shape[-1] // 4
    xs = _nanbuf(dev, (B * H * H, 128))
    _run(dev, "cnx_stem", CL.ptr(x), B, 4 * H, *(CL.ptr(t) for t in P["stem"]), 96, CL.ptr(xs))
    for i, ((C, Cp), (ds, blocks)) in enumerate(zip(R.STAGES, P["stages"])):
        if ds is not None:
            Cv, Cvp = R.STAGES[i - 1]
            A = _nanbuf(dev, (B * (H // 2) ** 2, 4 * Cv), dt)
            _run(dev, "cnx_ln_s2d", pr, CL.ptr(xs), B, H, H, Cv, Cvp, CL.ptr(ds["lnw"]), CL.ptr(ds["lnb"]), CL.ptr(A))
            H //= 2
            xs = _nanbuf(dev, (B * H * H, Cp))
            _run(dev, "linear", pr, R.EPI_BIAS_F32, CL.ptr(A), CL.ptr(ds["w"]), CL.ptr(ds["bias"]), None, None, CL.ptr(xs), B * H * H, Cp, 4 * Cv)
        M = B * H * H
        for L in blocks:
            A, hid = _nanbuf(dev, (M, Cp), dt), _nanbuf(dev, (M, 4 * C), dt)
            _run(dev, "cnx_dwconv_ln", pr, CL.ptr(xs), B, H, H, C, Cp, *(CL.ptr(t) for t in L["dw"]), CL.ptr(A))
            _run(dev, "linear", pr, R.EPI_BIAS_GELU, CL.ptr(A), CL.ptr(L["w1"]), CL.ptr(L["b1"]), None, None, CL.ptr(hid), M, 4 * C, Cp)
            _run(dev, "linear", pr, R.EPI_BIAS_SCALE_RESID, CL.ptr(hid), CL.ptr(L["w2"]), CL.ptr(L["b2"]), CL.ptr(xs), CL.ptr(L["gamma"]), CL.ptr(xs),
                 M, Cp, 4 * C)
    emb = _nanbuf(dev, (B, 768))
    status = torch.zeros(64, dtype=torch.int32, device=dev)
    _run(dev, "cnx_head", CL.ptr(xs), B, H * H, 768, 768, CL.ptr(P["head"][0]), CL.ptr(P["head"][1]), l2, CL.ptr(emb), CL.ptr(status))
    assert not status.any()
    return emb


@pytest.mark.parametrize("prec", R.PRECS)
def test_chain_equals_the_product(dev, prec):
    """convnext_tiny at 32^2, B = 2, through the operator entry points on weights packed here = HipEncoder.forward on the same crops, bit
    for bit: both libraries compile the same sources with the same flags and every reduction order is fixed by the shapes.  This ties
    the Python restatement of the layouts (and with it every test above) to pack_convnext."""
    from effocr_amd.encoders import HipEncoder
    sd = W.init_state_dict("convnext_tiny", seed=3, img_size=32)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(dev)
    enc = HipEncoder("convnext_tiny", sd, img_size=32, precision=prec, device=dev)
    P = _pack_chain(sd, prec, dev)
    for l2 in (0, 1):
        want = enc.forward(x, normalize=bool(l2))
        enc.check_status()
        got = _chain_gpu(dev, P, x, prec, l2)
        diff = (got != want).sum().item()
        print(f"chain vs product {prec} l2={l2}: {diff} of {want.numel()} elements differ"
              + (f", largest difference {(got - want).abs().max().item():.3e}" if diff else ""))
        assert torch.equal(got, want)
