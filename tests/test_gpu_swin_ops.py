"""The five kernels of csrc/swin.hip and the linears of swin_forward on the MI355X (-m gpu), one launch each through libeffocr_swin.so's
test entry points (effocr_swin_op_*), against the float64 restatements of tests/swin_ops_ref.py within bounds derived from the
arithmetic (tests/test_swin_ops_host.py shows on the CPU that each bound rejects the mutants of its operator).  Every bound here is
derived; the one measured constant is swin_ops_ref.ERF_F32_ABS (libm's erff), re-measured below against float64 torch.erf.

Asymmetric data; output buffers pre-filled with NaN (an unwritten element fails); the pad channels C .. Cp-1 of every activation and
the pad columns of q, k and v hold NaN on input (the kernels must not read them) and must be exactly 0 on output.

Non-finite data, what is intended and asserted:
  * LayerNorm-type kernels: a NaN or inf element makes every real output of its token non-finite (inf - mean is NaN), no other token
    changes by a bit, and the pad outputs stay 0.
  * window attention: the running maximum starts at -3e38 and fmaxf drops a NaN score, so a NaN never becomes the maximum; exp(NaN - max)
    is NaN, the sum is NaN and every output of the query is NaN — what torch's softmax gives.  A -inf score is a key of weight 0, a +inf
    score makes the row NaN (inf - inf), both as in torch.
  * head: the status word is set from the final embedding.  LayerNorm turns an inf token into NaN (never into an inf that a later token
    could cancel), and NaN survives the token sum, the mean and F.normalize, so a non-finite input always reaches the check."""
import functools

import pytest
import torch

from effocr_amd import _lib
from tests import swin_ops_ref as R
from tests.convops_ref import assert_exact_premise, check_bound, check_exact
from tests.mobilenetv3_ops_ref import NONFINITE, check_nonfinite

pytestmark = pytest.mark.gpu

NAN = float("nan")
WA_IDS = lambda c: "B%d_H%d_s%d_C%d_Cp%d" % c


def _run(dev, name, *args):
    L = _lib.swin_lib()
    rc = getattr(L, "effocr_swin_op_" + name)(*args, _lib.current_stream(dev))
    assert rc == 0, L.effocr_swin_last_error()
    torch.cuda.synchronize(dev)


def _nanbuf(dev, shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _real(out, C):
    """The real channels of an output [M, Cp] as float32; the pad channels must be exactly 0."""
    out = out.float().cpu()
    assert bool((out[:, C:] == 0).all()), "pad channels of the output are not 0"
    return out[:, :C]


def run_stem(dev, d):
    B, _, S, _ = d["x"].shape
    C0 = d["w"].shape[0]
    x = d["x"].to(dev)
    wt, b, lnw, lnb = (t.contiguous().to(dev) for t in R.pack_stem(d))
    out = _nanbuf(dev, (B * (S // 4) ** 2, 128))
    _run(dev, "stem", _lib.ptr(x), B, S, _lib.ptr(wt), _lib.ptr(b), _lib.ptr(lnw), _lib.ptr(lnb), C0, _lib.ptr(out))
    return _real(out, C0)


def run_ln(dev, d, Cp, prec):
    M, C = d["x"].shape
    x = R.pad_cols(d["x"], Cp, NAN).to(dev)
    lnw, lnb = R.pad_cols(d["lnw"], Cp).to(dev), R.pad_cols(d["lnb"], Cp).to(dev)
    out = _nanbuf(dev, (M, Cp), R.DTYPE[prec])
    _run(dev, "layernorm", _lib.PREC[prec], _lib.ptr(x), M, C, Cp, _lib.ptr(lnw), _lib.ptr(lnb), _lib.ptr(out))
    return _real(out, C)


def run_merge(dev, d, Cp, prec):
    B, H, _, C = d["x"].shape
    x = R.pad_cols(d["x"], Cp, NAN).to(dev)
    lnw, lnb = d["lnw"].to(dev), d["lnb"].to(dev)
    out = _nanbuf(dev, (B * (H // 2) ** 2, 4 * C), R.DTYPE[prec])
    _run(dev, "merge", _lib.PREC[prec], _lib.ptr(x), B, H, C, Cp, _lib.ptr(lnw), _lib.ptr(lnb), _lib.ptr(out))
    return out.float().cpu()


def run_wa(dev, case, d, prec):
    B, H, shift, C, Cp = case
    qkv = R.pack_qkv(d, Cp, R.DTYPE[prec]).to(dev)
    table = d["table"].contiguous().to(dev)
    out = _nanbuf(dev, (B * H * H, Cp), R.DTYPE[prec])
    _run(dev, "window_attention", _lib.PREC[prec], _lib.ptr(qkv), B, H, C, Cp, shift, _lib.ptr(table), _lib.ptr(out))
    return _real(out, C)


def run_head(dev, d, Cp, l2):
    B, HW, C = d["x"].shape
    x = R.pad_cols(d["x"], Cp, NAN).to(dev)
    lnw, lnb = R.pad_cols(d["lnw"], Cp).to(dev), R.pad_cols(d["lnb"], Cp).to(dev)
    emb = _nanbuf(dev, (B, C))
    status = torch.zeros(64, dtype=torch.int32, device=dev)
    _run(dev, "head", _lib.ptr(x), B, HW, C, Cp, _lib.ptr(lnw), _lib.ptr(lnb), l2, _lib.ptr(emb), _lib.ptr(status))
    assert not status[1:].any() and int(status[0]) in (0, 1)                    # only word 0 may change
    return emb.cpu(), int(status[0])


def run_linear(dev, d, epi, prec, in_place=False):
    M, K = d["x"].shape
    N = d["w"].shape[0]
    dt = R.DTYPE[prec]
    x, w, bias = d["x"].to(dt).to(dev), d["w"].to(dt).to(dev), d["bias"].to(dev)
    if in_place:
        out = d["resid"].to(dev).clone()
        resid = out
    else:
        out = _nanbuf(dev, (M, N), R.lin_out_dtype(epi, prec))
        resid = None if d["resid"] is None else d["resid"].to(dev)
    _run(dev, "linear", _lib.PREC[prec], epi, _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(resid), _lib.ptr(out), M, N, K)
    return out.float().cpu()


# ---------------------------------------------------------------------------------------------------- parity within the derived bounds
@pytest.mark.parametrize("S,B,C0", R.STEM_CASES)
def test_stem(dev, S, B, C0):
    d = R.stem_data(S, B, C0)
    r = check_bound(run_stem(dev, d), R.stem_ref(d), R.stem_bound(d), f"stem S={S} B={B} C0={C0}")
    print(f"stem S={S} B={B} C0={C0}: error / bound {r:.3f}")


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("C,Cp,M,kind", R.LN_CASES)
def test_layernorm(dev, C, Cp, M, kind, prec):
    d = R.ln_data(C, Cp, M, kind)
    r = check_bound(run_ln(dev, d, Cp, prec), R.ln_ref(d), R.ln_op_bound(d, prec), f"layernorm C={C} Cp={Cp} M={M} {kind} {prec}")
    print(f"layernorm C={C} Cp={Cp} M={M} {kind} {prec}: error / bound {r:.3f}")


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("B,H,C,Cp", R.MERGE_CASES)
def test_merge(dev, B, H, C, Cp, prec):
    d = R.merge_data(B, H, C, Cp)
    r = check_bound(run_merge(dev, d, Cp, prec), R.merge_ref(d), R.merge_bound(d, prec), f"merge B={B} H={H} C={C} Cp={Cp} {prec}")
    print(f"merge B={B} H={H} C={C} Cp={Cp} {prec}: error / bound {r:.3f}")


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("case,kind", R.WA_RUNS, ids=lambda v: v if isinstance(v, str) else WA_IDS(v))
def test_window_attention(dev, case, kind, prec):
    d = R.wa_data(case, kind, prec)
    r = check_bound(run_wa(dev, case, d, prec), R.wa_ref(case, d), R.wa_bound(case, d, prec), f"window attention {WA_IDS(case)} {kind} {prec}")
    print(f"window attention {WA_IDS(case)} {kind} {prec}: error / bound {r:.3f}")


@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("B,HW,C,Cp,kind", R.HEAD_CASES)
def test_head(dev, B, HW, C, Cp, kind, l2):
    d = R.head_data(B, HW, C, Cp, kind)
    got, status = run_head(dev, d, Cp, l2)
    assert status == 0
    if kind == "zero":
        assert bool((got == 0).all())                                           # 0 / max(0, 1e-12): the zero vector, not NaN
        return
    r = check_bound(got, R.head_ref(d, l2), R.head_bound(d, l2), f"head B={B} HW={HW} C={C} Cp={Cp} l2={l2}")
    print(f"head B={B} HW={HW} C={C} Cp={Cp} l2={l2}: error / bound {r:.3f}")


ROLES = R.linear_roles()
# one launch per test: every (N, K) of the forward with its epilogue x M = 1, 49, 130 and one row past the row tile of the kernel it
# dispatches to x (the residual linears in place, resid == out as swin_forward runs them, and out of place; the reduction with a zero and
# a non-zero bias)
VARIANTS = {R.EPI_BIAS: ["plain"], R.EPI_BIAS_GELU: ["plain"], R.EPI_BIAS_RESID: ["in place", "out of place"],
            R.EPI_BIAS_F32: ["zero bias", "bias"]}
LINEAR_RUNS = [(*role, mi, prec, v) for role in ROLES for mi in range(4) for prec in R.PRECS for v in VARIANTS[role[3]]]


@functools.lru_cache(maxsize=4)
def _linear_case(N, K, M, epi, prec, zero_bias):
    """(data, float64 reference, bound), shared by the in-place and the out-of-place run."""
    d = R.lin_data(N, K, M, epi, prec, zero_bias=zero_bias)
    return d, R.lin_ref(d, epi), R.lin_bound(d, epi, prec)


@pytest.mark.parametrize("name,N,K,epi,mi,prec,variant", LINEAR_RUNS,
                         ids=[f"{r[0]}-{R.LINEAR_ROW_IDS[r[4]]}-{r[5]}-{r[6].replace(' ', '_')}" for r in LINEAR_RUNS])
def test_linear(dev, name, N, K, epi, mi, prec, variant):
    M = R.linear_rows(prec)[mi]
    d, ref, bound = _linear_case(N, K, M, epi, prec, variant == "zero bias")
    what = f"linear {name} N={N} K={K} {R.EPI_NAME[epi]} M={M} {prec} {variant}"
    r = check_bound(run_linear(dev, d, epi, prec, variant == "in place"), ref, bound, what)
    print(f"{what}: error / bound {r:.3f}")


@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("epi", [R.EPI_BIAS, R.EPI_BIAS_RESID, R.EPI_BIAS_F32])
def test_linear_exact(dev, epi, prec):
    """Small integers: every partial sum is exact in fp32 in any order, so the kernel equals float64 bit for bit."""
    d = R.lin_data(384, 128, 130, epi, prec, kind="exact")
    assert_exact_premise(d["x"].abs().double() @ d["w"].abs().double().T, d["bias"], d["resid"])
    for in_place in ([True, False] if epi == R.EPI_BIAS_RESID else [False]):
        got = run_linear(dev, d, epi, prec, in_place)
        check_exact(got.to(R.lin_out_dtype(epi, prec)), R.lin_ref(d, epi), f"linear exact {R.EPI_NAME[epi]} {prec}")


def test_erf_f32_measured_constant_holds(dev):
    """The fp32 GELU epilogue alone: an identity weight and a zero bias make the linear's sum exactly x.  Against float64 torch.erf."""
    x = torch.linspace(-6, 6, 240001, dtype=torch.float64).float()
    x = torch.cat([x, torch.zeros(-x.numel() % 128)]).view(-1, 128)
    d = dict(x=x, w=torch.eye(128), bias=torch.zeros(128), resid=None)
    got = run_linear(dev, d, R.EPI_BIAS_GELU, "fp32").double()
    xd = x.double()
    nz = xd != 0
    worst = ((got - R.gelu64(xd)).abs()[nz] / (0.5 * xd.abs()[nz])).max().item()
    print(f"fp32 GELU epilogue: worst |gelu - gelu64| / (0.5 |x|) over [-6, 6] = {worst:.3e} = {worst / R.U:.2f} u "
          f"(ERF_F32_ABS = {R.ERF_F32_ABS:.3e}, the bound term twice it)")
    assert bool((got[~nz] == 0).all()) and worst <= 2 * R.ERF_F32_ABS            # the GELU bound's term


# ---------------------------------------------------------------------------------------------------- non-finite data
def _others_equal(got, clean, rows):
    keep = torch.ones(got.shape[0], dtype=torch.bool)
    keep[rows] = False
    assert torch.equal(got[keep], clean[keep]), "an output outside the planted token's changed"
    return keep


@pytest.mark.parametrize("bad", list(NONFINITE))
def test_nonfinite_stem(dev, bad):
    S, B, C0 = 12, 3, 96
    d = R.stem_data(S, B, C0)
    clean = run_stem(dev, d)
    d["x"][1, 2, 6, 9] = NONFINITE[bad]                                         # crop 1, patch (1, 2)
    got = run_stem(dev, d)                                                      # (run_stem asserts the pad outputs to be 0)
    t = 1 * 9 + 1 * 3 + 2
    _others_equal(got, clean, [t])
    assert not torch.isfinite(got[t]).any()
    check_nonfinite(got, R.stem_ref(d), f"stem {bad}")


@pytest.mark.parametrize("bad", list(NONFINITE))
@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("C,Cp,M", [(96, 128, 37), (384, 384, 5)])
def test_nonfinite_layernorm(dev, C, Cp, M, prec, bad):
    d = R.ln_data(C, Cp, M, "real")
    clean = run_ln(dev, d, Cp, prec)
    t = M - 2
    d["x"][t, C - 3] = NONFINITE[bad]
    got = run_ln(dev, d, Cp, prec)
    _others_equal(got, clean, [t])
    assert not torch.isfinite(got[t]).any()


@pytest.mark.parametrize("bad", list(NONFINITE))
@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("B,H,C,Cp", [(3, 4, 96, 128), (2, 2, 384, 384)])
def test_nonfinite_merge(dev, B, H, C, Cp, prec, bad):
    d = R.merge_data(B, H, C, Cp)
    clean = run_merge(dev, d, Cp, prec)
    d["x"][1, H - 1, 1, 7] = NONFINITE[bad]
    got = run_merge(dev, d, Cp, prec)
    Ho = H // 2
    t = 1 * Ho * Ho + (H - 1) // 2 * Ho + 0
    _others_equal(got, clean, [t])
    assert not torch.isfinite(got[t]).any()


def _window_tokens(case, token):
    """The 49 tokens (rows of the output) of the (crop, window) that holds `token`."""
    B, H, shift, C, Cp = case
    ids = torch.arange(B * H * H, dtype=torch.float64).view(B, H, H, 1)
    if shift:
        ids = torch.roll(ids, (-shift, -shift), (1, 2))
    w = R.windows(ids, R.WS).squeeze(-1).long()
    return w[(w == token).any(1)][0]


@pytest.mark.parametrize("bad", list(NONFINITE))
@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("case", [R.WA_CASES[2], R.WA_CASES[5]], ids=WA_IDS)
def test_nonfinite_window_attention_key(dev, case, prec, bad):
    B, H, shift, C, Cp = case
    d = R.wa_data(case, "random", prec)
    clean = run_wa(dev, case, d, prec)
    b, y, x, h = B - 1, H - 2, 1, 1                                             # a token whose window wraps round the map
    d["k"][b, y, x, h * R.HD + 5] = NONFINITE[bad]
    got = run_wa(dev, case, d, prec)
    rows = _window_tokens(case, (b * H + y) * H + x)
    cols = slice(h * R.HD, (h + 1) * R.HD)
    keep = _others_equal(got, clean, rows)
    assert keep.sum() == B * H * H - 49
    other = torch.ones(C, dtype=torch.bool)
    other[cols] = False
    assert torch.equal(got[rows][:, other], clean[rows][:, other])              # the window's other heads
    if bad == "nan":
        assert not torch.isfinite(got[rows][:, cols]).any()
    check_nonfinite(got, R.wa_ref(case, d), f"window attention {bad}")


@pytest.mark.parametrize("bad", list(NONFINITE))
@pytest.mark.parametrize("prec", R.PRECS)
@pytest.mark.parametrize("case", [R.WA_CASES[2], R.WA_CASES[5]], ids=WA_IDS)
def test_nonfinite_window_attention_query(dev, case, prec, bad):
    B, H, shift, C, Cp = case
    d = R.wa_data(case, "random", prec)
    clean = run_wa(dev, case, d, prec)
    b, y, x, h = 0, H - 1, H - 1, 0
    d["q"][b, y, x, h * R.HD + 31] = NONFINITE[bad]
    got = run_wa(dev, case, d, prec)
    t = (b * H + y) * H + x
    _others_equal(got, clean, [t])
    assert torch.equal(got[t, R.HD:], clean[t, R.HD:])
    assert not torch.isfinite(got[t, :R.HD]).any()


@pytest.mark.parametrize("bad", list(NONFINITE))
@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("B,HW,C,Cp", [(3, 49, 768, 768), (2, 4, 128, 256)])
def test_nonfinite_head_rows_and_status(dev, B, HW, C, Cp, l2, bad):
    d = R.head_data(B, HW, C, Cp, "real")
    clean, status = run_head(dev, d, Cp, l2)
    assert status == 0
    d["x"][1, HW // 2, C - 5] = NONFINITE[bad]
    got, status = run_head(dev, d, Cp, l2)
    assert status == 1
    _others_equal(got, clean, [1])
    assert check_nonfinite(got, R.head_ref(d, l2), f"head {bad}") == C
