"""The six kernels of csrc/mnv3g.hip on the MI355X (-m gpu), one launch each through libeffocr_mnv3.so's test entry points
(effocr_mnv3_op_*), against the float64 restatements of tests/mobilenetv3_ops_ref.py within bounds derived from the arithmetic
(tests/test_mobilenetv3_ops_host.py shows on the CPU that each bound rejects every mutant of its operator).  Asymmetric data, output
buffers pre-filled with NaN (an unwritten element fails), and non-finite data through every operator.

Non-finite data: the set of non-finite outputs and their values are torch's, with one documented difference — in mg_pw's 16-bit modes an
inf activation enters the MFMAs as hi = inf plus lo = rn16(inf - inf) = NaN, so where torch gives +-inf the kernel gives NaN (the set of
non-finite outputs is torch's; this is also what an f16 operand overflow looks like, and what EFFOCR_MNV3_EOVERFLOW reports)."""
import pytest
import torch
import torch.nn.functional as F

from effocr_amd import _lib
from tests import mobilenetv3_ops_ref as R
from tests.convops_ref import check_bound, check_exact

pytestmark = pytest.mark.gpu

PRECS = ["fp32", "fp16", "bf16"]
NAN = float("nan")


def _run(dev, name, *args):
    L = _lib.mnv3_lib()
    rc = getattr(L, "effocr_mnv3_op_" + name)(*args, _lib.current_stream(dev))
    assert rc == 0, L.effocr_mnv3_last_error()
    torch.cuda.synchronize(dev)


def _nanbuf(dev, *shape):
    return torch.full(shape, NAN, device=dev)


def run_stem(dev, d):
    B, _, S, _ = d["x"].shape
    x, w, b = d["x"].to(dev), R.pack_stem_w(d["w"]).to(dev), d["b"].to(dev)
    out = _nanbuf(dev, B, S // 2, S // 2, 16)
    _run(dev, "stem", _lib.ptr(x), B, S, _lib.ptr(w), _lib.ptr(b), _lib.ptr(out))
    return out.cpu()


def run_dw(dev, c, d):
    x, w, b = d["x"].to(dev), R.pack_dw_w(d["w"]).to(dev), d["b"].to(dev)
    out = _nanbuf(dev, c.B, c.Ho, c.Ho, c.C)
    _run(dev, "dw", _lib.ptr(x), c.B, c.H, c.C, c.k, c.stride, _lib.ptr(w), _lib.ptr(b), c.act, _lib.ptr(out))
    return out.cpu()


def run_se(dev, d):
    B, HW, C = d["t"].shape
    Rr = d["wr"].shape[0]
    t, wr, br, we, be = (d[k].contiguous().to(dev) for k in ("t", "wr", "br", "we", "be"))
    gate = _nanbuf(dev, B, C)
    _run(dev, "se_gate", _lib.ptr(t), B, HW, C, Rr, _lib.ptr(wr), _lib.ptr(br), _lib.ptr(we), _lib.ptr(be), _lib.ptr(gate))
    return gate.cpu()


def run_pw(dev, c, d, prec):
    a, w, bias = d["a"].to(dev), R.pack_pw_w(d["w"], prec).to(dev), d["bias"].to(dev)
    gate = None if d["gate"] is None else d["gate"].to(dev)
    resid = None if d["resid"] is None else d["resid"].to(dev)
    out = _nanbuf(dev, c.M, c.N)
    _run(dev, "pw", _lib.PREC[prec], _lib.ptr(a), c.M, c.K, _lib.ptr(w), c.N, _lib.ptr(bias), _lib.ptr(gate), c.HW, c.act, _lib.ptr(resid),
         _lib.ptr(out))
    return out.cpu()


def run_pool(dev, d):
    B, HW, C = d["t"].shape
    t = d["t"].to(dev)
    out = _nanbuf(dev, B, C)
    _run(dev, "pool", _lib.ptr(t), B, HW, C, _lib.ptr(out))
    return out.cpu()


def run_finish(dev, e, l2):
    B, D = e.shape
    emb = e.to(dev).clone()
    status = torch.zeros(64, dtype=torch.int32, device=dev)
    _run(dev, "finish", _lib.ptr(emb), B, D, l2, _lib.ptr(status))
    assert not status[1:].any()
    return emb.cpu(), int(status[0].item())


# ---------------------------------------------------------------------------------------------------- parity within the derived bounds
@pytest.mark.parametrize("S,B", R.STEM_CASES)
def test_stem(dev, S, B):
    d = R.stem_data(S, B)
    r = check_bound(run_stem(dev, d), R.stem_ref(d), R.stem_bound(d), f"mg_stem S={S} B={B}")
    print(f"mg_stem S={S} B={B}: error / bound {r:.3f}")


@pytest.mark.parametrize("case", R.DW_CASES, ids=lambda c: c.name)
def test_dw(dev, case):
    d = R.dw_data(case)
    r = check_bound(run_dw(dev, case, d), R.dw_ref(case, d), R.dw_bound(case, d), "mg_dw " + case.name)
    print(f"mg_dw {case.name}: error / bound {r:.3f}")


@pytest.mark.parametrize("B,C,Rr,HW", R.SE_CASES)
def test_se_gate(dev, B, C, Rr, HW):
    d = R.se_data(B, C, Rr, HW)
    r = check_bound(run_se(dev, d), R.se_ref(d), R.se_bound(d), f"mg_se_gate B={B} C={C} R={Rr} HW={HW}")
    print(f"mg_se_gate B={B} C={C} R={Rr} HW={HW}: error / bound {r:.3f}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", R.PW_CASES, ids=lambda c: c.name)
def test_pw(dev, case, prec):
    d = R.pw_data(case, prec)
    r = check_bound(run_pw(dev, case, d, prec), R.pw_ref(case, d), R.pw_bound(case, d, prec), f"mg_pw {case.name} {prec}")
    print(f"mg_pw {case.name} {prec}: error / bound {r:.3f}")


@pytest.mark.parametrize("B,HW,C", R.POOL_CASES)
def test_pool(dev, B, HW, C):
    d = R.pool_data(B, HW, C)
    r = check_bound(run_pool(dev, d), R.pool_ref(d), R.pool_bound(d), f"mg_pool B={B} HW={HW} C={C}")
    print(f"mg_pool B={B} HW={HW} C={C}: error / bound {r:.3f}")


@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("D", R.FINISH_DIMS)
def test_finish(dev, D, l2):
    d = R.finish_data(D)
    got, status = run_finish(dev, d["e"], l2)
    assert status == 0
    if not l2:
        check_exact(got, R.finish_ref(d, l2), f"mg_finish D={D}")
        return
    assert not got[1].any()                                                     # the all-zero row stays 0
    r = check_bound(got, R.finish_ref(d, l2), R.finish_bound(d, l2), f"mg_finish D={D} l2")
    print(f"mg_finish D={D} l2: error / bound {r:.3f}")


@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("D", R.FINISH_DIMS)
@pytest.mark.parametrize("bad", ["inf", "nan", "-inf"])
def test_finish_nonfinite_rows_and_status(dev, D, l2, bad):
    """One inf / NaN column in row 2: the row is what F.normalize gives (NaN in every column for a NaN; 0 and one NaN for an inf), the
    other rows are those of the clean run bit for bit, and the status word is set exactly when a row is non-finite."""
    d = R.finish_data(D)
    clean, status = run_finish(dev, d["e"], l2)
    assert status == 0
    e = d["e"].clone()
    e[2, D - 300] = R.NONFINITE[bad]
    got, status = run_finish(dev, e, l2)
    assert status == 1
    want = F.normalize(e.double(), dim=1) if l2 else e.double()
    assert R.check_nonfinite(got, want, f"mg_finish D={D} l2={l2} {bad}") == (D if (l2 and bad == "nan") else 1)
    check_exact(got[2], want[2], "the non-finite row")
    assert torch.equal(got[[0, 1, 3]], clean[[0, 1, 3]])


# ---------------------------------------------------------------------------------------------------- non-finite data through each operator
def _finite_part(got, ref, bound, what):
    ok = torch.isfinite(ref)
    z = torch.zeros((), dtype=torch.float64)
    check_bound(torch.where(ok, got.double(), z), torch.where(ok, ref, z), torch.where(ok, bound, z + 1), what)


@pytest.mark.parametrize("bad", list(R.NONFINITE))
def test_nonfinite_stem(dev, bad):
    d = R.stem_data(10, 2)
    clean = run_stem(dev, d)
    d["x"][1, 1, 5, 4] = R.NONFINITE[bad]
    got, ref = run_stem(dev, d), R.stem_ref(d)
    assert R.check_nonfinite(got, ref, f"mg_stem {bad}") >= 16
    assert torch.equal(got[0], clean[0])


@pytest.mark.parametrize("bad", list(R.NONFINITE))
@pytest.mark.parametrize("case", [R.DW_CASES[0], R.DW_CASES[1], R.DW_CASES[4]], ids=lambda c: c.name)
def test_nonfinite_dw(dev, case, bad):
    """ReLU and hard-swish: relu(NaN) = NaN, relu(-inf) = 0, hardswish(-inf) = NaN."""
    d = R.dw_data(case)
    clean = run_dw(dev, case, d)
    d["x"][1, case.H // 2, case.H // 2, 5] = R.NONFINITE[bad]
    got, ref = run_dw(dev, case, d), R.dw_ref(case, d)
    n = R.check_nonfinite(got, ref, f"mg_dw {case.name} {bad}")
    assert n >= 1 or bad != "nan"
    _finite_part(got, ref, R.dw_bound(case, R.dw_data(case)), f"mg_dw {case.name} {bad}: the finite outputs")
    assert torch.equal(got[[0, 2]], clean[[0, 2]])


@pytest.mark.parametrize("bad", list(R.NONFINITE))
@pytest.mark.parametrize("B,C,Rr,HW", [R.SE_CASES[0], R.SE_CASES[2]])
def test_nonfinite_se_gate(dev, B, C, Rr, HW, bad):
    """The SE mean, the hidden ReLU and the hard-sigmoid: a NaN pixel makes every gate of its crop NaN; an inf pixel drives the hidden
    units to inf or 0 and the gates to 1, 0 or NaN, as in torch."""
    d = R.se_data(B, C, Rr, HW)
    clean = run_se(dev, d)
    d["t"][1, HW // 2, 3] = R.NONFINITE[bad]
    got, ref = run_se(dev, d), R.se_ref(d)
    n = R.check_nonfinite(got, ref, f"mg_se_gate C={C} {bad}")
    if bad == "nan":
        assert n == C
    check_exact(got[1], ref[1], f"mg_se_gate C={C} {bad}: the crop's gates")
    keep = [i for i in range(B) if i != 1]
    assert torch.equal(got[keep], clean[keep])


@pytest.mark.parametrize("bad", list(R.NONFINITE))
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", [R.PW_CASES[1], R.PW_CASES[4], R.PW_CASES[5]], ids=lambda c: c.name)
def test_nonfinite_pw(dev, case, prec, bad):
    d = R.pw_data(case, prec)
    clean = run_pw(dev, case, d, prec)
    row = case.M // 2
    d["a"][row, 7] = R.NONFINITE[bad]
    got, ref = run_pw(dev, case, d, prec), R.pw_ref(case, d)
    if prec != "fp32" and bad != "nan":
        # (module docstring) hi + lo of an inf is inf + NaN: every output of the row is NaN, where torch has +-inf (or relu(-inf) = 0)
        assert bool(got[row].isnan().all()) and not bool(torch.isfinite(ref[row]).all())
    else:
        R.check_nonfinite(got, ref, f"mg_pw {case.name} {prec} {bad}")
    nf = ~torch.isfinite(got)
    assert bool(nf[row].any()) and not bool(nf[torch.arange(case.M) != row].any())
    assert torch.equal(got[torch.arange(case.M) != row], clean[torch.arange(case.M) != row])


@pytest.mark.parametrize("bad", list(R.NONFINITE))
def test_nonfinite_pool(dev, bad):
    d = R.pool_data(3, 49, 960)
    clean = run_pool(dev, d)
    d["t"][1, 24, 500] = R.NONFINITE[bad]
    got = run_pool(dev, d)
    assert R.check_nonfinite(got, R.pool_ref(d), f"mg_pool {bad}") == 1
    got[1, 500] = clean[1, 500]
    assert torch.equal(got, clean)
