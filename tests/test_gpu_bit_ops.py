"""libeffocr_bit.so's three operators on the MI355X (-m gpu), one launch per case through the effocr_bit_op_* entry points, in float / f16
/ bf16, against the float64 restatements of tests/bit_ref.py on the already-rounded inputs.  The bounds are bit_ref's (one output
rounding plus the fp32 statistics budget; tests/test_bit_host.py shows that they reject every mutant); the stem pool is exact."""
import pytest
import torch

from effocr_amd import _lib
from tests import bit_ref as R

pytestmark = pytest.mark.gpu


def _gn(dev, prec, x, gamma, beta, inplace=False):
    L = _lib.bit_lib()
    B, HW, C = x.shape
    xd = x.to(R.DTYPES[prec]).to(dev).contiguous()
    gd, bd = gamma.float().to(dev), beta.float().to(dev)
    out = xd if inplace else torch.empty_like(xd)
    tiles = -(-HW // max(1, 16384 // C))
    scratch = torch.empty(B * tiles * 512, dtype=torch.uint8, device=dev)
    _lib.bit_check(L.effocr_bit_op_groupnorm_relu(_lib.PREC[prec], _lib.ptr(xd), B, HW, C, _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(out),
                                                  _lib.ptr(scratch), scratch.numel(), _lib.current_stream(dev)), "effocr_bit_op_groupnorm_relu")
    torch.cuda.synchronize(dev)
    return out.cpu().double()


@pytest.mark.parametrize("name,prec", [(n, p) for n, c in R.GN_CASES.items() for p in c[5]])
def test_groupnorm_relu(dev, name, prec):
    x, gamma, beta = R.gn_case(name, prec)
    ref, bound = R.gn_relu_ref(x, gamma, beta), R.gn_bound(x, gamma, beta, prec)
    got = _gn(dev, prec, x, gamma, beta)
    w = R.worst(got, ref, bound)
    print(f"groupnorm+relu {name} {prec}: worst |err| / bound {w:.3f}, max |err| {(got - ref).abs().max():.3e}")
    assert w <= 1
    assert (got >= 0).all()
    assert torch.equal(_gn(dev, prec, x, gamma, beta, inplace=True), got)      # in place, as the forward runs norm2 / norm3


def test_groupnorm_relu_is_call_size_invariant(dev):
    x, gamma, beta = R.gn_case("odd pixel count", "fp16")
    big = torch.cat([x[1:], x, x[:1]])
    got, gbig = _gn(dev, "fp16", x, gamma, beta), _gn(dev, "fp16", big, gamma, beta)
    assert torch.equal(gbig[1:3], got) and torch.equal(gbig[0], got[1]) and torch.equal(gbig[3], got[0])


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", list(R.POOL_CASES))
def test_stem_pool(dev, name, prec):
    L = _lib.bit_lib()
    x = R.pool_case(name, prec)
    B, S, _, C = x.shape
    xd = x.to(R.DTYPES[prec]).to(dev).contiguous()
    out = torch.empty(B, S // 2, S // 2, C, dtype=xd.dtype, device=dev)
    _lib.bit_check(L.effocr_bit_op_stem_pool(_lib.PREC[prec], _lib.ptr(xd), B, S, S, C, _lib.ptr(out), _lib.current_stream(dev)),
                   "effocr_bit_op_stem_pool")
    torch.cuda.synchronize(dev)
    got = out.cpu().double()
    assert torch.equal(got, R.stem_pool_ref(x))
    assert not torch.equal(got, R.stem_pool_mutant(x))


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("name", list(R.HEAD_CASES))
def test_head(dev, name, l2, prec):
    L = _lib.bit_lib()
    x, gamma, beta = R.head_case(name, prec)
    B, HW, C = x.shape
    xd = x.to(R.DTYPES[prec]).to(dev).contiguous()
    gd, bd = gamma.float().to(dev), beta.float().to(dev)
    emb = torch.empty(B, C, device=dev)
    status = torch.zeros(64, dtype=torch.int32, device=dev)
    _lib.bit_check(L.effocr_bit_op_head(_lib.PREC[prec], _lib.ptr(xd), B, HW, C, _lib.ptr(gd), _lib.ptr(bd), int(l2), _lib.ptr(emb),
                                        _lib.ptr(status), _lib.current_stream(dev)), "effocr_bit_op_head")
    torch.cuda.synchronize(dev)
    got = emb.cpu().double()
    ref, bound = R.head_ref(x, gamma, beta, l2), R.head_bound(x, gamma, beta, l2)
    w = R.worst(got, ref, bound)
    print(f"head {name} l2={l2} {prec}: worst |err| / bound {w:.3f}")
    assert w <= 1
    assert status[0].item() == 0
    if name == "HW 4" and not l2:                                              # a NaN pixel reaches the status word; the other crop does not
        xd[1, 2, 100] = float("nan")
        _lib.bit_check(L.effocr_bit_op_head(_lib.PREC[prec], _lib.ptr(xd), B, HW, C, _lib.ptr(gd), _lib.ptr(bd), 0, _lib.ptr(emb),
                                            _lib.ptr(status), _lib.current_stream(dev)), "effocr_bit_op_head")
        torch.cuda.synchronize(dev)
        assert status[0].item() == 1 and torch.isfinite(emb[0]).all() and not torch.isfinite(emb[1]).all()
