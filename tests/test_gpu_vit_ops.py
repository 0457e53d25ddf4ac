"""The non-GEMM kernels of the main ViT path on the MI355X (-m gpu), one launch each through the test-only libeffocr_convops.so
(effocr_convops_vit_*): the fused patch embedding (patch.hip), im2col16 + EPI_PATCH (vit_ops.hip; gemm.hip, gemm2.hip), set_cls / gather_cls,
the final class-token norm (vit_ops.hip) and the class-token form of the fused qkv + attention kernel (qkvattn.hip), against the float64
restatements of tests/vit_ops_ref.py.  Integer data must match bit for bit, real data within bounds derived from the arithmetic, pure movement
bit for bit; tests/test_vit_ops_host.py shows on the CPU that each comparison rejects the mutants of its operator.  No tolerance here is
measured; the class-token attention keeps tests/test_gpu_kernels.py::test_qkv_attn_fused_blocked's own.

Every output buffer is pre-filled with NaN (16-bit outputs: with NaN or a sentinel pattern) up to 32 rows past rows_alloc, and every row the
contract does not write must keep it; inputs must come back unchanged; every element the contract writes is compared.  Where a launcher
chooses between kernels the test asserts, from the dispatch the library recorded, the instantiation it meant to run.

Non-finite data: a NaN pixel (fp16: also a pixel of 1e5, which overflows to inf) makes exactly its patch's row non-finite — not the class row,
not a neighbour's — and no other token changes by a bit.  Final norm: a non-finite class row makes its embedding NaN and ORs 1 into the
status word (never stores); with l2 a NaN in beta makes every channel of every embedding NaN, as F.normalize does."""
import functools

import pytest
import torch

from effocr_amd import _lib
from tests import convops_lib as CL
from tests import vit_ops_ref as R
from tests.convops_ref import check_bound, check_exact

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL16 = -12345                                             # int16 fill of the 16-bit buffers that are compared as bit patterns
GUARD = 32                                                      # rows past rows_alloc that must keep the fill


def _call(dev, name, *args):
    rc = getattr(CL.lib(), "effocr_convops_vit_" + name)(*args, _lib.current_stream(dev))
    torch.cuda.synchronize(dev)
    return rc


def _run(dev, name, *args):
    rc = _call(dev, name, *args)
    assert rc == 0, f"rc {rc}: {CL.last_error()}"


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _unchanged(pairs):
    for name, (dev_t, host_t) in pairs.items():
        assert _same_bits(dev_t.cpu(), host_t), f"the input {name} was modified"


@functools.lru_cache(maxsize=1)
def cus():
    n = CL.lib().effocr_convops_device_cus()
    assert n > 0
    return n


# ---------------------------------------------------------------------------------------------------- patch embedding (patch.hip)
def run_patch(dev, d, prec, x16, with_cls, x=None):
    """tokens [B, 1 + P, D] fp32 as the kernel left them (NaN where it wrote nothing) and the recorded (slice width, grid)."""
    dt = R.DTYPE[prec]
    xs = d["x"] if x is None else x
    B, _, H, W = xs.shape
    P, D = d["P"], d["w"].shape[0]
    rows, ra = B * (P + 1), R.up32(B * (P + 1))
    host = dict(x=(xs.to(dt) if x16 else xs).contiguous(), wb=R.to_blocked(d["w"].to(dt), D), bias=d["bias"], pos=d["pos"].contiguous(), cls=d["cls"])
    devt = {k: v.to(dev) for k, v in host.items()}
    out = torch.full(((ra + GUARD) * D,), NAN, device=dev)
    _run(dev, "patch_embed", CL.PREC[prec], CL.ptr(devt["x"]), x16, B, H, W, CL.ptr(devt["wb"]), CL.ptr(devt["bias"]), CL.ptr(devt["pos"]),
         CL.ptr(devt["cls"]) if with_cls else None, CL.ptr(out), D, P)
    disp = CL.patch_last_dispatch()
    _unchanged({k: (devt[k], host[k]) for k in host})
    tok = R.from_blocked(out.cpu(), ra + GUARD, D, ra + GUARD)
    assert bool(tok[rows:].isnan().all()), "a row past batch * tokens was written"
    return tok[:rows].view(B, P + 1, D), disp


@functools.lru_cache(maxsize=2)
def _patch_case(D, H, W, B, prec, kind, order="bias_pos"):
    d = R.patch_data(D, H, W, B, kind)
    return d, R.patch_ref(d, prec, order), (R.patch_bound(d, prec, order) if kind == "real" else None)


def _compare(got, ref, bound, what):
    """Bit equality on integer data (bound None), the derived bound otherwise; returns the largest error / bound."""
    if bound is None:
        check_exact(got, ref, what)
        return 0.0
    return check_bound(got, ref, bound, what)


def patch_case_list():
    return R.patch_cases(256)                                   # names and small shapes; the whole-panel batch is re-derived from the device below


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("case", patch_case_list(), ids=[c[0] for c in patch_case_list()])
def test_patch_embed(dev, case, prec, kind):
    name, D, H, W, B, _ = case
    if name == "whole_panels":
        B = R.whole_panel_batch(cus())
    d, ref, bound = _patch_case(D, H, W, B, prec, kind)
    P = d["P"]
    panels = (B * P + 127) // 128
    dw = R.patch_slice_width(D, B, P, cus())
    assert dw == (384 if name == "whole_panels" or D == 768 else 128 if D == 384 else D), "the case no longer reaches the kernel it names"
    got, worst = {}, 0.0
    for x16 in (0, 1):
        for with_cls in (1, 0):
            tok, disp = run_patch(dev, d, prec, x16, with_cls)
            assert disp == (dw, panels * (D // dw)), f"{name}: ran <{disp[0]}> on a grid of {disp[1]}"
            what = f"patch_embed {name} B={B} {prec} {kind} x16={x16} cls={'given' if with_cls else 'NULL'}"
            if with_cls:
                worst = max(worst, _compare(tok, ref, bound, what))
            else:
                assert bool(tok[:, 0].isnan().all()), f"{what}: a class-token row was written"
                worst = max(worst, _compare(tok[:, 1:], ref[:, 1:], None if bound is None else bound[:, 1:], what))
            got[x16, with_cls] = tok
    assert _same_bits(got[0, 1], got[1, 1]) and _same_bits(got[0, 0][:, 1:], got[1, 0][:, 1:]), "16-bit crops and fp32 crops give different tokens"
    assert _same_bits(got[0, 1][:, 1:], got[0, 0][:, 1:])
    print(f"patch_embed {name} B={B} {prec} {kind}: <{dw}> x {panels * (D // dw)}, error / bound {worst:.3f}")


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_patch_embed_crop_0_is_call_size_invariant(dev, prec):
    """Three 128-wide slices (B = 1) and whole 384-wide panels (the whole-panel batch) do the same arithmetic per output."""
    B = R.whole_panel_batch(cus())
    d, _, _ = _patch_case(384, 32, 32, B, prec, "real")
    big, disp_big = run_patch(dev, d, prec, 0, 1)
    one, disp_one = run_patch(dev, d, prec, 0, 1, x=d["x"][:1])
    assert disp_big[0] == 384 and disp_one == (128, 3)
    assert _same_bits(one[0], big[0]), "crop 0's tokens depend on the call size"
    print(f"patch_embed {prec}: crop 0 of 1 (<128> x 3) == crop 0 of {B} (<384> x {disp_big[1]}) bit for bit")


@pytest.mark.parametrize("x16", [0, 1])
@pytest.mark.parametrize("prec,bad", [("bf16", NAN), ("fp16", NAN), ("fp16", 1e5)])
def test_patch_embed_nonfinite_pixel_stays_in_its_row(dev, prec, bad, x16):
    d, _, _ = _patch_case(384, 32, 48, 5, prec, "real")
    clean, _ = run_patch(dev, d, prec, x16, 1)
    x = d["x"].clone()
    img, ty, tx = 2, 1, 0                                       # patch 3 of image 2: rows 16.., columns 0..
    x[img, 1, ty * 16 + 5, tx * 16 + 9] = bad
    got, _ = run_patch(dev, d, prec, x16, 1, x=x)
    row = got[img, 1 + ty * 3 + tx]
    assert not bool(torch.isfinite(row).any()), "part of the poisoned patch's row is finite"
    keep = torch.ones(got.shape[:2], dtype=torch.bool)
    keep[img, 1 + ty * 3 + tx] = False
    assert bool(torch.isfinite(got[keep]).all()) and _same_bits(got[keep], clean[keep]), "another token changed"


# ---------------------------------------------------------------------------------------------------- im2col16 + EPI_PATCH
@pytest.mark.parametrize("prec,x16", [("fp32", 0), ("bf16", 0), ("fp16", 0), ("bf16", 1), ("fp16", 1)])
@pytest.mark.parametrize("H,W,B", [(32, 48, 5), (224, 224, 1)])
def test_im2col16(dev, H, W, B, prec, x16):
    dt = R.DTYPE[prec]
    x = R.patch_data(128, H, W, B, "real")["x"]
    M = B * (H // 16) * (W // 16)
    host = (x.to(dt) if x16 else x).contiguous()
    xd = host.to(dev)
    col = torch.full((M + 1, R.PATCH_K), NAN, dtype=dt, device=dev)
    _run(dev, "im2col16", CL.PREC[prec], CL.ptr(xd), x16, B, H, W, CL.ptr(col))
    _unchanged({"x": (xd, host)})
    got = col.cpu()
    assert bool(got[M].isnan().all()), "the guard row was written"
    assert _same_bits(got[:M], R.im2col(x).reshape(M, R.PATCH_K).to(dt)), "patch rows differ from the crops' pixels rounded once"


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("blocked", [0, 1])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("P,B", [(4, 1), (196, 3)])
def test_epi_patch(dev, P, B, prec, blocked, kind):
    H = 32 if P == 4 else 224
    D, dt = 384, R.DTYPE[prec]
    d, ref, bound = _patch_case(D, H, H, B, prec, kind, "pos_bias")
    host = dict(col=R.im2col(d["x"]).reshape(B * P, R.PATCH_K).to(dt).contiguous(), w=d["w"].to(dt).contiguous(), bias=d["bias"], pos=d["pos"].contiguous())
    devt = {k: v.to(dev) for k, v in host.items()}
    rows, ra = B * (P + 1), R.up32(B * (P + 1))
    out = torch.full(((ra + GUARD) * D,), NAN, device=dev)
    args = (CL.PREC[prec], CL.ptr(devt["col"]), CL.ptr(devt["w"]), CL.ptr(devt["bias"]), CL.ptr(devt["pos"]), CL.ptr(out), B, P, D, blocked)
    if prec == "fp32" and blocked:                              # gemm.hip writes row-major rows only; vit_forward never asks it for the blocked layout
        assert _call(dev, "patch_gemm", *args) == CL.EUNSUPPORTED and bool(out.isnan().all())
        return
    _run(dev, "patch_gemm", *args)
    _unchanged({k: (devt[k], host[k]) for k in host})
    tok = R.from_blocked(out.cpu(), ra + GUARD, D, ra + GUARD) if blocked else out.cpu().view(ra + GUARD, D)
    assert bool(tok[rows:].isnan().all()), "a row past batch * tokens was written"
    tok = tok[:rows].view(B, P + 1, D)
    assert bool(tok[:, 0].isnan().all()), "a class-token row was written"
    what = f"EPI_PATCH P={P} B={B} {prec} {'blocked' if blocked else 'row-major'} {kind}"
    r = _compare(tok[:, 1:], ref[:, 1:], None if bound is None else bound[:, 1:], what)
    print(f"{what}: error / bound {r:.3f}")


# ---------------------------------------------------------------------------------------------------- set_cls / gather_cls
MOVE_CASES = [(B, T, D) for B in (1, 33, 129) for T in (5, 197) for D in (128, 384, 768)]


@pytest.mark.parametrize("blocked", [0, 1])
@pytest.mark.parametrize("B,T,D", MOVE_CASES)
def test_set_cls(dev, B, T, D, blocked):
    cls = torch.randn(D, generator=torch.Generator().manual_seed(B + T + D))
    cd = cls.to(dev)
    rows, ra = B * T, R.up32(B * T)
    for with_status in (1, 0):
        x = torch.full(((ra + GUARD) * D,), NAN, device=dev)
        status = torch.full((2,), 7, dtype=torch.int32, device=dev)
        _run(dev, "set_cls", CL.ptr(cd), CL.ptr(x), B, T, D, blocked, CL.ptr(status) if with_status else None)
        assert status.tolist() == ([0, 7] if with_status else [7, 7])
        tok = R.from_blocked(x.cpu(), ra + GUARD, D, ra + GUARD) if blocked else x.cpu().view(ra + GUARD, D)
        assert _same_bits(tok[:rows:T], cls.expand(B, D)), "class-token rows differ from cls_pos0"
        rest = torch.ones(ra + GUARD, dtype=torch.bool)
        rest[:rows:T] = False
        assert bool(tok[rest].isnan().all()), "a row other than the class tokens' was written"
    _unchanged({"cls_pos0": (cd, cls)})


@pytest.mark.parametrize("B,T,D", MOVE_CASES)
def test_gather_cls(dev, B, T, D):
    g = torch.Generator().manual_seed(B * 7 + T + D)
    x = torch.randn(B * T, D, generator=g)
    att = torch.randint(-32768, 32767, (B * T, D), generator=g, dtype=torch.int16)          # any 16-bit pattern: the kernel moves 16-byte chunks
    ra, rb = R.up32(B * T), R.up32(B)
    hx, ha = R.to_blocked(x, ra), R.to_blocked(att, ra)
    xd, ad = hx.to(dev), ha.to(dev)
    xc = torch.full(((rb + GUARD) * D,), NAN, device=dev)
    ac = torch.full(((rb + GUARD) * D,), SENTINEL16, dtype=torch.int16, device=dev)
    _run(dev, "gather_cls", CL.ptr(xd), CL.ptr(ad), B, T, D, CL.ptr(xc), CL.ptr(ac))
    _unchanged({"x": (xd, hx), "att": (ad, ha)})
    gx, ga = R.from_blocked(xc.cpu(), rb + GUARD, D, rb + GUARD), R.from_blocked(ac.cpu(), rb + GUARD, D, rb + GUARD)
    wx, wa = R.gather_ref(x, att, T)
    assert _same_bits(gx[:B], wx) and torch.equal(ga[:B], wa), "gathered rows differ from rows img * T"
    assert bool(gx[B:].isnan().all()) and bool((ga[B:] == SENTINEL16).all()), "a row past the batch was written"


# ---------------------------------------------------------------------------------------------------- final norm (cls_norm_kernel)
def run_norm(dev, d, l2, blocked, status0=0, with_status=True, x=None, lnb=None):
    """(emb [B, D], status word): emb has B + 1 rows whose last keeps the NaN fill; only word 0 of the status buffer may change, by OR."""
    xs = d["x"] if x is None else x
    B, T, D = d["B"], d["T"], xs.shape[1]
    hx = R.to_blocked(xs, R.up32(B * T)) if blocked else xs.contiguous()
    hb = d["lnb"] if lnb is None else lnb
    xd, gd, bd = hx.to(dev), d["lnw"].to(dev), hb.to(dev)
    emb = torch.full((B + 1, D), NAN, device=dev)
    status = torch.tensor([status0, 7, 7, 7], dtype=torch.int32, device=dev)
    _run(dev, "final_norm", CL.ptr(xd), B, T, D, CL.ptr(gd), CL.ptr(bd), R.EPS, l2, blocked, CL.ptr(emb), CL.ptr(status) if with_status else None)
    _unchanged({"x": (xd, hx), "gamma": (gd, d["lnw"]), "beta": (bd, hb)})
    e, st = emb.cpu(), status.tolist()
    assert bool(e[B].isnan().all()), "the row past the batch was written"
    assert st[1:] == [7, 7, 7] and (with_status or st[0] == status0)
    return e[:B], st[0]


NORM_CASES = ([(D, T, B, "real") for D in (128, 384, 768) for T in (1, 5, 197) for B in (1, R.NORM_WG_IMAGES[D] + 1)]
              + [(128, 5, 9, "cancel"), (384, 5, 9, "cancel"), (768, 5, 5, "cancel"), (128, 5, 9, "zero"), (384, 197, 9, "zero"), (768, 5, 5, "zero")])


@pytest.mark.parametrize("D,T,B,kind", NORM_CASES)
def test_final_norm(dev, D, T, B, kind):
    d = R.norm_data(D, T, B, kind)
    worst = 0.0
    for l2 in (0, 1):
        ref, bound = R.norm_ref(d, l2), R.norm_bound(d, l2)
        for blocked in (0, 1):
            got, status = run_norm(dev, d, l2, blocked)
            assert status == 0
            if kind == "zero" and l2:
                assert bool((got[0] == 0).all())                # 0 / max(0, 1e-12): the zero vector, not NaN
            worst = max(worst, check_bound(got, ref, bound, f"final_norm D={D} T={T} B={B} {kind} l2={l2} blocked={blocked}"))
    print(f"final_norm D={D} T={T} B={B} {kind}: error / bound {worst:.3f}")


@pytest.mark.parametrize("blocked", [0, 1])
@pytest.mark.parametrize("D,B", [(128, 9), (384, 9), (768, 5)])
def test_final_norm_status(dev, D, B, blocked):
    d = R.norm_data(D, 5, B, "real")
    clean, st = run_norm(dev, d, 1, blocked, status0=4)
    assert st == 4                                              # finite data: nothing is ORed in, nothing is stored
    run_norm(dev, d, 1, blocked, with_status=False)             # NULL status is accepted
    for bad in (NAN, float("inf")):
        x = d["x"].clone()
        x[(B - 1) * 5, 3] = bad                                 # the class row of the last image
        got, st = run_norm(dev, d, 1, blocked, status0=4, x=x)
        assert st == 5, "a non-finite embedding must OR 1 into the status word"
        assert bool(got[B - 1].isnan().all()) and _same_bits(got[:B - 1], clean[:B - 1]), "only the poisoned image's embedding may change"
        x = d["x"].clone()
        x[(B - 1) * 5 + 1, 3] = bad                             # token 1: not a class row
        got, st = run_norm(dev, d, 1, blocked, status0=4, x=x)
        assert st == 4 and _same_bits(got, clean)


@pytest.mark.parametrize("D,B", [(128, 9), (384, 1), (768, 5)])
def test_final_norm_nan_beta_reaches_every_channel(dev, D, B):
    """F.normalize semantics: a NaN norm makes the whole embedding NaN (x / max(NaN, eps) is NaN in torch: clamp_min keeps a NaN)."""
    d = R.norm_data(D, 5, B, "real")
    lnb = d["lnb"].clone()
    lnb[5] = NAN
    want = torch.nn.functional.normalize(torch.nn.functional.layer_norm(d["x"][::5], (D,), d["lnw"], lnb, R.EPS), dim=1)
    assert bool(want.isnan().all())
    got, st = run_norm(dev, d, 1, 1, lnb=lnb)
    assert st == 1
    assert bool(got.isnan().all()), f"{int(torch.isfinite(got).sum())} of {got.numel()} channels are finite behind a NaN norm"
    got, st = run_norm(dev, d, 0, 1, lnb=lnb)                   # without l2 only channel 5 carries the NaN
    assert st == 1 and bool(got[:, 5].isnan().all()) and int(got.isnan().sum()) == B


# ---------------------------------------------------------------------------------------------------- class-token attention (qkvattn.hip)
def run_qkv_attn(dev, d, B, T, D, prec, cls_only):
    dt = R.DTYPE[prec]
    M = B * T
    ra = (M + 127) // 128 * 128
    wv, bv = d["w"].clone(), d["bias"].clone()                  # the kernel's weight copy: v rows (and bias) P32-permuted
    wv[2 * D:], bv[2 * D:] = R.perm32_rows(d["w"][2 * D:]), R.perm32_rows(d["bias"][2 * D:])
    host = dict(xn=R.to_blocked(d["xn"], ra), wb=R.to_blocked(wv, 3 * D), bias=bv)
    devt = {k: v.to(dev) for k, v in host.items()}
    out = torch.full(((ra + GUARD) * D,), NAN, dtype=dt, device=dev)
    _run(dev, "qkv_attn", CL.PREC[prec], CL.ptr(devt["xn"]), CL.ptr(devt["wb"]), CL.ptr(devt["bias"]), CL.ptr(out), B, T, D, ra, cls_only, 0)
    disp = CL.qkv_attn_last_dispatch()
    _unchanged({k: (devt[k], host[k]) for k in host})
    rows = R.from_blocked(out.cpu(), ra + GUARD, D, ra + GUARD)
    assert bool(rows[M:].isnan().all()), "a row past batch * tokens was written"
    return rows[:M], disp


def expected_qkv_dispatch(B, T, cls_only, ncu):
    """launch_qkvattn at D = 384, 7 token tiles: [(D, tiles, cls, P.V steps, head split, grid)] per launch."""
    npv = 13 if T <= 208 else 14
    split = lambda n: next((c for c in (6, 3, 2) if n * c <= ncu), 1)
    if split(B) == 1 and B > ncu and B % ncu and split(B % ncu) > 1:
        tail = B % ncu
        return [(384, 7, cls_only, npv, 1, min(B - tail, ncu)), (384, 7, cls_only, npv, split(tail), tail * split(tail))]
    hs = split(B)
    return [(384, 7, cls_only, npv, hs, B * hs if hs > 1 else min(B, ncu))]


ATTN_AGREE = {}


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("T", [197, 210])
@pytest.mark.parametrize("Bname", ["B1", "B5", "CUs+3"])
def test_class_token_attention(dev, Bname, T, prec):
    D, ncu = 384, cus()
    B = {"B1": 1, "B5": 5, "CUs+3": ncu + 3}[Bname]
    d = R.attn_data(B, T, D, prec)
    got, disp = run_qkv_attn(dev, d, B, T, D, prec, 1)
    assert disp == expected_qkv_dispatch(B, T, 1, ncu), f"ran {disp}"
    if Bname == "B1":
        assert disp[0][4:] == (6, 6)
    if Bname == "CUs+3":
        assert len(disp) == 2 and disp[0][4:] == (1, ncu) and disp[1][4:] == (6, 18)
    ref = R.cls_attn_ref(d, B, T, D, prec)
    cls_rows = got[::T].double()
    assert bool(torch.isfinite(cls_rows).all())
    err, scale = (cls_rows - ref).abs().max().item(), ref.abs().max().item()
    full, disp_all = run_qkv_attn(dev, d, B, T, D, prec, 0)
    assert disp_all == expected_qkv_dispatch(B, T, 0, ncu)
    agree = _same_bits(got[::T], full[::T])
    ATTN_AGREE[Bname, T, prec] = agree
    print(f"class-token attention B={B} T={T} {prec}: {disp}; error / bound {err / (R.ATTN_TOL[prec] * scale):.3f}; "
          f"class rows {'equal' if agree else 'DIFFER from'} the all-token kernel's bit for bit")
    assert err <= R.ATTN_TOL[prec] * scale, f"err {err:.3e} vs scale {scale:.3e}"
    assert agree, "the class-token form and the all-token kernel disagree on row img * T"
