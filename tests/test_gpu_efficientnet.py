"""efficientnet_b0 / tf_efficientnet_b0 on the MI355X (-m gpu), through libeffocr_effnet.so: parity with the float64 CPU restatement
(tests/efficientnet_ref.py, pinned to transformers.EfficientNetModel by tests/test_efficientnet_host.py) in every precision — on the
issue's four shapes and on a checkpoint whose embedding depends on the crop —, bitwise batch / chunk invariance, the stem and the
depthwise + squeeze-excite kernel pair on their own, status word, normalisation, workspace, crop type, the
engines end to end on a 300 x 1280 index built by train_knn, and the classifier head.

Measured on the MI355X (profiles/efficientnet_parity.txt, one run): see DESIGN.md "EfficientNet-B0", accuracy."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from effocr_amd import _lib
from effocr_amd import weights as W
from tests.efficientnet_ref import efficientnet_forward

pytestmark = pytest.mark.gpu

ARCHS = ["efficientnet_b0", "tf_efficientnet_b0"]
# bounds, max norm AND worst-row relative L2 (the project's own): fp32 = the exact mode; fp16 = north_star's 1e-3; bf16 = 1e-2
REL = {"fp32": 1e-5, "fp16": 1e-3, "bf16": 1e-2}
DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}
# img, B, trained-magnitude weights: 32 -> final map 1x1, k = 5 depthwise on 2x2 and 1x1 maps, a stride-2 depthwise on a 2x2 input, one SE
# tile; 96 -> odd maps (3x3 final), tiles that do not divide the map (48, 24); 224 -> the real tile counts (49 at 112^2, 16 at 56^2, 4 at 28^2)
SHAPES = [(32, 5, False), (96, 3, False), (224, 2, False), (64, 4, True)]


def rel_err(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def row_l2_err(got, ref):
    return ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()


@functools.lru_cache(maxsize=None)
def _sd_cached(arch, seed, img, trained):
    if not trained:
        return W.init_state_dict(arch, seed=seed, img_size=img)
    # trained magnitudes, as tests/test_gpu_mobilenetv3_family.py: timm's conv init, BN running variances log-uniform in [0.32, 5], running
    # means N(0, 0.2), gains U(0.5, 1.5), shifts N(0, 0.2), SE biases N(0, 0.5)
    sd = W.init_state_dict(arch, seed=seed, img_size=img, scale="timm")
    g = torch.Generator().manual_seed(seed + 100)
    for k, v in sd.items():
        if k.endswith("running_var"):
            sd[k] = 10 ** (torch.rand(v.shape, generator=g) * 1.2 - 0.5)
        elif k.endswith("running_mean"):
            sd[k] = torch.randn(v.shape, generator=g) * 0.2
        elif v.dim() == 1 and k.endswith(".weight"):
            sd[k] = torch.rand(v.shape, generator=g) + 0.5
        elif v.dim() == 1:
            sd[k] = torch.randn(v.shape, generator=g) * (0.5 if ".se." in k else 0.2)
    return sd


def _sd(arch, seed, img, trained=False):
    return dict(_sd_cached(arch, seed, img, trained))       # (a copy of the dict: the cached tensors themselves are never written)


def _crops(B, img, seed):
    return torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _reference(arch, seed, img, trained, B, xseed, round_pw=None):
    """The float64 restatement, computed once per case and shared by the precisions (read-only)."""
    return efficientnet_forward(arch, _sd_cached(arch, seed, img, trained), _crops(B, img, xseed).double(), round_pw=round_pw).float()


def _engine(arch, sd, img, prec, dev):
    from effocr_amd.encoders import EfficientNetEncoder, make_encoder
    enc = make_encoder(arch, sd, img_size=img, precision=prec, device=dev)
    assert type(enc) is EfficientNetEncoder and enc.crop_dtype == torch.float32 and enc.embed_dim == 1280
    return enc


# ---------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("img,B,trained", SHAPES)
@pytest.mark.parametrize("arch", ARCHS)
def test_parity(dev, arch, prec, img, B, trained):
    """fp32: 1e-5 on both norms, no exception.  16-bit, unit init: the project's 1e-3 / 1e-2.  16-bit, trained magnitudes:
    max(project bound, 1.3 x e_w), e_w from the reference alone — the float64 restatement with ONLY the folded pointwise and head
    weights rounded to the operand type (the cause DESIGN.md identified for mobilenetv3_large_100, with the margin the project uses there)."""
    seed, xseed = 1 + img, 7 + B
    ref = _reference(arch, seed, img, trained, B, xseed)
    enc = _engine(arch, _sd(arch, seed, img, trained), img, prec, dev)
    got = enc.forward(_crops(B, img, xseed).to(dev)).cpu()
    enc.check_status()
    e_max, e_row = rel_err(got, ref), row_l2_err(got, ref)
    b_max = b_row = REL[prec]
    note = ""
    if trained and prec != "fp32":
        rounded = _reference(arch, seed, img, trained, B, xseed, DTYPE[prec])
        w_max, w_row = rel_err(rounded, ref), row_l2_err(rounded, ref)
        b_max, b_row = max(b_max, 1.3 * w_max), max(b_row, 1.3 * w_row)
        note = f"; e_w {w_max:.2e} / {w_row:.2e}, bound {b_max:.2e} / {b_row:.2e}"
    print(f"{arch} {prec} {img}^2 B={B} {'trained' if trained else 'unit'}: max-norm {e_max:.2e}, row L2 {e_row:.2e}{note}")
    assert got.shape == (B, 1280) and ref.abs().max() > 1e-3
    assert e_max <= b_max and e_row <= b_row


# ---------------------------------------------------------------------------------------------------- parity on crop-dependent embeddings
SIGNAL_GAIN = 1.6
SIGNAL_SHAPES = [(32, 5), (64, 3), (96, 2)]


@functools.lru_cache(maxsize=None)
def _signal_sd(arch, img):
    """A checkpoint whose embedding depends on the crop.  Under init_state_dict's "unit" rule (and the trained-magnitude one) sixteen
    SiLU + squeeze-excite blocks damp the input's share of the embedding to 1e-6 of its norm, so the cases above cannot see a stem that
    ignores its input or a transposed depthwise kernel.  With every convolution but the squeeze-excite ones 1.6 x larger the input's
    share neither dies nor explodes: in the float64 restatement all-zero crops move these embeddings by 0.6 - 1.0 of their norm and
    transposed crops by 0.3 - 0.7 (both checked below), while a float32 run of the restatement stays 1e-6 - 3.3e-6 from float64."""
    sd = W.init_state_dict(arch, seed=7, img_size=img)
    return {k: (v * SIGNAL_GAIN if v.dim() == 4 and ".se." not in k else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _signal_reference(arch, img, B, round_pw=None):
    x = _crops(B, img, 5).double()
    with torch.no_grad():
        ref = efficientnet_forward(arch, _signal_sd(arch, img), x, round_pw=round_pw)
        if round_pw is not None:
            return ref.float()
        zero = efficientnet_forward(arch, _signal_sd(arch, img), torch.zeros_like(x))
        transposed = efficientnet_forward(arch, _signal_sd(arch, img), x.transpose(2, 3))
    return ref.float(), rel_err(zero, ref), rel_err(transposed, ref)


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("img,B", SIGNAL_SHAPES)
@pytest.mark.parametrize("arch", ARCHS)
def test_parity_on_crop_dependent_embeddings(dev, arch, prec, img, B):
    """The whole network against the float64 restatement where the embedding depends on the crop (_signal_sd): the case that sees the
    stem, the spatial order of every depthwise kernel, padding and the residual path at once.  fp32: the project's 1e-5 on both norms.
    16-bit: max(project bound, 1.3 x e_w), e_w from the reference alone (only the folded pointwise and head weights rounded), as for
    the trained-magnitude case — this checkpoint does not damp a weight's rounding error either."""
    ref, d_zero, d_transposed = _signal_reference(arch, img, B)
    assert d_zero > 0.1 and d_transposed > 0.1                 # the reference itself depends on the crop and on its orientation
    enc = _engine(arch, dict(_signal_sd(arch, img)), img, prec, dev)
    got = enc.forward(_crops(B, img, 5).to(dev)).cpu()
    enc.check_status()
    e_max, e_row = rel_err(got, ref), row_l2_err(got, ref)
    b_max = b_row = REL[prec]
    note = ""
    if prec != "fp32":
        rounded = _signal_reference(arch, img, B, DTYPE[prec])
        w_max, w_row = rel_err(rounded, ref), row_l2_err(rounded, ref)
        b_max, b_row = max(b_max, 1.3 * w_max), max(b_row, 1.3 * w_row)
        note = f"; e_w {w_max:.2e} / {w_row:.2e}, bound {b_max:.2e} / {b_row:.2e}"
    print(f"{arch} {prec} {img}^2 B={B} gain {SIGNAL_GAIN} (zero crops move the reference by {d_zero:.2f}, transposed by {d_transposed:.2f}): "
          f"max-norm {e_max:.2e}, row L2 {e_row:.2e}{note}")
    assert e_max <= b_max and e_row <= b_row


# ---------------------------------------------------------------------------------------------------- the stem on its own
@pytest.mark.parametrize("padb", [0, 1])
@pytest.mark.parametrize("S,B", [(10, 2), (64, 3)])
def test_stem_against_conv2d(dev, S, B, padb):
    """ef_stem through its test entry point against F.conv2d in float64: pad-before 1 (symmetric) and 0 (TensorFlow SAME: 0 before, 1
    after), a map that is mostly border and one of several workgroups.  Asymmetric weights and crops: a swapped axis or channel shows."""
    L = _lib.effnet_lib()
    g = torch.Generator().manual_seed(S + padb)
    x = torch.randn(B, 3, S, S, generator=g)
    w = torch.randn(32, 3, 3, 3, generator=g) / 27 ** 0.5
    b = torch.randn(32, generator=g) * 0.3
    x_d, b_d = x.to(dev), b.to(dev)
    w_d = w.reshape(32, 27).T.contiguous().to(dev)             # [(ci, ky, kx)][32]
    out = torch.full((B, S // 2, S // 2, 32), float("nan"), device=dev)
    rc = L.effocr_effnet_op_stem(_lib.ptr(x_d), B, S, padb, _lib.ptr(w_d), _lib.ptr(b_d), _lib.ptr(out), _lib.current_stream(dev))
    assert rc == 0, L.effocr_effnet_last_error()
    torch.cuda.synchronize(dev)
    xp = F.pad(x.double(), (padb, 2 - padb, padb, 2 - padb))
    want = _silu64(F.conv2d(xp, w.double(), b.double(), stride=2))[:, :, : S // 2, : S // 2].permute(0, 2, 3, 1)
    e = rel_err(out.cpu().double(), want)
    print(f"ef_stem {S}^2 B={B} pad-before {padb}: {e:.2e}")
    assert e <= 1e-5
    other = _silu64(F.conv2d(F.pad(x.double(), (1 - padb, 1 + padb, 1 - padb, 1 + padb)), w.double(), b.double(), stride=2))
    assert rel_err(other[:, :, : S // 2, : S // 2].permute(0, 2, 3, 1), want) > 1e-2       # (the two paddings are told apart)
    assert L.effocr_effnet_op_stem(_lib.ptr(x_d), B, S, 2, _lib.ptr(w_d), _lib.ptr(b_d), _lib.ptr(out), _lib.current_stream(dev)) == -2


# ---------------------------------------------------------------------------------------------------- bitwise invariance
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_batch_and_chunk_invariance(dev, prec):
    arch, img = "efficientnet_b0", 64
    enc = _engine(arch, _sd(arch, 2, img), img, prec, dev)
    x7 = _crops(7, img, 21).to(dev)
    base = enc.forward(x7)
    assert torch.equal(enc.forward(x7[3:4]), base[3:4])                        # a call of 1 crop
    big = _crops(64, img, 164).to(dev)                                         # ... and of 64, the seven scattered among them
    pos = torch.randperm(64, generator=torch.Generator().manual_seed(64))[:7].to(dev)
    big[pos] = x7
    out64 = enc.forward(big)
    assert torch.equal(out64[pos], base)
    for chunk in (1, 3, 0):
        enc.set_chunk(chunk)
        assert torch.equal(enc.forward(x7), base), chunk
        assert torch.equal(enc.forward(big), out64), chunk
    enc.check_status()


# ---------------------------------------------------------------------------------------------------- the SE pair on its own
def _silu64(t):
    return t * torch.sigmoid(t)


@pytest.mark.parametrize("C,H,k,stride,padb,R,B", [
    (32, 16, 3, 1, 1, 8, 3),          # C = 32 on 16x16: exactly one tile
    (1152, 2, 5, 2, 2, 48, 3),        # C = 1152 on 1x1: k = 5 over a 2x2 input, every tap but four outside the map
    (1152, 1, 5, 1, 2, 48, 2),        # ... and a 1x1 input
    (96, 56, 3, 2, 0, 4, 2),          # 28x28 out: 2 x 2 tiles, the edge tiles 12 wide; SAME padding (0 before)
    (240, 17, 5, 1, 2, 10, 2),        # 17x17: edge tiles one pixel wide
    (144, 40, 5, 2, 1, 6, 1),         # 20x20 out, SAME padding for k = 5 (1 before, 2 after)
])
def test_depthwise_tile_sums_and_gate(dev, C, H, k, stride, padb, R, B):
    """The gate computed from the depthwise kernel's per-tile channel sums equals the gate computed from a plain ordered mean of the same
    depthwise output (float64 on the CPU) within 1e-6 relative: a wrong tile count or a dropped edge tile shows here.  The depthwise
    output itself is checked against F.conv2d."""
    L = _lib.effnet_lib()
    g = torch.Generator().manual_seed(C + H)
    Ho = (H - 1) // stride + 1
    NT = L.effocr_effnet_op_tiles(Ho)
    assert NT == ((Ho + 15) // 16) ** 2
    x = torch.randn(B, H, H, C, generator=g)
    dw_w = torch.randn(C, k, k, generator=g) / k
    dw_b = torch.randn(C, generator=g) * 0.3
    wr = torch.randn(R, C, generator=g) / C ** 0.5
    br = torch.randn(R, generator=g) * 0.3
    we = torch.randn(C, R, generator=g) / R ** 0.5
    be = torch.randn(C, generator=g) * 0.3
    d = lambda t: t.contiguous().to(dev)
    x_d, w_d, b_d = d(x), d(dw_w.reshape(C, k * k).T), d(dw_b)                   # taps major
    wr_d, br_d, wet_d, be_d = d(wr), d(br), d(we.T), d(be)
    out = torch.empty(B, Ho, Ho, C, device=dev)
    part = torch.full((B, NT, C), float("nan"), device=dev)
    gate = torch.empty(B, C, device=dev)
    rc = L.effocr_effnet_op_dw_se(_lib.ptr(x_d), B, H, C, k, stride, padb, _lib.ptr(w_d), _lib.ptr(b_d), R, _lib.ptr(wr_d), _lib.ptr(br_d),
                                  _lib.ptr(wet_d), _lib.ptr(be_d), _lib.ptr(out), _lib.ptr(part), _lib.ptr(gate), _lib.current_stream(dev))
    assert rc == 0, L.effocr_effnet_last_error()
    torch.cuda.synchronize(dev)
    out, part, gate = out.cpu().double(), part.cpu().double(), gate.cpu().double()
    # the depthwise output: pad `padb` before and whatever the window needs after
    after = max((Ho - 1) * stride + k - padb - H, 0)
    xp = F.pad(x.double().permute(0, 3, 1, 2), (padb, after, padb, after))
    want = _silu64(F.conv2d(xp, dw_w.double()[:, None], dw_b.double(), stride=stride, groups=C)).permute(0, 2, 3, 1)
    assert want.shape == out.shape
    assert rel_err(out, want) <= 1e-5
    # the tile sums: every tile, edge tiles included, in tile order ty * ntx + tx
    ntx = (Ho + 15) // 16
    tiles = torch.stack([out[:, 16 * (t // ntx):16 * (t // ntx) + 16, 16 * (t % ntx):16 * (t % ntx) + 16].sum((1, 2)) for t in range(NT)], 1)
    assert torch.isfinite(part).all()
    assert rel_err(part, tiles) <= 1e-6
    # the gate, from a plain mean of the same depthwise output
    mean = out.reshape(B, Ho * Ho, C).mean(1)
    gate_ref = torch.sigmoid(_silu64(mean @ wr.double().T + br.double()) @ we.double().T + be.double())
    e = rel_err(gate, gate_ref)
    print(f"C={C} {H}x{H} -> {Ho}x{Ho} k={k} s={stride} padb={padb}: {NT} tiles, gate vs plain mean {e:.2e}")
    assert e <= 1e-6


# ---------------------------------------------------------------------------------------------------- normalise, status, workspace, crops
@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_l2_normalize_fused(dev, prec):
    arch = "tf_efficientnet_b0"
    enc = _engine(arch, _sd(arch, 4, 64), 64, prec, dev)
    x = _crops(6, 64, 3).to(dev)
    raw = enc.forward(x)
    nrm = enc.forward(x, normalize=True)
    assert (nrm - F.normalize(raw, dim=1)).abs().max().item() <= 1e-6
    assert (nrm.norm(dim=1) - 1).abs().max().item() <= 1e-6
    enc.check_status()


@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_status_reports_nonfinite_weight(dev, prec):
    arch = "efficientnet_b0"
    sd = _sd(arch, 5, 64)
    x = _crops(4, 64, 8).to(dev)
    enc = _engine(arch, sd, 64, prec, dev)
    enc.forward(x)
    enc.check_status()                                     # clean weights: OK
    bad = dict(sd)
    bad["bn2.bias"] = sd["bn2.bias"].clone()
    bad["bn2.bias"][17] = float("inf")                     # (data, not a fault: SiLU(inf) = inf in one embedding column)
    enc_bad = _engine(arch, bad, 64, prec, dev)
    enc_bad.forward(x)
    enc_bad.forward(x[:1])
    with pytest.raises(_lib.EffOCRHipError, match="code -6"):
        enc_bad.check_status()                             # sticky: reported once for both forwards ...
    enc_bad.check_status()                                 # ... and read-and-clear: the word is clear again
    enc_bad.forward(x)
    enc_bad.reset_status()                                 # cleared without being read
    enc_bad.check_status()
    enc.forward(x)
    enc.check_status()                                     # the next clean forward is OK


@functools.lru_cache(maxsize=None)
def _nonfinite_reference(arch, bad):
    """Four 64^2 crops with one non-finite pixel in crop 2, through the float64 restatement on the signal checkpoint: row 2 is NaN in
    every column, the other rows are those of the clean crops bit for bit."""
    x = _crops(4, 64, 8)
    xb = x.clone()
    xb[2, 1, 29, 41] = bad
    sd = _signal_sd(arch, 64)
    clean, ref = efficientnet_forward(arch, sd, x.double()), efficientnet_forward(arch, sd, xb.double())
    assert bool(ref[2].isnan().all()) and torch.equal(ref[[0, 1, 3]], clean[[0, 1, 3]]) and bool(torch.isfinite(clean).all())
    return x, xb


@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("arch", ARCHS)
def test_status_reports_nonfinite_input(dev, arch, prec):
    """A NaN pixel, then an inf pixel, in crop 2 of 4 (data, not a fault): check_status raises code -6, row 2 of the embedding is NaN in
    every column as the restatement's, rows 0, 1 and 3 are bit-equal to the clean forward, and the word then reads clear — with and
    without the fused normalisation (mg_finish, shared with the MobileNetV3 library)."""
    enc = _engine(arch, dict(_signal_sd(arch, 64)), 64, prec, dev)
    for bad in (float("nan"), float("inf")):
        x, xb = _nonfinite_reference(arch, bad)
        for normalize in (False, True):
            clean = enc.forward(x.to(dev), normalize=normalize)
            enc.check_status()
            got = enc.forward(xb.to(dev), normalize=normalize)
            with pytest.raises(_lib.EffOCRHipError, match="code -6"):
                enc.check_status()
            enc.check_status()                                 # read-and-clear: the word is clear again
            nan_cols = int(got[2].isnan().sum().item())
            assert nan_cols == got.shape[1], f"{arch} {prec} {bad} normalize={normalize}: row 2 has {nan_cols} NaN columns of {got.shape[1]}"
            assert torch.equal(got[[0, 1, 3]], clean[[0, 1, 3]])


def test_workspace_too_small_and_16bit_crops_are_refused(dev):
    arch = "efficientnet_b0"
    enc = _engine(arch, _sd(arch, 6, 64), 64, "fp16", dev)
    L = enc._L
    B = 3
    need = enc.workspace_bytes(B)
    x = _crops(B, 64, 1).to(dev)
    emb = torch.full((B, 1280), 7.0, device=dev)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    s = _lib.current_stream(dev)
    fp32 = _lib.PREC["fp32"]
    # refused on the host, before any launch: nothing is written
    assert L.effocr_effnet_forward(enc._h, _lib.ptr(x), fp32, B, _lib.ptr(emb), 0, _lib.ptr(ws), need - 1, s) == -3
    for p in ("fp16", "bf16"):
        assert L.effocr_effnet_forward(enc._h, _lib.ptr(x), _lib.PREC[p], B, _lib.ptr(emb), 0, _lib.ptr(ws), need, s) == -2
    torch.cuda.synchronize(dev)
    assert torch.equal(emb, torch.full_like(emb, 7.0)) and not ws.any()
    assert L.effocr_effnet_forward(enc._h, _lib.ptr(x), fp32, B, _lib.ptr(emb), 0, _lib.ptr(ws), need, s) == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(emb, enc.forward(x))
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match="float32"):
            enc.forward(x.to(dt))


# ---------------------------------------------------------------------------------------------------- end to end
E2E = dict(arch="tf_efficientnet_b0", img=32, n=12, rows=300, seed=7, gain=1.7)


@functools.lru_cache(maxsize=None)
def _e2e_sd():
    """A checkpoint whose embeddings depend on the crop.  Under init_state_dict's "unit" rule (and the trained-magnitude one) sixteen
    SiLU + squeeze-excite blocks damp the input's share of the embedding to 1e-6 of its norm: every crop then has the same nearest
    neighbour.  Convolutions 1.7 x larger sit at the edge where that share neither dies nor explodes (measured on the CPU: the
    embeddings of random crops spread by half their norm)."""
    sd = W.init_state_dict(E2E["arch"], seed=E2E["seed"], img_size=E2E["img"])
    return {k: (v * E2E["gain"] if v.dim() == 4 and ".se." not in k else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _e2e_fixture():
    """300 "renders" (the index) of which the first 12 resemble the 12 query crops; the float64 restatement's exact top-1 ids, its top-1
    margin (best score minus runner-up) and the safety margin of the 16-bit mode, computed once on the CPU."""
    arch, img, n, rows = E2E["arch"], E2E["img"], E2E["n"], E2E["rows"]
    sd = _e2e_sd()
    g = torch.Generator().manual_seed(22)
    crops = torch.randn(n, 3, img, img, generator=g)
    renders = torch.randn(rows, 3, img, img, generator=g)
    renders[:n] = crops + 0.05 * torch.randn(n, 3, img, img, generator=g)
    with torch.no_grad():
        index = F.normalize(efficientnet_forward(arch, sd, renders.double()), dim=1)
        q = efficientnet_forward(arch, sd, crops.double())
        q16 = efficientnet_forward(arch, sd, crops.double(), round_pw=torch.float16)
    top2 = (F.normalize(q, dim=1) @ index.T).topk(2, dim=1)
    e_w = row_l2_err(q16, q)
    # An embedding error of e in row L2 moves a cosine between two unit rows by at most 2 e + e^2 (both rows move), a score DIFFERENCE by
    # twice that: 4.1 e.  e is the mode's bound, or 1.3 x what rounding the pointwise weights alone does to this checkpoint if that is more.
    safety = {"fp32": 4.1 * REL["fp32"], "fp16": 4.1 * max(REL["fp16"], 1.3 * e_w)}
    return crops, renders, top2.indices[:, 0], (top2.values[:, 0] - top2.values[:, 1]).min().item(), safety


def test_e2e_fixture_margin_on_the_cpu():
    """(No GPU work: the margin the end-to-end test relies on.)"""
    _, _, want, margin, safety = _e2e_fixture()
    print(f"end-to-end fixture: top-1 margin {margin:.3e}, safety margins {safety}")
    assert torch.equal(want, torch.arange(E2E["n"]))           # every crop finds its own render
    assert margin > safety["fp16"] > safety["fp32"]


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_end_to_end_engines(dev, prec, tmp_path):
    from effocr_amd.encoders import AutoEncoderFactory
    from effocr_amd.knn import FaissKNN, IndexFlatIP, InferenceModel
    from effocr_amd.pipeline import Recognizer
    from effocr_amd.recognizer_engine import EffRecognizer
    arch, img, n, rows = E2E["arch"], E2E["img"], E2E["n"], E2E["rows"]
    crops, renders, want, margin, safety = _e2e_fixture()
    assert margin > safety[prec]
    sd = _e2e_sd()
    ckpt = tmp_path / "enc_best.pth"
    W.save_checkpoint(sd, ckpt)
    chars = [chr(0x4E00 + i) for i in range(rows)]

    enc = AutoEncoderFactory("timm", arch, precision=prec, img_size=img).load(str(ckpt))
    enc.to(dev).eval()
    knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
    InferenceModel(enc, knn_func=knn).train_knn(renders, batch_size=64)
    assert knn.index.ntotal == rows and knn.index.d == 1280
    rec = Recognizer(enc, knn, chars, knn=10)
    _, idx = rec.neighbors(crops.to(dev))
    assert torch.equal(idx[:, 0].cpu(), want)
    _, _, text = rec(crops.to(dev))
    assert text == "".join(chars[i] for i in want.tolist())
    enc.check_status()

    # the checkpoint cannot say "tf_": without arch= it is read as efficientnet_b0, with it as the variant it is
    assert EffRecognizer(str(ckpt), precision=prec, img_size=img, device=dev).arch == "efficientnet_b0"
    er = EffRecognizer(str(ckpt), arch=arch, precision=prec, img_size=img, device=dev)
    assert er.arch == arch and er.crop_dtype == torch.float32
    emb = er.run(crops.numpy())[0]
    assert emb.shape == (n, 1280) and emb.dtype == np.float32
    index_rows = F.normalize(torch.cat([enc.engine.forward(renders[i:i + 64].to(dev)) for i in range(0, rows, 64)]), dim=1).cpu()
    top1 = (F.normalize(torch.from_numpy(emb), dim=1) @ index_rows.T).argmax(dim=1)
    assert torch.equal(top1, want)


def test_classifier_logits(dev):
    from effocr_amd.classifiers import AutoClassifierFactory
    arch, img, n_classes, B = "efficientnet_b0", 64, 7, 5
    sd = _sd(arch, 8, img, trained=True)
    sd.update(W.init_head(arch, n_classes, seed=8))
    x = _crops(B, img, 13)
    feat = efficientnet_forward(arch, sd, x.double())
    ref = (feat @ sd["classifier.weight"].double().T + sd["classifier.bias"].double()).float()
    clf = AutoClassifierFactory("timm", arch, n_classes=n_classes, precision="fp32", img_size=img)()
    clf.load_state_dict(sd)
    clf.to(dev).eval()
    got = clf(x.to(dev)).cpu()
    assert got.shape == (B, n_classes)
    e = rel_err(got, ref)
    print(f"{arch} classifier logits fp32 vs float64 restatement: {e:.2e}")
    assert e <= 1e-4
    assert torch.equal(clf.predict(x.to(dev)).cpu(), got.argmax(-1))
    assert torch.equal(got.argmax(-1), ref.argmax(-1))
