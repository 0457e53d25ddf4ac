"""mobilenetv3_small_050 on the MI355X (-m gpu): parity with the float64 CPU restatement (tests/mobilenetv3_ref.py, checked against a
second restatement by tests/test_mobilenetv3_host.py) in every precision, parity on a checkpoint whose embedding depends on the crop (through both libraries that run this network), bitwise
batch / chunk invariance, status word (non-finite weights and non-finite crops),
normalisation, workspace, the engines end to end on a planted-glyph 1024-d index, and the k-NN at d = 1024 against the C oracle."""

import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from effocr_amd import _lib
from effocr_amd import weights as W
from oracle import knn_ref
from tests import mobilenetv3_family_ref as MR
from tests.mobilenetv3_ref import mobilenetv3_forward

pytestmark = pytest.mark.gpu

ARCH = "mobilenetv3_small_050"
D = 1024
# bounds, max norm AND worst-row relative L2: fp32 = the exact mode; fp16 = north_star's 1e-3; bf16 = 1e-2
REL = {"fp32": 1e-5, "fp16": 1e-3, "bf16": 1e-2}
DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}
LIBS = ["merged", "mnv3"]                                   # libeffocr_hip.so's LDS-resident kernels; libeffocr_mnv3.so's forward
# the one exception: fp16 max norm at 64^2 with trained-magnitude weights measured 1.14e-3 (row L2 7.7e-4).  The error is the fp16
# rounding of the folded pointwise weights (the activations enter the MFMAs as hi + lo parts); a 2 x 2 final map averages little of it
# away in the pool.  Bound 1.5e-3 (DESIGN.md "MobileNetV3-Small", precision)
REL_64_TRAINED_FP16_MAX = 1.5e-3


def rel_err(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def row_l2_err(got, ref):
    return ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()


def _sd(seed, img, trained=False):
    if not trained:
        return W.init_state_dict(ARCH, seed=seed, img_size=img)
    # trained magnitudes: timm's conv init, BN running variances log-uniform in [0.32, 5], running means N(0, 0.2), gains U(0.5, 1.5),
    # shifts N(0, 0.2), SE biases N(0, 0.5) (activations peak near 50 at 224^2; wider variance ranges compound over the 11 blocks)
    sd = W.init_state_dict(ARCH, seed=seed, img_size=img, scale="timm")
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


def _crops(B, img, seed):
    return torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(seed))


def _engine(sd, img, prec, dev, lib="merged"):
    from effocr_amd.encoders import HipEncoder, MobileNetV3Encoder
    return (HipEncoder if lib == "merged" else MobileNetV3Encoder)(ARCH, sd, img_size=img, precision=prec, device=dev)


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("img,B,trained", [(224, 3, False), (96, 5, False), (224, 3, True), (64, 4, True)])
def test_parity(dev, prec, img, B, trained):
    sd = _sd(1 + img, img, trained)
    x = _crops(B, img, 7 + B)
    ref = mobilenetv3_forward(ARCH, sd, x.double()).float()
    enc = _engine(sd, img, prec, dev)
    got = enc.forward(x.to(dev)).cpu()
    enc.check_status()
    e_max, e_row = rel_err(got, ref), row_l2_err(got, ref)
    print(f"mobilenetv3 {prec} {img}^2 B={B} {'trained' if trained else 'unit'}: max-norm {e_max:.2e}, row L2 {e_row:.2e}")
    bound_max = REL_64_TRAINED_FP16_MAX if (img, trained, prec) == (64, True, "fp16") else REL[prec]
    assert e_max <= bound_max and e_row <= REL[prec]


# ---------------------------------------------------------------------------------------------------- parity on crop-dependent embeddings
def _signal_sd(img, arch=ARCH):
    """A checkpoint whose embedding depends on the crop (tests/mobilenetv3_family_ref.py: init_state_dict(arch, seed=7) with every 4-d
    weight outside the squeeze-excite layers multiplied by 1.6).  On the "unit" checkpoints above the crop's share of the
    embedding is 6e-4 - 6e-3 at most, at or under the 16-bit bounds: those cases pass with a stem that ignores its input."""
    return dict(MR.signal_sd(arch, img))


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("img", MR.SIGNAL_IMGS)
@pytest.mark.parametrize("lib", LIBS)
def test_parity_on_crop_dependent_embeddings(dev, lib, prec, img):
    """The whole network against the float64 restatement where the embedding depends on the crop: the case that sees the stem, the
    spatial order of every depthwise kernel, padding and the residual path at once, through both libraries that run this network.  fp32: the project's 1e-5 on both norms.  16-bit:
    max(project bound, 1.3 x e_w), e_w from the reference alone (only the folded pointwise and head weights rounded) — this checkpoint
    does not damp a weight's rounding error either."""
    arch = ARCH
    ref, d_zero, d_transposed = MR.signal_reference(arch, img)
    assert d_zero > 0.1 and d_transposed > 0.1                 # the reference itself depends on the crop and on its orientation
    enc = _engine(_signal_sd(img), img, prec, dev, lib)
    got = enc.forward(MR.signal_crops(img).to(dev)).cpu()
    enc.check_status()
    e_max, e_row = rel_err(got, ref), row_l2_err(got, ref)
    b_max = b_row = REL[prec]
    note = ""
    if prec != "fp32":
        rounded = MR.signal_reference(arch, img, DTYPE[prec])
        w_max, w_row = rel_err(rounded, ref), row_l2_err(rounded, ref)
        b_max, b_row = max(b_max, 1.3 * w_max), max(b_row, 1.3 * w_row)
        note = f"; e_w {w_max:.2e} / {w_row:.2e}, bound {b_max:.2e} / {b_row:.2e}"
    print(f"{arch} ({lib}) {prec} {img}^2 B={MR.SIGNAL_B} gain {MR.SIGNAL_GAIN[arch]} (zero crops move the reference by {d_zero:.2f}, transposed by "
          f"{d_transposed:.2f}): max-norm {e_max:.2e}, row L2 {e_row:.2e}{note}")
    assert e_max <= b_max and e_row <= b_row


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_batch_and_chunk_invariance(dev, prec):
    img = 224
    # one case on the checkpoint whose embedding depends on the crop (at 224^2 zero crops move it by 0.98, transposed ones by 0.19:
    # tests/test_mobilenetv3_family_host.py); on the unit checkpoint a crop that landed in the wrong row could go unseen in 16 bits
    sd = _signal_sd(img) if prec == "fp16" else _sd(2, img)
    enc = _engine(sd, img, prec, dev)
    x7 = _crops(7, img, 21).to(dev)
    base = enc.forward(x7)
    singles = torch.cat([enc.forward(x7[i:i + 1]) for i in range(7)])
    assert torch.equal(singles, base)
    for n in (64, 300, 1024):
        big = _crops(n, img, 100 + n).to(dev)
        pos = torch.randperm(n, generator=torch.Generator().manual_seed(n))[:7].to(dev)
        big[pos] = x7
        assert torch.equal(enc.forward(big)[pos], base), n
    for chunk in (0, 5, 100, 1):
        enc.set_chunk(chunk)
        assert torch.equal(enc.forward(x7), base), chunk
        big = torch.cat([_crops(29, img, 5).to(dev), x7])
        assert torch.equal(enc.forward(big)[29:], base), chunk
    enc.check_status()


@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_l2_normalize_fused(dev, prec):
    sd = _sd(4, 64)
    enc = _engine(sd, 64, prec, dev)
    x = _crops(6, 64, 3).to(dev)
    raw = enc.forward(x)
    nrm = enc.forward(x, normalize=True)
    torch.testing.assert_close(nrm, F.normalize(raw, dim=1), rtol=0, atol=2e-7)
    enc.check_status()


@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_status_reports_nonfinite_weight(dev, prec):
    sd = _sd(5, 64)
    x = _crops(4, 64, 8).to(dev)
    enc = _engine(sd, 64, prec, dev)
    enc.forward(x)
    enc.check_status()                                     # clean weights: OK
    bad = dict(sd)
    bad["conv_head.bias"] = sd["conv_head.bias"].clone()
    bad["conv_head.bias"][17] = float("inf")
    enc_bad = _engine(bad, 64, prec, dev)
    enc_bad.forward(x)
    with pytest.raises(_lib.EffOCRHipError, match="code -6"):
        enc_bad.check_status()
    enc_bad.check_status()                                 # read-and-clear: the word is clear again
    enc.forward(x)
    enc.check_status()                                     # the next clean forward is OK


@functools.lru_cache(maxsize=None)
def _nonfinite_reference(arch, bad):
    """Four 64^2 crops with one non-finite pixel in crop 2, through the float64 restatement on the signal checkpoint: row 2 is NaN in
    every column, the other rows are those of the clean crops bit for bit."""
    x = _crops(4, 64, 8)
    xb = x.clone()
    xb[2, 1, 29, 41] = bad
    sd = MR.signal_sd(arch, 64)
    clean, ref = MR.mobilenetv3_family_forward(arch, sd, x.double()), MR.mobilenetv3_family_forward(arch, sd, xb.double())
    assert bool(ref[2].isnan().all()) and torch.equal(ref[[0, 1, 3]], clean[[0, 1, 3]]) and bool(torch.isfinite(clean).all())
    return x, xb


@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("lib", LIBS)
def test_status_reports_nonfinite_input(dev, lib, prec):
    """A NaN pixel, then an inf pixel, in crop 2 of 4 (data, not a fault): check_status raises code -6, row 2 of the embedding is NaN in
    every column as the restatement's, rows 0, 1 and 3 are bit-equal to the clean forward, and the word then reads clear — with and
    without the fused normalisation, through both libraries that run this network."""
    arch = ARCH
    enc = _engine(_signal_sd(64), 64, prec, dev, lib)
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
            assert nan_cols == got.shape[1], f"{arch} ({lib}) {prec} {bad} normalize={normalize}: row 2 has {nan_cols} NaN columns of {got.shape[1]}"
            assert torch.equal(got[[0, 1, 3]], clean[[0, 1, 3]])


def test_workspace_too_small_is_refused(dev):
    sd = _sd(6, 64)
    enc = _engine(sd, 64, "fp16", dev)
    L = enc._L
    B = 3
    need = enc.workspace_bytes(B)
    x = _crops(B, 64, 1).to(dev)
    emb = torch.empty(B, D, device=dev)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    s = _lib.current_stream(dev)
    assert L.effocr_encoder_forward(enc._h, _lib.ptr(x), B, _lib.ptr(emb), 0, _lib.ptr(ws), need - 1, s) == -3
    assert L.effocr_encoder_forward(enc._h, _lib.ptr(x), B, _lib.ptr(emb), 0, _lib.ptr(ws), need, s) == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(emb, enc.forward(x))
    x16 = x.half()                                         # 16-bit crops are a ViT-only hand-off
    assert L.effocr_encoder_forward_ex(enc._h, _lib.ptr(x16), 1, B, _lib.ptr(emb), 0, _lib.ptr(ws), need, s) == -2


def _planted_index(ref_emb, n_distract, seed):
    g = torch.Generator().manual_seed(seed)
    dis = F.normalize(torch.randn(n_distract, D, generator=g), dim=1)
    glyph = F.normalize(ref_emb, dim=1)
    return torch.cat([dis[: n_distract // 2], glyph, dis[n_distract // 2:]])


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_end_to_end_engines(dev, prec, tmp_path):
    from effocr_amd.encoders import AutoEncoderFactory
    from effocr_amd.knn import FaissKNN, IndexFlatIP
    from effocr_amd.pipeline import Recognizer
    from effocr_amd.recognizer_engine import EffRecognizer
    img, n = 224, 12
    sd = _sd(7, img, trained=True)      # (the "unit" init's embeddings barely depend on the crop: std over crops ~1e-3 of their mean)
    ckpt = tmp_path / "enc_best.pth"
    W.save_checkpoint(sd, ckpt)
    glyphs = _crops(n, img, 31)
    ref = mobilenetv3_forward(ARCH, sd, glyphs.double()).float()
    index = _planted_index(ref, 500, 9)
    chars = [chr(0x4E00 + i) for i in range(index.shape[0])]
    q = glyphs + 0.05 * _crops(n, img, 32)
    q_ref = F.normalize(mobilenetv3_forward(ARCH, sd, q.double()).float(), dim=1)
    want = torch.from_numpy(np.argmax(q_ref.numpy() @ index.numpy().T, axis=1))        # exact numpy search
    assert torch.equal(want, torch.arange(n) + 250)

    enc = AutoEncoderFactory("timm", ARCH, precision=prec, img_size=img).load(str(ckpt))
    enc.to(dev).eval()
    knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
    knn.train(index)
    rec = Recognizer(enc, knn, chars, knn=10)
    _, idx = rec.neighbors(q.to(dev))
    assert torch.equal(idx[:, 0].cpu(), want)
    _, _, text = rec(q.to(dev))
    assert text == "".join(chars[i] for i in want.tolist())

    er = EffRecognizer(str(ckpt), precision=prec, device=dev)
    assert er.arch == ARCH and er._eng_net.crop_dtype == torch.float32
    emb = er.run(q.numpy())[0]
    assert emb.shape == (n, D) and emb.dtype == np.float32
    top1 = (F.normalize(torch.from_numpy(emb), dim=1) @ index.T).argmax(dim=1)
    assert torch.equal(top1, want)


@pytest.mark.parametrize("B", [1, 16, 64, 1024])
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("screen", [False, True])
def test_knn_d1024_bit_exact(dev, B, k, screen):
    from effocr_amd.knn import IndexFlatIP
    rng = np.random.default_rng(B + k)
    X = rng.standard_normal((10_000, D)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = X[rng.integers(0, 10_000, B)] + 0.1 * rng.standard_normal((B, D)).astype(np.float32)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    idx = IndexFlatIP(D, device=dev, screen=screen)
    idx.add(X)
    Dg, Ig = idx.search(Q, k)
    Dr, Ir = knn_ref.flat_ip_search(Q, X, k)
    np.testing.assert_array_equal(Ig, Ir)
    np.testing.assert_array_equal(Dg.view(np.uint32), Dr.view(np.uint32))
