"""pvt_v2_b0 ... pvt_v2_b5 on the MI355X (-m gpu): end-to-end parity of libeffocr_pvt.so with the CPU restatement (tests/pvt_ref.py, pinned
to transformers.PvtV2Model by tests/test_pvt_host.py) in float64 — both miniatures at 32^2, 64^2, 96^2 and 224^2 (1, 4, 9 and 49 reduced
keys), pvt_v2_b0 and pvt_v2_b1 at 32^2 and 224^2, pvt_v2_b2 at 32^2 (other depths), every precision, 3 crops each —, bitwise invariance
to the call size, the position and the chunk, the fused normalise, the status word, the workspace, and the engines end to end.  The kernels
alone: tests/test_gpu_pvt_ops.py.

Bounds, in max norm relative to max|ref| AND in worst-row relative L2: the project's {"fp32": 1e-5, "fp16": 1e-3, "bf16": 8e-3}
(tests/test_gpu_encoder.py, tests/test_gpu_vit8.py).  Where the CPU emulation of the declared roundings (pvt_forward(prec=...): weights
and pixels rounded once, activations rounded between the kernels, the attention's P and output) on the same checkpoint and crops is itself
above half of a bound, that bound is 2 x the emulation's error in the same metric — the LeViT / RegNet precedent.  Never the device's output.

The crops (pvt_ref.crops) are square waves at every stride's scale: a token mean averages white noise away.

Sensitivity (test_reference_is_sensitive, on the CPU, the same checkpoints and crops): every entry of pvt_ref.MISTAKES moves every test
embedding by at least 10 x the bf16 bound of its case, all-zero crops move it by more than a quarter of its norm.  One size is left out
for two of the mistakes, by construction and for every model: at 32^2 each attention has a single key (8 x 8 tokens reduced by 8, ... ,
1 x 1 by 1) and the last stage a single token, so "scores not scaled" (a softmax over one key is 1 at any scale) and "token 0 instead of
the mean" are the network itself there; both are checked from 64^2 on, the other five at 32^2 too."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from effocr_amd import _lib
from effocr_amd import weights as W
from tests import pvt_ref as R

gpu = pytest.mark.gpu

MINI32, MINI64 = "pvt_v2_mini32_test", "pvt_v2_mini64_test"
REL = {"fp32": 1e-5, "fp16": 1e-3, "bf16": 8e-3}
PRECS = ["fp32", "fp16", "bf16"]
CASES = [(a, s) for a in (MINI32, MINI64) for s in (32, 64, 96, 224)] + [("pvt_v2_b0", 32), ("pvt_v2_b0", 224), ("pvt_v2_b1", 32), ("pvt_v2_b1", 224),
                                                                          ("pvt_v2_b2", 32)]
N_CROPS = 3
# init_state_dict(scale="trained") seed of a parity case: 1, except where seed 1 leaves one mistake under 10 x the bound on the CPU reference
# (pvt_v2_mini32_test at 32^2: "no_sr_norm" moves the embedding 9.7 %, the bound is 1.04 %); seed 8 was chosen there on the reference alone
CKPT_SEED = {(MINI32, 32): 8}


def max_err(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def row_l2_err(got, ref):
    return ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()


def _engine(arch, sd, img, prec, dev):
    from effocr_amd.encoders import make_encoder
    return make_encoder(arch, sd, img_size=img, precision=prec, device=dev)


_REFS = {}


def _ref(arch, img):
    """(state dict, crops, float64 reference embeddings, {precision: (max-norm, row-L2) error of the emulation}), computed once per case and
    shared, unchanged, by the precisions and the sensitivity test."""
    key = (arch, img)
    if key not in _REFS:
        sd, x = W.init_state_dict(arch, seed=CKPT_SEED.get(key, 1), scale="trained"), R.crops(N_CROPS, img, 7 + img)
        with torch.no_grad():
            ref = R.pvt_forward(arch, sd, x)
            emu = {}
            for p in ("fp16", "bf16"):
                e = R.pvt_forward(arch, sd, x, prec=p)
                emu[p] = (max_err(e, ref), row_l2_err(e, ref))
        _REFS[key] = (sd, x, ref, emu)
    return _REFS[key]


def _bounds(prec, emu):
    """(max-norm bound, row-L2 bound)"""
    if prec == "fp32":
        return REL[prec], REL[prec]
    return tuple(2 * e if e > REL[prec] / 2 else REL[prec] for e in emu[prec])


@gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("arch,img", CASES)
def test_parity(dev, arch, img, prec):
    sd, x, ref, emu = _ref(arch, img)
    bm, bl = _bounds(prec, emu)
    enc = _engine(arch, sd, img, prec, dev)
    assert enc.call_size_invariant is True and enc.embed_dim == W.embed_dim(arch)
    got = enc.forward(x.to(dev)).cpu().double()
    enc.check_status()
    em, el = max_err(got, ref), row_l2_err(got, ref)
    um, ul = emu.get(prec, (0.0, 0.0))
    print(f"pvt {arch} img {img} {prec}: max-norm {em:.2e} (emulated {um:.2e}, bound {bm:.2e})  row L2 {el:.2e} (emulated {ul:.2e}, bound {bl:.2e})")
    assert em <= bm and el <= bl, (em, bm, el, bl)


@pytest.mark.parametrize("arch,img", CASES)
def test_reference_is_sensitive(arch, img):
    """On the CPU, the yardstick alone, on the checkpoints and crops of test_parity: a device forward with one of pvt_ref.MISTAKES, or one
    that ignored its input, cannot pass the parity case."""
    sd, x, ref, emu = _ref(arch, img)
    bound = max(_bounds("bf16", emu))                      # the loosest mode the case runs in
    moved = lambda other: ((other.double() - ref).norm(dim=1) / ref.norm(dim=1)).min().item()
    with torch.no_grad():
        changes = {m: moved(R.pvt_forward(arch, sd, x, mistake=m, dtype=torch.float32)) for m in R.MISTAKES if not (img == 32 and m in ("token0", "no_scale"))}
        zero = moved(R.pvt_forward(arch, sd, torch.zeros_like(x), dtype=torch.float32))
    print(f"pvt {arch} img {img} reference moves (bf16 bound {bound:.2e}): " + ", ".join(f"{k} {v:.3f}" for k, v in changes.items()) + f", zero crops {zero:.3f}")
    for what, m in changes.items():
        assert m >= 10 * bound, (what, m, bound)
    assert zero > 0.25


@gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("arch,img", [(MINI32, 64), (MINI64, 224)])
def test_batch_position_and_chunk_invariance(dev, arch, prec, img):
    enc = _engine(arch, W.init_state_dict(arch, seed=2), img, prec, dev)
    crop = R.crops(1, img, 21).to(dev)
    alone = enc.forward(crop)
    five = R.crops(5, img, 22).to(dev)
    for at in (0, 4):
        call = five.clone()
        call[at] = crop[0]
        assert torch.equal(enc.forward(call)[at:at + 1], alone), at
    whole = enc.forward(five)
    for chunk in (2, 1, 0):
        enc.set_chunk(chunk)
        assert torch.equal(enc.forward(crop), alone), chunk
        assert torch.equal(enc.forward(five), whole), chunk
    enc.check_status()


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_l2_normalize_fused(dev, prec):
    enc = _engine(MINI32, W.init_state_dict(MINI32, seed=4), 64, prec, dev)
    x = R.crops(4, 64, 3).to(dev)
    raw = enc.forward(x)
    nrm = enc.forward(x, normalize=True)
    torch.testing.assert_close(nrm, F.normalize(raw, dim=1), rtol=0, atol=2e-7)
    enc.check_status()


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_status_reports_nonfinite_input(dev, prec):
    enc = _engine(MINI32, W.init_state_dict(MINI32, seed=5), 64, prec, dev)
    x = R.crops(4, 64, 8).to(dev)
    clean = enc.forward(x)
    enc.check_status()
    x[2, 1, 10, 10] = float("nan")
    emb = enc.forward(x)
    with pytest.raises(_lib.EffOCRHipError, match="code -6"):
        enc.check_status()
    assert not torch.isfinite(emb[2]).all()
    assert torch.equal(emb[[0, 1, 3]], clean[[0, 1, 3]])   # the other crops of the call are intact, bit for bit
    enc.check_status()                                     # read-and-clear
    x[2, 1, 10, 10] = 0.0
    assert torch.isfinite(enc.forward(x)).all()            # a clean call afterwards passes
    enc.check_status()
    enc.reset_status()
    enc.check_status()


@gpu
def test_workspace_is_monotone_honoured_and_too_small_is_refused(dev):
    img, B = 64, 3
    sd = W.init_state_dict(MINI32, seed=6)
    enc = _engine(MINI32, sd, img, "fp16", dev)
    L = enc._L
    sizes = [enc.workspace_bytes(b) for b in (1, 2, 3, 64, 256, 257, 4096)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[3] and sizes[4] == sizes[5] == sizes[6] < 1000 * (1 << 20)
    big = _engine("pvt_v2_b1", W.init_state_dict("pvt_v2_b1", seed=6, scale="timm"), 224, "fp32", dev)
    cap = big.workspace_bytes(4096)
    assert cap < 1000 * (1 << 20) and big.workspace_bytes(255) == cap and big.workspace_bytes(8) < cap   # the 1 GB budget, not 256 crops, binds here
    need = enc.workspace_bytes(B)
    x = R.crops(B, img, 1).to(dev)
    emb = torch.empty(B, 128, device=dev)
    guard = 4096                                           # the forward stays inside the bytes it asked for
    ws = torch.zeros(need + guard, dtype=torch.uint8, device=dev)
    ws[need:] = 0xA5
    s = _lib.current_stream(dev)
    assert L.effocr_pvt_forward(enc._h, _lib.ptr(x), B, _lib.ptr(emb), 0, _lib.ptr(ws), need - 1, s) == -3
    assert L.effocr_pvt_last_error() == b"pvt_forward: workspace too small"
    assert L.effocr_pvt_forward(enc._h, _lib.ptr(x), B, _lib.ptr(emb), 0, _lib.ptr(ws), need, s) == 0
    torch.cuda.synchronize(dev)
    assert torch.all(ws[need:] == 0xA5)
    assert torch.equal(emb, enc.forward(x))
    with pytest.raises(ValueError):
        enc.forward(x.half())                              # fp32 crops only
    h = ctypes.c_void_p()                                  # a handle whose weights were never uploaded refuses to run
    assert L.effocr_pvt_create(MINI32.encode(), img, 1, ctypes.byref(h)) == 0
    try:
        assert L.effocr_pvt_forward(h, _lib.ptr(x), B, _lib.ptr(emb), 0, _lib.ptr(ws), need, s) == -5
    finally:
        L.effocr_pvt_destroy(h)


@gpu
def test_end_to_end_engines(dev, tmp_path):
    """A saved pvt_v2_mini32_test checkpoint (64^2 crops) through AutoEncoderFactory.load, EffRecognizer (architecture inferred from the
    checkpoint, the crop size given) and the Recognizer pipeline on a 300-row index built by train_knn: top-1 ids equal to those of the
    float64 reference embeddings; then the classifier's logits against emb @ W^T + b."""
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.encoders import AutoEncoderFactory, PvtEncoder
    from effocr_amd.knn import FaissKNN, IndexFlatIP, InferenceModel
    from effocr_amd.pipeline import Recognizer
    from effocr_amd.recognizer_engine import EffRecognizer
    n, rows, ncls, img = 8, 300, 7, 64
    sd = W.init_state_dict(MINI32, seed=7, scale="trained", num_classes=ncls)
    ckpt = tmp_path / "enc_best.pth"
    W.save_checkpoint(sd, ckpt)
    renders = R.crops(rows, img, 31)
    pick = torch.arange(n) * 37 % rows
    q = renders[pick] + 0.05 * torch.randn(n, 3, img, img, generator=torch.Generator().manual_seed(32))
    enc_sd = {k: v for k, v in sd.items() if not k.startswith("head.")}
    with torch.no_grad():
        index64 = F.normalize(R.pvt_forward(MINI32, enc_sd, renders), dim=1)
        q64 = R.pvt_forward(MINI32, enc_sd, q)
    want = (F.normalize(q64, dim=1) @ index64.T).argmax(dim=1)
    assert torch.equal(want, pick)                         # crop i resembles glyph pick[i]
    chars = [chr(0x4E00 + i) for i in range(rows)]

    enc = AutoEncoderFactory("timm", MINI32, precision="fp32", img_size=img).load(str(ckpt))
    enc.to(dev).eval()
    assert isinstance(enc.engine, PvtEncoder)
    knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
    InferenceModel(enc, knn_func=knn).train_knn(renders, batch_size=64)
    assert knn.index.ntotal == rows and knn.index.d == 128
    rec = Recognizer(enc, knn, chars, knn=10)
    _, idx = rec.neighbors(q.to(dev))
    assert torch.equal(idx[:, 0].cpu(), want)
    _, _, text = rec(q.to(dev))
    assert text == "".join(chars[i] for i in want.tolist())
    enc.check_status()

    for prec in ("fp32", "fp16"):
        er = EffRecognizer(str(ckpt), precision=prec, img_size=img, device=dev)
        assert er.arch == MINI32 and er.img_size == img and er.crop_dtype == torch.float32 and er.call_size_invariant
        emb = er.run(q.numpy())[0]
        assert emb.shape == (n, 128) and emb.dtype == np.float32
        assert torch.equal((F.normalize(torch.from_numpy(emb).double(), dim=1) @ index64.T).argmax(dim=1), want)

    clf = AutoClassifierFactory("timm", MINI32, n_classes=ncls, img_size=img, precision="fp32").load(str(ckpt))
    clf.to(dev).eval()
    lg = clf(q.to(dev))
    want_lg = q64 @ sd["head.weight"].double().T + sd["head.bias"].double()
    assert lg.shape == (n, ncls)
    assert max_err(lg.cpu().double(), want_lg) <= 1e-5
    assert torch.equal(clf.predict(q.to(dev)), lg.argmax(dim=1))
    clf.check_status()
