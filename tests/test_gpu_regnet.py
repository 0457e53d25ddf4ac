"""RegNetX / RegNetY on libeffocr_regnet.so on the MI355X (-m gpu) against the float64 restatement (tests/regnet_ref.py): three miniatures
(group widths 8, 16 and 24 — the last a RegNetY with odd group counts) at 32^2, 64^2 and 96^2 with 1, 3 and 5 crops, regnetx_002 and
regnety_008 at 224^2 with 1 and 3 crops, all three precisions; call-size invariance, the fused normalisation, the status word, the engines.

Bounds (max norm relative to max|ref| AND worst-row relative L2), from tests/test_gpu_mobilenetv3_family.py, which runs the same scheme
(fp32 activations, weights in the mode's type): fp32 1e-5, fp16 1e-3, bf16 1e-2.  For every seeded checkpoint the CPU emulation of the
declared roundings (regnet_forward(..., prec=...): BatchNorm folded in double, the 1x1 and grouped weights rounded once to the mode's type,
activations as hi + lo, everything else exact) is run first; where its error already exceeds half the bound, the bound is 2 x the emulation's
error (bound_for).  The emulation's error is printed with every case.

Sensitivity, asserted on the CPU reference inside every parity case: two different crops' embeddings differ by at least 10 x the bound, and
each of five mistakes — the groups shifted by one, the gate dropped (RegNetY), the ReLU before the add, the shortcut sampled at the odd
pixels, stride 2 missing in s1 — moves EVERY embedding by at least 10 x the bound.  White-noise crops average out under the global pool
(at 224^2 two crops' embeddings differ by 5 to 7 %, under 10 x the bf16 bound), so the crops carry square waves of period 4 to 64 with
per-crop amplitudes over the noise: structure at every stride's scale.  The seeds below were chosen on the CPU reference for the widest
margin; no size had to be left out.  A sixth mistake, the squeeze-excite width taken from w instead of the block's input width, cannot be
stated on a fixed checkpoint: it changes se.fc1's shape, so it is a load error, not a different embedding — tests/test_regnet_host.py pins
the widths through the parameter counts and transformers.RegNetModel instead."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from effocr_amd import _lib
from effocr_amd import weights as W
from tests.regnet_ref import ARCHS, MISTAKES, regnet_forward, regnet_logits

gpu = pytest.mark.gpu

MINI8, MINI16, MINI24 = "regnetx_mini8_test", "regnetx_mini16_test", "regnety_mini24_test"
REL = {"fp32": 1e-5, "fp16": 1e-3, "bf16": 1e-2}
MAX_B = {32: 5, 64: 5, 96: 5, 224: 3}
# checkpoint seeds (init_state_dict(arch, seed)), chosen on the CPU reference: the widest margin of the sensitivity checks
CKPT_SEED = {(MINI8, 32): 3, (MINI8, 64): 2, (MINI8, 96): 3, (MINI16, 32): 2, (MINI16, 64): 2, (MINI16, 96): 2,
             (MINI24, 32): 1, (MINI24, 64): 3, (MINI24, 96): 1, ("regnetx_002", 224): 4, ("regnety_008", 224): 3}


def rel_err(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def row_l2_err(got, ref):
    return ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()


def bound_for(prec, emulated):
    """The mode's bound, or 2 x the emulation's error where that already exceeds half of it."""
    return 2 * emulated if emulated > REL[prec] / 2 else REL[prec]


def structured_crops(B, img, seed=None):
    """[B,3,img,img] fp32: N(0, 0.5) noise plus, per crop and channel, square waves of period 4, 8, 16, 32 and 64 in both directions with
    amplitudes +-U(0.5, 1.5): what a stride-2 sampling at the wrong phase, at any stage, changes."""
    g = torch.Generator().manual_seed(7 + img if seed is None else seed)
    x = torch.randn(B, 3, img, img, generator=g) * 0.5
    i = torch.arange(img)
    for p in (4, 8, 16, 32, 64):
        if p > img:
            break
        sq = torch.where((i % p) < p // 2, 1.0, -1.0)
        amp = (torch.rand(B, 3, 1, 1, generator=g) + 0.5) * torch.where(torch.rand(B, 3, 1, 1, generator=g) < 0.5, -1.0, 1.0)
        x = x + amp * sq[None, None, :, None] * sq[None, None, None, :]
    return x


@functools.lru_cache(maxsize=None)
def _case(arch, img):
    """Computed once per (arch, img) and shared by the precisions: the checkpoint, MAX_B crops, the float64 reference, the least relative
    distance between two crops' embeddings, the least move of an embedding under each mistake, and the emulation's errors per mode."""
    sd = W.init_state_dict(arch, seed=CKPT_SEED[(arch, img)])
    B = MAX_B[img]
    x = structured_crops(B, img)
    with torch.no_grad():
        ref = regnet_forward(arch, sd, x.double())
        crop = min(((ref[i] - ref[j]).norm() / ref[i].norm()).item() for i in range(B) for j in range(B) if i != j)
        moves = {}
        for m in MISTAKES:
            if m == "no_gate" and not ARCHS[arch][3]:
                continue
            moves[m] = ((regnet_forward(arch, sd, x.double(), mistake=m) - ref).norm(dim=1) / ref.norm(dim=1)).min().item()
        emu = {"fp32": (0.0, 0.0)}
        for prec in ("fp16", "bf16"):
            e = regnet_forward(arch, sd, x.double(), prec=prec)
            emu[prec] = (rel_err(e, ref), row_l2_err(e, ref))
    return sd, x, ref, crop, moves, emu


def _engine(arch, sd, img, prec, dev):
    from effocr_amd.encoders import RegNetEncoder, make_encoder
    enc = make_encoder(arch, sd, img_size=img, precision=prec, device=dev)
    assert type(enc) is RegNetEncoder and enc.crop_dtype == torch.float32 and enc.call_size_invariant
    return enc


def _parity(dev, arch, img, prec, batches):
    sd, x, ref, crop, moves, emu = _case(arch, img)
    b_max, b_row = bound_for(prec, emu[prec][0]), bound_for(prec, emu[prec][1])
    worst = max(b_max, b_row)
    print(f"{arch} {prec} {img}^2: emulation {emu[prec][0]:.2e} / {emu[prec][1]:.2e}, bound {b_max:.2e} / {b_row:.2e}; crops differ by "
          f"{crop:.3f}, mistakes move an embedding by at least " + ", ".join(f"{k} {v:.3f}" for k, v in moves.items()))
    assert crop >= 10 * worst                                  # the reference depends on the crop ...
    for m, v in moves.items():
        assert v >= 10 * worst, m                              # ... and on every property a wrong kernel or forward would break
    enc = _engine(arch, sd, img, prec, dev)
    for B in batches:
        got = enc.forward(x[:B].to(dev)).cpu().double()
        enc.check_status()
        e_max, e_row = rel_err(got, ref[:B]), row_l2_err(got, ref[:B])
        print(f"    B={B}: max-norm {e_max:.2e}, row L2 {e_row:.2e}")
        assert got.shape == (B, W.embed_dim(arch))
        assert e_max <= b_max and e_row <= b_row, (B, e_max, e_row)


@gpu
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("img", [32, 64, 96])
@pytest.mark.parametrize("arch", [MINI8, MINI16, MINI24])
def test_miniature_parity(dev, arch, img, prec):
    _parity(dev, arch, img, prec, (1, 3, 5))


@gpu
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("arch", ["regnetx_002", "regnety_008"])
def test_full_model_parity(dev, arch, prec):
    _parity(dev, arch, 224, prec, (1, 3))


@gpu
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("arch,img", [(MINI24, 64), (MINI8, 96), ("regnety_008", 224)])
def test_embedding_is_bitwise_independent_of_the_call(dev, arch, img, prec):
    """A crop's embedding is bitwise the same alone, at any position of a 5-crop call, under set_chunk(2) and across sub-batches."""
    sd = _case(arch, img)[0]
    enc = _engine(arch, sd, img, prec, dev)
    five = structured_crops(5, img, seed=99).to(dev)
    whole = enc.forward(five)
    for pos in range(5):
        assert torch.equal(enc.forward(five[pos:pos + 1])[0], whole[pos]), pos
    order = [3, 0, 4, 1, 2]
    assert torch.equal(enc.forward(five[order]), whole[order])
    for chunk in (1, 2, 3, 0):
        enc.set_chunk(chunk)
        assert torch.equal(enc.forward(five), whole), chunk
    enc.check_status()


@gpu
@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_l2_normalize_fused(dev, prec):
    enc = _engine(MINI24, _case(MINI24, 64)[0], 64, prec, dev)
    x = structured_crops(4, 64, seed=3).to(dev)
    raw = enc.forward(x)
    nrm = enc.forward(x, normalize=True)
    torch.testing.assert_close(nrm, F.normalize(raw, dim=1), rtol=0, atol=2e-7)
    enc.check_status()


@gpu
@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("arch", [MINI16, MINI24])
def test_status_reports_nonfinite_input(dev, arch, prec):
    enc = _engine(arch, _case(arch, 64)[0], 64, prec, dev)
    x = structured_crops(4, 64, seed=8).to(dev)
    clean = enc.forward(x)
    enc.check_status()
    x[2, 1, 10, 10] = float("nan")
    emb = enc.forward(x)
    with pytest.raises(_lib.EffOCRHipError, match="code -6"):
        enc.check_status()
    assert not torch.isfinite(emb[2]).all()
    assert torch.equal(emb[[0, 1, 3]], clean[[0, 1, 3]])   # the other crops of the call are intact, bit for bit
    enc.check_status()                                     # read-and-clear
    enc.forward(x)
    enc.reset_status()                                     # cleared without being read
    enc.check_status()


@gpu
def test_workspace_is_honoured_too_small_is_refused_and_upload_comes_first(dev):
    img, B = 64, 3
    sd = _case(MINI24, img)[0]
    enc = _engine(MINI24, sd, img, "fp16", dev)
    L = enc._L
    need = enc.workspace_bytes(B)
    x = structured_crops(B, img, seed=1).to(dev)
    emb = torch.empty(B, 120, device=dev)
    guard = 4096                                           # the forward stays inside the bytes it asked for
    ws = torch.zeros(need + guard, dtype=torch.uint8, device=dev)
    ws[need:] = 0xA5
    s = _lib.current_stream(dev)
    assert L.effocr_regnet_forward(enc._h, _lib.ptr(x), B, _lib.ptr(emb), 0, _lib.ptr(ws), need - 1, s) == -3
    assert L.effocr_regnet_last_error() == b"regnet_forward: workspace too small"
    assert L.effocr_regnet_forward(enc._h, _lib.ptr(x), B, _lib.ptr(emb), 0, _lib.ptr(ws), need, s) == 0
    torch.cuda.synchronize(dev)
    assert torch.all(ws[need:] == 0xA5)
    assert torch.equal(emb, enc.forward(x))
    with pytest.raises(ValueError):
        enc.forward(x.half())                              # fp32 crops only
    h = ctypes.c_void_p()
    assert L.effocr_regnet_create(MINI24.encode(), img, 1, ctypes.byref(h)) == 0
    try:
        assert L.effocr_regnet_forward(h, _lib.ptr(x), B, _lib.ptr(emb), 0, _lib.ptr(ws), need, s) == -5
        assert L.effocr_regnet_last_error() == b"regnet_forward: weights were not uploaded"
    finally:
        L.effocr_regnet_destroy(h)


@gpu
def test_end_to_end_engines(dev, tmp_path):
    """A saved regnety_mini24_test checkpoint (64^2 crops) through AutoEncoderFactory.load, EffRecognizer (architecture inferred from the
    checkpoint, the crop size given), top-1 ids against a seeded index identical to the reference's wherever the margin is above 1e-4, the
    Recognizer pipeline, and the classifier (logits and predict)."""
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.encoders import AutoEncoderFactory, RegNetEncoder
    from effocr_amd.knn import FaissKNN, IndexFlatIP
    from effocr_amd.pipeline import Recognizer
    from effocr_amd.recognizer_engine import EffRecognizer
    from oracle import knn_ref
    n, ncls, img, D = 8, 7, 64, 120
    sd = W.init_state_dict(MINI24, seed=7, num_classes=ncls)
    ckpt = tmp_path / "enc_best.pth"
    W.save_checkpoint(sd, ckpt)
    q = structured_crops(n, img, seed=31)
    with torch.no_grad():
        ref = F.normalize(regnet_forward(MINI24, sd, q.double()), dim=1)
    index = F.normalize(torch.randn(600, D, generator=torch.Generator().manual_seed(9)).abs(), dim=1)   # (embeddings are non-negative)
    scores = ref @ index.double().T
    top2 = scores.topk(2, dim=1)
    clear = (top2.values[:, 0] - top2.values[:, 1]) > 1e-4
    assert clear.sum() >= n - 1
    chars = [chr(0x4E00 + i) for i in range(600)]

    for prec in ("fp32", "fp16", "bf16"):
        er = EffRecognizer(str(ckpt), precision=prec, img_size=img, device=dev)
        assert er.arch == MINI24 and er.img_size == img and er.crop_dtype == torch.float32 and er.call_size_invariant
        emb = er.run(q.numpy())[0]
        assert emb.shape == (n, D) and emb.dtype == np.float32
        ids = (F.normalize(torch.from_numpy(emb), dim=1) @ index.T).argmax(dim=1)
        if prec == "fp32":
            assert torch.equal(ids[clear], top2.indices[clear, 0])
        else:                                              # 16-bit: identical wherever the reference's margin exceeds the mode's error
            far = (top2.values[:, 0] - top2.values[:, 1]) > 4 * REL[prec]
            assert torch.equal(ids[far], top2.indices[far, 0])

    enc = AutoEncoderFactory("timm", MINI24, img_size=img, precision="fp32").load(str(ckpt))
    enc.to(dev).eval()
    assert isinstance(enc.engine, RegNetEncoder)
    knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
    knn.train(index)
    rec = Recognizer(enc, knn, chars, knn=10)
    dist, idx = rec.neighbors(q.to(dev))
    emb_hip = rec.recognizer.get_embeddings(q.to(dev)).cpu()
    _, i_ref = knn_ref.flat_ip_search(emb_hip.numpy(), index.numpy(), 10)
    assert np.array_equal(idx.cpu().numpy(), i_ref)        # k-NN ids equal to the oracle search
    assert torch.equal(idx[:, 0].cpu()[clear], top2.indices[clear, 0])

    clf = AutoClassifierFactory("timm", MINI24, n_classes=ncls, img_size=img, precision="fp32").load(str(ckpt))
    clf.to(dev).eval()
    lg = clf(q.to(dev))
    assert lg.shape == (n, ncls)
    with torch.no_grad():
        want_lg = regnet_logits(MINI24, sd, q.double())
    assert ((lg.cpu().double() - want_lg).abs().max() / want_lg.abs().max()).item() <= 1e-5
    assert torch.equal(clf.predict(q.to(dev)), lg.argmax(dim=1))
    gap = want_lg.topk(2, dim=1).values
    sure = (gap[:, 0] - gap[:, 1]) > 1e-4
    assert torch.equal(clf.predict(q.to(dev)).cpu()[sure], want_lg.argmax(dim=1)[sure])
    clf.check_status()


@gpu
@pytest.mark.parametrize("d", [368, 440, 888, 120])
def test_knn_index_takes_regnet_embedding_widths(dev, d, tmp_path):
    """Six of the ten models' embedding widths (368, 440, 528, 888, 912) are no multiple of 32, which the k-NN kernels require:
    IndexFlatIP stores and searches such rows with zero columns up to the next multiple — the same inner products — and speaks d outside."""
    from effocr_amd.knn import IndexFlatIP, read_index, write_index
    from oracle import knn_ref
    g = torch.Generator().manual_seed(d)
    xb = F.normalize(torch.randn(700, d, generator=g), dim=1)
    q = F.normalize(xb[:40] + 0.1 * torch.randn(40, d, generator=g), dim=1)
    idx = IndexFlatIP(d, device=dev)
    idx.add(xb.numpy())
    assert idx.d == d and idx.ntotal == 700 and idx.reconstruct_n(3, 5).shape == (5, d)
    assert np.array_equal(idx.reconstruct_n(), xb.numpy())
    D, I = idx.search(q.numpy(), 10)
    D_ref, I_ref = knn_ref.flat_ip_search(q.numpy(), xb.numpy(), 10)
    assert np.array_equal(I, I_ref) and np.array_equal(I[:, 0], np.arange(40))
    assert np.abs(D - D_ref).max() <= 1e-6
    assert idx.remove_ids([0, 5]) == 2 and idx.ntotal == 698 and idx.search(q.numpy()[1:2], 1)[1][0, 0] == 0
    write_index(idx, str(tmp_path / "ref.index"))
    back = read_index(str(tmp_path / "ref.index"), device=dev)
    assert back.d == d and np.array_equal(back.reconstruct_n(), idx.reconstruct_n())
    with pytest.raises(ValueError):
        idx.search(np.zeros((1, d + 1), dtype=np.float32), 1)


@gpu
def test_named_classifier_factory(dev):
    """AutoClassifierFactory("timm", "regnetx_002", n_classes=7): logits against the reference, predict against argmax."""
    from effocr_amd.classifiers import AutoClassifierFactory
    clf = AutoClassifierFactory("timm", "regnetx_002", n_classes=7, precision="fp32")(seed=3)
    clf.to(dev).eval()
    x = structured_crops(2, 224, seed=5)
    lg = clf(x.to(dev))
    sd = W.strip_prefix(clf.state_dict())
    with torch.no_grad():
        want = regnet_logits("regnetx_002", sd, x.double())
    assert lg.shape == (2, 7)
    assert ((lg.cpu().double() - want).abs().max() / want.abs().max()).item() <= 1e-5
    assert torch.equal(clf.predict(x.to(dev)), lg.argmax(dim=1))
    clf.check_status()
