"""resnet34 / resnet50 on the MI355X (-m gpu): parity with the CPU restatement (tests/resnet_ref.py, pinned to transformers by
tests/test_resnet_host.py) in every precision at 224^2 and 64^2, an f16 range case with trained-magnitude BatchNorm statistics, call-size
and sub-batch invariance, the status word, the workspace, and the engines end to end (EffRecognizer, Recognizer, the classifier)."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from effocr_amd import _lib
from effocr_amd import weights as W
from tests.resnet_ref import resnet_forward

pytestmark = pytest.mark.gpu

ARCHS = ["resnet34", "resnet50"]
# bounds, max norm AND worst-row relative L2, those of the other encoders: fp32 = the exact mode, fp16 = north_star's 1e-3, bf16 1e-2
REL = {"fp32": 1e-5, "fp16": 1e-3, "bf16": 1e-2}


def rel_err(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def row_l2_err(got, ref):
    return ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()


def _trained(arch, seed):
    """BatchNorm statistics of a trained network's magnitude: small running variances (U(0.002, 0.05)), large gammas (U(1, 3), the
    last BN of a branch U(0.1, 0.4)) and means / betas of a few tenths, so BN folding scales the weights by up to ~70x."""
    sd = W.init_state_dict(arch, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    last = "bn3" if arch == "resnet50" else "bn2"
    for k in sd:
        if k.endswith("running_var"):
            sd[k] = torch.rand(sd[k].shape, generator=g) * 0.048 + 0.002
        elif k.endswith("running_mean") or (k.endswith(".bias") and sd[k].dim() == 1):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.3
        elif k.endswith(".weight") and sd[k].dim() == 1:
            lo, hi = (0.1, 0.4) if k.rsplit(".", 2)[-2] == last else (1.0, 3.0)
            sd[k] = torch.rand(sd[k].shape, generator=g) * (hi - lo) + lo
    # the fan-in-scaled convs of a network whose BN divides by sqrt(var): keep the pre-BN activations at the running statistics' scale
    for k in sd:
        if sd[k].dim() == 4:
            sd[k] = sd[k] * 0.1
    return sd


def _crops(B, seed, img=224):
    """ImageNet-normalised-looking crops with bright / dark glyph strokes near the borders (the padded taps of every stride)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, img, img, generator=g) * 0.5
    s = img // 32
    for b in range(B):
        o = int(torch.randint(0, s + 1, (1,), generator=g))
        x[b, :, 1 + o:4 * s + o, 0:2 * s] += 2.5
        x[b, :, img - 4 * s:img, img - 3 * s - o:img - o] -= 2.0
        x[b, :, img // 2:img // 2 + s, :] += 1.5
    return x


def _engine(arch, sd, prec, dev, img=224):
    from effocr_amd.encoders import make_encoder
    return make_encoder(arch, sd, img_size=img, precision=prec, device=dev)


_REFS = {}


def _ref(arch, img, B, trained=False):
    key = (arch, img, B, trained)
    if key not in _REFS:                                   # (the float64 restatement takes seconds: once per case, not per precision)
        sd = _trained(arch, 11) if trained else W.init_state_dict(arch, seed=1, img_size=img)
        x = _crops(B, 7 + B, img)
        _REFS[key] = (sd, x, resnet_forward(arch, sd, x.double()).float())
    return _REFS[key]


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("img,B", [(224, 3), (64, 4)])
def test_parity(dev, arch, prec, img, B):
    sd, x, ref = _ref(arch, img, B)
    enc = _engine(arch, sd, prec, dev, img)
    assert enc.embed_dim == W.embed_dim(arch)
    got = enc.forward(x.to(dev)).cpu()
    enc.check_status()
    e_max, e_row = rel_err(got, ref), row_l2_err(got, ref)
    print(f"{arch} {prec} {img}^2 B={B}: max-norm {e_max:.2e}, row L2 {e_row:.2e}")
    assert e_max <= REL[prec] and e_row <= REL[prec]


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_parity_trained_magnitudes(dev, arch, prec):
    sd, x, ref = _ref(arch, 224, 2, trained=True)
    enc = _engine(arch, sd, prec, dev)
    got = enc.forward(x.to(dev)).cpu()
    enc.check_status()                                     # no f16 overflow
    e_max, e_row = rel_err(got, ref), row_l2_err(got, ref)
    print(f"{arch} {prec} trained magnitudes: max-norm {e_max:.2e}, row L2 {e_row:.2e}, |emb| max {ref.abs().max():.3g}")
    assert e_max <= REL[prec] and e_row <= REL[prec]


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_call_size_and_chunk_invariance(dev, arch, prec):
    sd = W.init_state_dict(arch, seed=2)
    enc = _engine(arch, sd, prec, dev)
    x7 = _crops(7, 21).to(dev)
    base = enc.forward(x7)
    assert torch.equal(enc.forward(x7[3:4]), base[3:4])
    for n in (64, 300):
        big = _crops(n, 140 + n).to(dev)
        pos = torch.randperm(n, generator=torch.Generator().manual_seed(n))[:7].to(dev)
        big[pos] = x7
        assert torch.equal(enc.forward(big)[pos], base), n
    for chunk in (5, 3, 1, 0):                             # sub-batch boundaries inside the 7 crops
        enc.set_chunk(chunk)
        assert torch.equal(enc.forward(x7), base), chunk
    enc.check_status()


@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_l2_normalize_fused(dev, prec):
    enc = _engine("resnet50", W.init_state_dict("resnet50", seed=4), prec, dev)
    x = _crops(4, 3).to(dev)
    raw = enc.forward(x)
    nrm = enc.forward(x, normalize=True)
    torch.testing.assert_close(nrm, F.normalize(raw, dim=1), rtol=0, atol=2e-7)
    enc.check_status()


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_status_reports_nonfinite_input(dev, prec):
    """Every precision, a NaN and an inf crop: the fp32 mode's ReLU and max pool propagate a NaN as the 16-bit path's do
    (tests/test_gpu_convops.py)."""
    enc = _engine("resnet34", W.init_state_dict("resnet34", seed=5), prec, dev)
    for bad in (float("nan"), float("inf")):
        x = _crops(4, 8).to(dev)
        enc.forward(x)
        enc.check_status()
        x[2, 1, 10, 10] = bad
        emb = enc.forward(x)
        with pytest.raises(_lib.EffOCRHipError, match="code -6"):
            enc.check_status()
        assert not torch.isfinite(emb[2]).all()
        assert torch.isfinite(emb[[0, 1, 3]]).all()        # the other crops of the call are untouched
        enc.check_status()                                 # read-and-clear


def test_workspace_too_small_is_refused(dev):
    enc = _engine("resnet50", W.init_state_dict("resnet50", seed=6), "fp16", dev)
    L = enc._L
    B = 3
    need = enc.workspace_bytes(B)
    x = _crops(B, 1).to(dev)
    emb = torch.empty(B, 2048, device=dev)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    s = _lib.current_stream(dev)
    assert L.effocr_resnet_forward(enc._h, _lib.ptr(x), B, _lib.ptr(emb), 0, _lib.ptr(ws), need - 1, s) == -3
    assert b"workspace" in L.effocr_resnet_last_error()
    assert L.effocr_resnet_forward(enc._h, _lib.ptr(x), B, _lib.ptr(emb), 0, _lib.ptr(ws), need, s) == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(emb, enc.forward(x))
    with pytest.raises(ValueError):
        enc.forward(x.half())                              # fp32 crops only


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_end_to_end_engines(dev, arch, prec, tmp_path):
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.encoders import AutoEncoderFactory
    from effocr_amd.knn import FaissKNN, IndexFlatIP
    from effocr_amd.pipeline import Recognizer
    from effocr_amd.recognizer_engine import EffRecognizer
    n, ncls, img = 10, 10, 64
    D = W.embed_dim(arch)
    sd = W.init_state_dict(arch, seed=7, img_size=img, num_classes=ncls)
    ckpt = tmp_path / "enc_best.pth"
    W.save_checkpoint(sd, ckpt)
    glyphs = _crops(n, 31, img)
    ref = resnet_forward(arch, sd, glyphs.double()).float()
    g = torch.Generator().manual_seed(9)
    dis = F.normalize(torch.randn(500, D, generator=g), dim=1)
    index = torch.cat([dis[:250], F.normalize(ref, dim=1), dis[250:]])
    chars = [chr(0x4E00 + i) for i in range(index.shape[0])]
    q = glyphs + 0.05 * torch.randn(glyphs.shape, generator=torch.Generator().manual_seed(32))
    want = torch.arange(n) + 250

    enc = AutoEncoderFactory("timm", arch, precision=prec, img_size=img).load(str(ckpt))
    enc.to(dev).eval()
    knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
    knn.train(index)
    rec = Recognizer(enc, knn, chars, knn=10)
    _, idx = rec.neighbors(q.to(dev))
    assert torch.equal(idx[:, 0].cpu(), want)              # top-1 against the planted glyph index is exact
    _, _, text = rec(q.to(dev))
    assert text == "".join(chars[i] for i in want.tolist())

    er = EffRecognizer(str(ckpt), precision=prec, img_size=img, device=dev)
    assert er.arch == arch and er.crop_dtype == torch.float32
    out = er.run(q.numpy())
    assert isinstance(out, list) and len(out) == 1         # the reference's list-of-one [B, D]
    emb = out[0]
    assert emb.shape == (n, D) and emb.dtype == np.float32
    top1 = (F.normalize(torch.from_numpy(emb), dim=1) @ index.T).argmax(dim=1)
    assert torch.equal(top1, want)

    clf = AutoClassifierFactory("timm", arch, n_classes=ncls, precision=prec, img_size=img).load(str(ckpt))
    clf.to(dev).eval()
    feats = enc(q.to(dev))                                 # the pooled feature before normalisation: the head's input
    lg_torch = feats.cpu() @ sd["fc.weight"].T + sd["fc.bias"]
    lg = clf(q.to(dev)).cpu()
    assert lg.shape == (n, ncls)
    torch.testing.assert_close(lg, lg_torch, rtol=1e-5, atol=1e-5 * lg_torch.abs().max().item())
    assert torch.equal(clf.predict(q.to(dev)).cpu(), lg.argmax(dim=1))
    print(f"{arch} end to end ({prec}): {n} planted glyphs recognised, classifier logits equal a torch fp32 head's")
