"""-m gpu: the FFNN classifier recognizer (libeffocr_head.so, effocr_amd.classifiers, pipeline.ClassifierRecognizer) on the MI355X."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from effocr_amd import _lib
from effocr_amd import weights as W

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL = {"fp32": 1e-5, "fp16": 1e-3, "bf16": 1e-2}


def head_call(emb, w, b, logits=True, ids=True, ws_bytes=None):
    """Raw call -> (rc, logits or None, ids or None)."""
    L = _lib.head_lib()
    B, d = emb.shape
    N = w.shape[0]
    lo = torch.full((B, N), -7.0, device=emb.device) if logits else None
    io = torch.full((B,), -5, dtype=torch.int64, device=emb.device) if ids else None
    need = int(L.effocr_classifier_head_workspace_bytes(B, N))
    nb = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=emb.device)
    rc = L.effocr_classifier_head(_lib.ptr(emb), B, d, _lib.ptr(w), _lib.ptr(b), N, _lib.ptr(lo), _lib.ptr(io), _lib.ptr(ws),
                                  ctypes.c_size_t(nb), _lib.current_stream(emb.device))
    torch.cuda.synchronize()
    return rc, lo, io


def problem(B, N, d, dev, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + B * 31 + N * 3 + d)
    emb = torch.randn(B, d, generator=g).to(dev)
    w = (torch.randn(N, d, generator=g) / d ** 0.5).to(dev)
    b = (torch.randn(N, generator=g) * 0.1).to(dev)
    return emb, w, b


def check_parity(emb, w, b, lo, io):
    ref = emb.double() @ w.double().T + b.double()
    if ref.numel():
        rel = ((lo.double() - ref).abs().max() / ref.abs().max()).item()
        assert rel < 2e-6, rel
    assert torch.equal(io, torch.argmax(lo, -1)), "ids differ from torch.argmax of the library's own logits"


SHAPES = [(B, N, 384) for B in (0, 1, 16, 37, 1024) for N in (1, 63, 64, 65, 182, 30813)] + \
         [(B, N, d) for d in (128, 512, 768, 1024) for B, N in ((1, 65), (37, 182), (16, 30813), (1024, 64))] + [(1024, 30813, 1024)]


@pytest.mark.parametrize("B,N,d", SHAPES)
def test_head_parity_and_argmax(dev, B, N, d):
    emb, w, b = problem(B, N, d, dev)
    rc, lo, io = head_call(emb, w, b)
    assert rc == 0, _lib.head_lib().effocr_head_last_error()
    check_parity(emb, w, b, lo, io)
    rc, lo2, io2 = head_call(emb, w, b, logits=False)            # the fused argmax alone gives the same ids
    assert rc == 0 and torch.equal(io2, io)


def test_head_bitwise_independent_of_batch_and_class_split(dev):
    B, N, d = 1024, 30813, 384
    emb, w, b = problem(B, N, d, dev, seed=3)
    _, lo, io = head_call(emb, w, b)
    for lo_b, hi_b in ((0, 1), (5, 21), (100, 137), (960, 1024), (0, 64), (200, 500)):
        _, l2, i2 = head_call(emb[lo_b:hi_b].contiguous(), w, b)
        assert torch.equal(l2, lo[lo_b:hi_b]) and torch.equal(i2, io[lo_b:hi_b]), (lo_b, hi_b)
    for n0, n1 in ((0, 182), (0, 64), (64, 30813), (1000, 1065), (30000, 30813)):
        _, l3, _ = head_call(emb, w[n0:n1].contiguous(), b[n0:n1].contiguous(), ids=False)
        assert torch.equal(l3, lo[:, n0:n1]), (n0, n1)


@pytest.mark.parametrize("B,N", [(1, 182), (37, 182), (16, 30813), (1024, 30813), (37, 63)])
def test_head_ties_pick_the_first_index(dev, B, N):
    emb, w, b = problem(B, N, 384, dev, seed=5)
    pos = [j for j in (5, 40, 63, 100, 180, 20000) if j < N]
    big = emb.mean(0) * 0 + 1.0                                   # every row of emb gets the same large logit on the planted classes
    for j in pos:
        w[j] = big * 5.0
        b[j] = 50.0
    emb = emb.abs() + 1.0                                          # positive rows: the planted classes dominate, exactly tied
    rc, lo, io = head_call(emb, w, b)
    assert rc == 0
    assert (io == pos[0]).all(), io.unique()
    assert torch.equal(io, torch.argmax(lo, -1))


@pytest.mark.parametrize("B,N", [(3, 182), (37, 30813), (100, 65)])
def test_head_nan_is_the_maximum_and_the_first_nan_wins(dev, B, N):
    emb, w, b = problem(B, N, 384, dev, seed=9)
    cols = [j for j in (64, 70, 130) if j < N]
    for j in cols:
        w[j, 11] = float("nan")                                   # class j's logit is NaN for every row
    w[0] = 100.0                                                   # a finite maximum before the NaNs
    emb[1] = float("nan")                                          # row 1: every logit NaN -> class 0
    rc, lo, io = head_call(emb, w, b)
    assert rc == 0
    want = torch.full((B,), cols[0], dtype=torch.int64, device=dev)
    want[1] = 0
    assert torch.equal(io, want), io


def test_head_refusals_launch_nothing(dev):
    emb, w, b = problem(16, 182, 384, dev)
    L = _lib.head_lib()
    need = int(L.effocr_classifier_head_workspace_bytes(16, 182))
    rc, lo, io = head_call(emb, w, b, ws_bytes=need - 8)
    assert rc == -1 and b"workspace" in L.effocr_head_last_error()
    assert (lo == -7.0).all() and (io == -5).all()
    # logits NULL: the ids land in the middle of a sentinel buffer, nothing else in it changes
    buf = torch.full((64,), -5, dtype=torch.int64, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = L.effocr_classifier_head(_lib.ptr(emb), 16, 384, _lib.ptr(w), _lib.ptr(b), 182, None, ctypes.c_void_p(buf.data_ptr() + 8 * 24),
                                  _lib.ptr(ws), ctypes.c_size_t(need), _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert rc == 0
    ref = torch.argmax(emb.double() @ w.double().T + b.double(), -1)
    assert torch.equal(buf[24:40], ref)
    assert (buf[:24] == -5).all() and (buf[40:] == -5).all()


E2E = [("vit_tiny_test", 64, p) for p in ("fp32", "fp16", "bf16")] + [("vit_small_patch16_224", 224, "fp16"),
       ("vit_small_patch16_224", 224, "fp32"), ("resnet18", 64, "fp32"), ("resnet18", 64, "fp16"), ("convnext_tiny", 64, "fp32"),
       ("convnext_tiny", 64, "fp16"), ("mobilenetv3_small_050", 64, "fp32"), ("mobilenetv3_small_050", 64, "fp16")]


@pytest.mark.parametrize("arch,img,prec", E2E)
def test_classifier_end_to_end_against_float64(dev, arch, img, prec):
    from classifier_ref import logits64
    from effocr_amd.classifiers import AutoClassifierFactory
    N = 997
    sd = W.init_state_dict(arch, seed=4, img_size=img, num_classes=N)
    x = torch.randn(12, 3, img, img, generator=torch.Generator().manual_seed(4))
    model = AutoClassifierFactory("timm", arch, N, precision=prec, img_size=img)()
    model.load_state_dict(sd)
    model.to(dev).eval()
    lo = model(x.to(dev))
    ids = model.predict(x.to(dev))
    model.check_status()
    assert lo.dtype == torch.float32 and lo.shape == (12, N) and lo.device == dev
    ref = logits64(arch, sd, x)
    bound = REL[prec] * (1.5 if (arch, prec) == ("mobilenetv3_small_050", "fp16") else 1.0)   # the encoder's own fp16 bound there
    rel = ((lo.cpu().double() - ref).abs().max() / ref.abs().max()).item()
    assert rel < bound, rel
    assert torch.equal(ids, torch.argmax(lo, -1))
    s = ref.sort(dim=1, descending=True).values
    stable = (s[:, 0] - s[:, 1]) > 2 * bound * ref.abs().max()
    assert stable.sum() >= 6
    assert torch.equal(ids.cpu()[stable], ref.argmax(-1)[stable])


def test_load_checkpoint_and_the_references_argmax_lines(dev, tmp_path):
    from effocr_amd.classifiers import AutoClassifierFactory
    arch, img, N = "vit_tiny_test", 64, 300
    sd = W.init_state_dict(arch, seed=8, img_size=img, num_classes=N)
    W.save_checkpoint(sd, tmp_path / "enc_best.pth")
    encoder = AutoClassifierFactory("timm", arch, n_classes=N, precision="fp32", img_size=img)
    recognizer = encoder.load(str(tmp_path / "enc_best.pth"))      # infer_effocr.py:177-179
    recognizer.to(dev)
    recognizer.eval()
    concat_char_dets = torch.randn(9, 3, img, img, generator=torch.Generator().manual_seed(2)).to(dev)
    with torch.no_grad():                                          # infer_effocr.py:329-333, verbatim
        outputs = recognizer(concat_char_dets)
        logits = outputs.logits if hasattr(outputs, 'logits') else outputs
        predictions = logits.argmax(-1)
        predlist = predictions.detach().cpu().tolist()
    assert predlist == recognizer.predict(concat_char_dets).cpu().tolist()


def test_line_recognizer_reproduces_the_references_ffnn_infer(dev):
    """tests/golden/ref_ffnn.json: the reference's own EffOCR.infer in its FFNN mode (float64 logits).  The product chain —
    LinePostprocessor, HIP crop transform, HIP encoder (fp32), HIP head + fused argmax, class map, en_postprocess — returns the same
    strings; every recorded top-2 logit gap is far above the fp32 error, so every id must agree."""
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.pipeline import ClassifierRecognizer, read_class_map
    from effocr_amd.postprocess import LinePostprocessor, LineRecognizer
    from test_ref_golden import infer_case_inputs
    with open(os.path.join(G, "ref_ffnn.json")) as f:
        meta = json.load(f)
    arr = np.load(os.path.join(G, "ref_ffnn.npz"))
    sd = W.init_state_dict(meta["arch"], seed=meta["enc_seed"], img_size=meta["size"])
    wk, bk = W.head_keys(meta["arch"])
    sd[wk], sd[bk] = torch.from_numpy(arr["head_weight"]), torch.from_numpy(arr["head_bias"])
    model = AutoClassifierFactory("timm", meta["arch"], meta["n_classes"], precision="fp32", img_size=meta["size"])()
    model.load_state_dict(sd)
    model.to(dev).eval()
    assert read_class_map(os.path.join(G, "ref_ffnn.json"))["class_map"] == meta["class_map"]   # (json.load, as the reference)
    rec = ClassifierRecognizer(model, meta["class_map"])
    n = 0
    for c in meta["infer"]:
        im, result = infer_case_inputs(c)
        post = LinePostprocessor(lang=c["lang"], vertical=c["vertical"], anchor_margin=c["anchor_margin"])
        out, nns, cb, wb = LineRecognizer(rec, post).infer(im, result)
        assert out == c["output"], (out, c["output"])
        assert nns == c["output_nns"]
        if cb is not None:
            assert [[float(v) for v in b] for b in cb] == c["char_bboxes"]
            n += len(nns)
    assert n >= 30 and any(s == "" for c in meta["infer"] for s in (c["output_nns"] or []))
