"""-m gpu: the YOLOv8 n / s / m / l / x localizers (libeffocr_yolov8.so) on the device against tests/yolov8_ref.py — network parity in
both operand modes, determinism, the im2col stem, batch independence in the call-size-invariant mode, nc = 1, the engine choice of
EffLocalizer, a checkpoint file end to end and run_effocr with a yolov8n localizer against the oracle driver.

Bounds.  fp32 operands: the bound the YOLOv5 scales meet with the same convolutions — boxes within 2e-4 of the largest reference box
coordinate, scores within 2e-4 — against the float64 restatement; where the float32 CPU restatement's own error against float64 exceeds
a quarter of that for a case, the case's bound is 4 x the CPU error (measured: it never does, profiles/yolov8_parity.txt).  bf16
operands: 2 x the error of the CPU emulation of that mode (tests/yolov8_ref.py: bf16=True) against float64 on the same case; the margin
covers roundings flipped by the summation order.  Every parity case prints its figures (``yolov8_parity ...``); profiles/yolov8_parity.txt
holds one run on an MI355X."""
import math

import numpy as np
import pytest
import torch

from effocr_amd.localizer_engine import (EffLocalizer, HipLocalizer, HipLocalizerV8, init_yolov5_state_dict, init_yolov8_state_dict)
from oracle import yolo_ref as Y
from tests.yolov8_ref import yolov8_forward

pytestmark = pytest.mark.gpu

SCALES = "nsmlx"
SHAPES = [((32, 32), 1), ((64, 96), 3), ((96, 160), 2)]      # one-pixel top level | non-square (an x / y swap) | odd 3 x 5 top level
BOX_REL, SCORE_ABS = 2e-4, 2e-4
_REF = {}


def _errors(got, ref):
    """(largest box error relative to the largest reference box coordinate, largest score error)."""
    err = (got.double() - ref).abs()
    return (err[..., :4].max() / ref[..., :4].abs().max()).item(), err[..., 4:].max().item()


def _case(scale, shape, B, nc=2):
    """(state dict, input, float64 reference, errors of the float32 CPU restatement), computed once per case."""
    key = (scale, shape, B, nc)
    if key not in _REF:
        sd = init_yolov8_state_dict(nc, scale, seed=1)
        x = torch.rand(B, 3, *shape, generator=torch.Generator().manual_seed(3))
        with torch.no_grad():
            ref = yolov8_forward(sd, x, scale)
            cpu32 = _errors(yolov8_forward(sd, x, scale, dtype=torch.float32), ref)
        _REF[key] = [sd, x, ref, cpu32, None]
    return _REF[key]


def _bf16_emulation_errors(scale, shape, B):
    c = _case(scale, shape, B)
    if c[4] is None:
        with torch.no_grad():
            c[4] = _errors(yolov8_forward(c[0], c[1], scale, bf16=True), c[2])
    return c[4]


def _bounds(cpu32):
    """The fixed bound, or 4 x the float32 CPU restatement's own error where that exceeds a quarter of it."""
    return (4 * cpu32[0] if cpu32[0] > BOX_REL / 4 else BOX_REL), (4 * cpu32[1] if cpu32[1] > SCORE_ABS / 4 else SCORE_ABS)


def _check_parity(tag, scale, shape, B, got, ref, cpu32):
    dev = _errors(got, ref)
    bound = _bounds(cpu32)
    print(f"yolov8_parity {tag} yolov8{scale} {shape[0]}x{shape[1]} B={B}: device box {dev[0]:.3e} score {dev[1]:.3e} | "
          f"cpu fp32 box {cpu32[0]:.3e} score {cpu32[1]:.3e} | bound box {bound[0]:.3e} score {bound[1]:.3e}")
    assert dev[0] < bound[0] and dev[1] < bound[1], (dev, bound)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape,B", SHAPES)
def test_network_matches_reference(dev, scale, shape, B):
    """fp32 operands against float64 (bounds: module docstring); a second run gives the same bits; the im2col stem (direct_stem = 0)
    meets the same bound."""
    sd, x, ref, cpu32, _ = _case(scale, shape, B)
    eng = HipLocalizerV8(sd, input_shape=shape, device=dev)
    assert (eng.arch, eng.scale, eng.nc, eng.no, eng.precision, eng.input_shape) == (f"yolov8{scale}", scale, 2, 7, "fp32", shape)
    assert eng.num_predictions == shape[0] * shape[1] // 64 * 21 // 16
    got = eng.forward(x.to(dev)).cpu()
    assert got.shape == ref.shape == (B, eng.num_predictions, 7)
    assert (got[..., 4] == 1).all()
    _check_parity("fp32", scale, shape, B, got, ref, cpu32)
    assert torch.equal(got, eng.forward(x.to(dev)).cpu())
    eng.set_option("direct_stem", 0)
    _check_parity("fp32-im2col-stem", scale, shape, B, eng.forward(x.to(dev)).cpu(), ref, cpu32)


def test_network_matches_reference_at_640(dev):
    """yolov8n at 640 x 640: the 8400 rows and the level offsets 0 / 6400 / 8000."""
    sd, x, ref, cpu32, _ = _case("n", (640, 640), 1)
    eng = HipLocalizerV8(sd, device=dev)
    assert eng.num_predictions == 8400 and eng.input_shape == (640, 640)
    got = eng.forward(x.to(dev)).cpu()
    _check_parity("fp32", "n", (640, 640), 1, got, ref, cpu32)
    for row0, n in ((0, 6400), (6400, 1600), (8000, 400)):
        assert _errors(got[:, row0:row0 + n], ref[:, row0:row0 + n])[0] < _bounds(cpu32)[0]
    assert torch.equal(got, eng.forward(x.to(dev)).cpu())


@pytest.mark.parametrize("scale", SCALES)
def test_image_does_not_depend_on_its_batch(dev, scale):
    """call_size_invariant=True: image i of a batch equals the single-image call bit for bit; the property reads back."""
    sd, x, _, _, _ = _case(scale, (64, 96), 3)
    eng = HipLocalizerV8(sd, input_shape=(64, 96), device=dev, call_size_invariant=True)
    assert eng.call_size_invariant is True
    full = eng.forward(x.to(dev)).cpu()
    for i in range(3):
        assert torch.equal(eng.forward(x[i:i + 1].to(dev)).cpu()[0], full[i])
    assert torch.equal(eng.forward(x[1:3].to(dev)).cpu(), full[1:3])
    eng.set_option("call_size_invariant", 0)
    assert eng.call_size_invariant is False
    assert HipLocalizerV8(sd, input_shape=(64, 96), device=dev).call_size_invariant is False


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape,B", [((64, 96), 3), ((96, 160), 2)])
def test_bf16_operands(dev, scale, shape, B):
    """precision="bf16": within 2 x the error of the CPU emulation of that mode against float64; it is another path, and switching the
    option back on the same handle restores the exact fp32 output."""
    sd, x, ref, _, _ = _case(scale, shape, B)
    emu = _bf16_emulation_errors(scale, shape, B)
    eng = HipLocalizerV8(sd, input_shape=shape, device=dev, precision="bf16")
    assert eng.precision == "bf16"
    got = eng.forward(x.to(dev)).cpu()
    err = _errors(got, ref)
    print(f"yolov8_parity bf16 yolov8{scale} {shape[0]}x{shape[1]} B={B}: device box {err[0]:.3e} score {err[1]:.3e} | "
          f"cpu bf16 emulation box {emu[0]:.3e} score {emu[1]:.3e} | bound 2 x the emulation")
    assert err[0] < 2 * emu[0] and err[1] < 2 * emu[1], (err, emu)
    assert torch.equal(got, eng.forward(x.to(dev)).cpu())
    exact = HipLocalizerV8(sd, input_shape=shape, device=dev).forward(x.to(dev)).cpu()
    assert not torch.equal(got, exact)
    eng.set_option("bf16_operands", 0)
    assert torch.equal(eng.forward(x.to(dev)).cpu(), exact)


@pytest.mark.parametrize("scale", "nx")
def test_single_class(dev, scale):
    """nc = 1: one class logit per anchor, padded to 4 channels inside; rows of 6."""
    sd = init_yolov8_state_dict(1, scale, seed=2)
    eng = HipLocalizerV8(sd, input_shape=(64, 64), device=dev)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(7))
    got = eng.forward(x.to(dev)).cpu()
    with torch.no_grad():
        ref = yolov8_forward(sd, x, scale)
        cpu32 = _errors(yolov8_forward(sd, x, scale, dtype=torch.float32), ref)
    assert got.shape == ref.shape == (2, 84, 6) and eng.nc == 1 and eng.no == 6
    _check_parity("fp32-nc1", scale, (64, 64), 2, got, ref, cpu32)


def test_arch_keyword_must_agree(dev):
    sd = init_yolov8_state_dict(2, "n", seed=0)
    assert HipLocalizerV8(sd, input_shape=(64, 64), device=dev, arch="yolov8n").arch == "yolov8n"
    with pytest.raises(ValueError, match="yolov8n"):
        HipLocalizerV8(sd, input_shape=(64, 64), device=dev, arch="yolov8s")
    with pytest.raises(ValueError, match="yolov8n"):
        EffLocalizer(sd, input_shape=(64, 64), device=dev, arch="yolov5n")
    assert EffLocalizer(sd, input_shape=(64, 64), device=dev, arch="yolov8n")._eng_net.arch == "yolov8n"


def test_yolov5_dicts_keep_their_engine(dev):
    """A YOLOv5 dict still builds a HipLocalizer, EffLocalizer picks it for such a dict and gives what the bare engine gives; a YOLOv8
    dict is refused by HipLocalizer with the message it always had."""
    v5 = init_yolov5_state_dict(2, "n", seed=1)
    loc = EffLocalizer(v5, input_shape=(64, 96), device=dev)
    assert type(loc._eng_net) is HipLocalizer and loc._eng_net.arch == "yolov5n"
    x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(3)).to(dev)
    assert torch.equal(loc._eng_net.forward(x), HipLocalizer(v5, input_shape=(64, 96), device=dev).forward(x))
    v8 = init_yolov8_state_dict(2, "n", seed=1)
    assert type(EffLocalizer(v8, input_shape=(64, 96), device=dev)._eng_net) is HipLocalizerV8
    with pytest.raises(ValueError, match="state dict has no 'model.24.m.0.bias'"):
        HipLocalizer(v8, input_shape=(64, 96), device=dev)


def _shift_class_bias(sd, scores, conf, k, cls=None):
    """Adds one constant to the class biases (of class ``cls``, or of all) so that the k-th largest of ``scores`` (computed with the
    biases as they are) lands on ``conf``: a random-weight head then keeps a handful of boxes instead of none or all."""
    z = torch.logit(scores.double().reshape(-1).clamp(1e-12, 1 - 1e-12))
    shift = math.log(conf / (1 - conf)) - torch.sort(z, descending=True).values[k].item()
    for l in range(3):
        b = sd[f"model.22.cv3.{l}.2.bias"]
        if cls is None:
            b += shift
        else:
            b[cls] += shift


def test_efflocalizer_yolov8m_checkpoint_end_to_end(dev, tmp_path):
    """EffLocalizer(path to a yolov8m .pt): uint8 image, its file and the pre-letterboxed array give the same boxes, and they are the
    restated non_max_suppression (oracle/yolo_ref.py) of the engine's own predictions, bit for bit.  The class bias is chosen on the CPU
    restatement so that it keeps at least 5 and fewer than max_det boxes."""
    from PIL import Image
    conf, iou, shape = 0.4, 0.3, (320, 320)
    sd = init_yolov8_state_dict(2, "m", seed=4)
    rng = np.random.default_rng(5)
    im = (rng.integers(0, 256, (48, 400, 3)) // 64 * 64).astype(np.uint8)
    pre = Y.load_localizer_img(im, shape, bgr=False)
    with torch.no_grad():
        _shift_class_bias(sd, yolov8_forward(sd, torch.from_numpy(pre), "m", dtype=torch.float32)[..., 5:].max(-1).values, conf, 500)
        kept_cpu = Y.non_max_suppression(yolov8_forward(sd, torch.from_numpy(pre), "m", dtype=torch.float32), conf, iou, max_det=1000)[0]
    assert 5 <= kept_cpu.shape[0] < 1000, kept_cpu.shape
    path = tmp_path / "yolov8m_line.pt"
    torch.save(sd, path)
    loc = EffLocalizer(str(path), iou_thresh=iou, conf_thresh=conf, device=dev, input_shape=shape)
    assert type(loc._eng_net) is HipLocalizerV8 and loc._eng_net.arch == "yolov8m"
    png = tmp_path / "line.png"
    Image.fromarray(im).save(png)
    outs = loc([im, str(png), pre])
    assert len(outs) == 3 and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    eng = loc._eng_net
    x = torch.cat([eng.letterbox(im, bgr=False)] * 3)
    pred = eng.forward(x)[0:1].cpu()
    assert torch.equal(outs[0], Y.non_max_suppression(pred, conf, iou, max_det=1000)[0])
    assert 5 <= outs[0].shape[0] < 1000


def test_run_effocr_with_yolov8n(dev):
    """Three 4096 x 256 lines through run_effocr with a yolov8n localizer: the first line's boxes are the restated NMS of the device
    network's own predictions, and the oracle driver fed the device localizer's boxes produces the same strings (as
    tests/test_gpu_yolov5_scales.py::test_run_effocr_with_scale for YOLOv5)."""
    from effocr_amd.knn import FaissKNN, IndexFlatIP
    from effocr_amd.pipeline import run_effocr
    from effocr_amd.recognizer_engine import EffRecognizer
    from effocr_amd.transforms import PairedTransform
    from effocr_amd.weights import init_state_dict
    from oracle import run_effocr_ref as R
    from oracle.crop_transform_ref import paired_transform
    from oracle.encoders_ref import encoder_forward, l2_normalize

    conf, iou = 0.5, 0.3
    chars = list("aenrwuosvcxzTHEQUICKBROWN-") + [chr(0x4E00 + i) for i in range(200)]
    rng = np.random.default_rng(11)
    lines = [(rng.integers(0, 256, (256, 4096, 3)) // 32 * 32).astype(np.uint8) for _ in range(3)]
    loc_sd = init_yolov8_state_dict(2, "n", seed=2)
    probe = HipLocalizerV8(loc_sd, device=dev)
    scores = probe.forward(torch.cat([probe.letterbox(im, bgr=False) for im in lines])).cpu()
    _shift_class_bias(loc_sd, scores[..., 5], conf, 400, cls=0)          # characters: a few hundred candidates over the three lines
    _shift_class_bias(loc_sd, scores[..., 6], conf, 30, cls=1)           # words: a few
    loc = EffLocalizer(loc_sd, iou_thresh=iou, conf_thresh=conf, device=dev)
    assert loc._eng_net.arch == "yolov8n"
    enc_sd = init_state_dict("vit_small_patch16_224", seed=1, img_size=224)
    rec = EffRecognizer(enc_sd, arch="vit_small_patch16_224", precision="fp32", img_size=224, device=dev)
    tf = PairedTransform(size=224, device=dev)
    dev_results = loc.run(lines)
    eng = loc._eng_net
    pred = eng.forward(torch.cat([eng.letterbox(im, bgr=False) for im in lines]))[0:1].cpu()
    assert torch.equal(dev_results[0], Y.non_max_suppression(pred, conf, iou, max_det=1000)[0])
    crops = []
    for im, res in zip(lines, dev_results):
        for bb in sorted(res[res[:, 5] == 0][:, :4], key=lambda x: x[0]):
            x0, _, x1, _ = torch.round(bb)
            x0, x1 = int(round(x0.item() * 4096 / 640)), int(round(x1.item() * 4096 / 640))
            c = im[0:256, max(x0, 0):x1, :]
            if c.shape[1] > 0:
                crops.append(c)
    keep = crops[:48]
    assert len(keep) >= 5, len(keep)
    xs = torch.stack([torch.from_numpy(np.asarray(paired_transform(c, size=224), dtype=np.float32)) for c in keep])
    emb = l2_normalize(encoder_forward("vit_small_patch16_224", enc_sd, xs)).numpy()
    distract = np.random.default_rng(5).standard_normal((len(chars) - emb.shape[0], emb.shape[1])).astype(np.float32)
    distract /= np.linalg.norm(distract, axis=1, keepdims=True)
    index = np.concatenate([emb, distract]).astype(np.float32)
    knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False, device=dev)
    knn.train(torch.from_numpy(index))
    got, _ = run_effocr(lines, loc, rec, tf, "en", knn_func=knn, candidate_chars=chars, anchor_margin=0.15)
    want, _ = R.run_effocr_ref(lines, loc_sd, "vit_small_patch16_224", enc_sd, index, chars, "en", localizer_results=dev_results,
                               anchor_margin=0.15, conf_thresh=conf, iou_thresh=iou)
    assert list(got.keys()) == [0, 1, 2]
    for i in range(3):
        assert got[i] == want[i], (i, got[i], want[i])
    assert sum(len(w) for w in want if w) >= 5
