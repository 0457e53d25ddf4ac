"""-m gpu: the YOLO11 n / s / m / l / x localizers (libeffocr_yolo11.so) on the device against tests/yolo11_ref.py — network parity in both
operand modes, determinism, the im2col stem, batch independence in the call-size-invariant mode, nc = 1, 400 tokens, the engine choice of
EffLocalizer, a checkpoint file end to end and run_effocr with a yolo11n localizer.

Bounds.  fp32 operands: the project's YOLOv8 bound — boxes within 2e-4 of the largest reference box coordinate, scores within 2e-4 —
against the float64 restatement.  bf16 operands: 2 x the error of the CPU emulation of that mode (tests/yolo11_ref.py: bf16=True, the
roundings declared in include/effocr_yolo11.h) against float64 on the same case; the margin covers roundings flipped by the summation
order.  The cases and their seeds are tests/yolo11_ref.py's NET_CASES / make_case: tests/test_yolo11_host.py shows on the CPU that each
of seven mistakes in the attention, the positional branch, the head's shortcuts and the class branch moves every image of these cases by
10 x the fp32 bound or more.  Every parity case prints its figures (``yolo11_parity ...``); profiles/yolo11_parity.txt holds one run on
an MI355X."""
import math

import numpy as np
import pytest
import torch

from effocr_amd.localizer_engine import (EffLocalizer, HipLocalizer, HipLocalizerV8, HipLocalizerV11, init_yolo11_state_dict, init_yolov5_state_dict,
                                         init_yolov8_state_dict)
from oracle import yolo_ref as Y
from tests.yolo11_ref import BOX_REL, NET_CASES, SCORE_ABS, blocky_images, make_case, row_errors, yolo11_forward

pytestmark = pytest.mark.gpu

SCALES = "nsmlx"
_REF = {}


def _case(scale, shape, B, nc=2):
    """(state dict, input, float64 reference, errors of the float32 CPU restatement, bf16 emulation errors), computed once per case."""
    key = (scale, shape, B, nc)
    if key not in _REF:
        sd, x = make_case(scale, shape, B, nc)
        with torch.no_grad():
            ref = yolo11_forward(sd, x, scale)
            cpu32 = row_errors(yolo11_forward(sd, x, scale, dtype=torch.float32), ref)
        _REF[key] = [sd, x, ref, cpu32, None]
    return _REF[key]


def _bf16_emulation_errors(scale, shape, B):
    c = _case(scale, shape, B)
    if c[4] is None:
        with torch.no_grad():
            c[4] = row_errors(yolo11_forward(c[0], c[1], scale, bf16=True), c[2])
    return c[4]


def _check_parity(tag, scale, shape, B, got, ref, cpu32):
    dev = row_errors(got, ref)
    print(f"yolo11_parity {tag} yolo11{scale} {shape[0]}x{shape[1]} B={B}: device box {dev[0]:.3e} score {dev[1]:.3e} | "
          f"cpu fp32 box {cpu32[0]:.3e} score {cpu32[1]:.3e} | bound box {BOX_REL:.3e} score {SCORE_ABS:.3e}")
    assert torch.isfinite(got).all() and dev[0] < BOX_REL and dev[1] < SCORE_ABS, (dev, (BOX_REL, SCORE_ABS))


@pytest.mark.parametrize("scale,shape,B,nc", NET_CASES)
def test_network_matches_reference(dev, scale, shape, B, nc):
    """fp32 operands against float64; a second run gives the same bits; the im2col stem (direct_stem = 0) meets the same bound."""
    sd, x, ref, cpu32, _ = _case(scale, shape, B, nc)
    eng = HipLocalizerV11(sd, input_shape=shape, device=dev)
    assert (eng.arch, eng.scale, eng.nc, eng.no, eng.precision, eng.input_shape) == (f"yolo11{scale}", scale, nc, nc + 5, "fp32", shape)
    assert eng.num_predictions == shape[0] * shape[1] // 64 * 21 // 16
    got = eng.forward(x.to(dev)).cpu()
    assert got.shape == ref.shape == (B, eng.num_predictions, nc + 5)
    assert (got[..., 4] == 1).all()
    _check_parity("fp32", scale, shape, B, got, ref, cpu32)
    assert torch.equal(got, eng.forward(x.to(dev)).cpu())
    eng.set_option("direct_stem", 0)
    _check_parity("fp32-im2col-stem", scale, shape, B, eng.forward(x.to(dev)).cpu(), ref, cpu32)


def test_level_offsets_at_640(dev):
    """yolo11n at 640 x 640 (400 tokens): the 8400 rows and the level offsets 0 / 6400 / 8000, each level within the bound."""
    sd, x, ref, cpu32, _ = _case("n", (640, 640), 2)
    eng = HipLocalizerV11(sd, device=dev)
    assert eng.num_predictions == 8400 and eng.input_shape == (640, 640)
    got = eng.forward(x.to(dev)).cpu()
    for row0, n in ((0, 6400), (6400, 1600), (8000, 400)):
        err = (got[:, row0:row0 + n].double() - ref[:, row0:row0 + n]).abs()
        assert (err[..., :4].max() / ref[..., :4].abs().max()).item() < BOX_REL and err[..., 4:].max().item() < SCORE_ABS


@pytest.mark.parametrize("scale", SCALES)
def test_image_does_not_depend_on_its_batch(dev, scale):
    """call_size_invariant=True: an image's rows are bitwise equal at batch 1, 3 and 16 and at every position; the property reads back."""
    sd = make_case(scale, (64, 64), 1)[0]
    x = blocky_images(16, (64, 64), seed=5).to(dev)
    eng = HipLocalizerV11(sd, input_shape=(64, 64), device=dev, call_size_invariant=True)
    assert eng.call_size_invariant is True
    full = eng.forward(x).cpu()
    for i in range(16):
        assert torch.equal(eng.forward(x[i:i + 1]).cpu()[0], full[i]), i
    for i in (0, 6, 13):
        assert torch.equal(eng.forward(x[i:i + 3]).cpu(), full[i:i + 3]), i
    rolled = eng.forward(x.roll(5, 0)).cpu()
    assert torch.equal(rolled.roll(-5, 0), full)
    eng.set_option("call_size_invariant", 0)
    assert eng.call_size_invariant is False
    assert HipLocalizerV11(sd, input_shape=(64, 64), device=dev).call_size_invariant is False


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape,B", [((64, 64), 3), ((96, 160), 3)])
def test_bf16_operands(dev, scale, shape, B):
    """precision="bf16": within 2 x the error of the CPU emulation of that mode against float64; it is another path, and switching the
    option back on the same handle restores the exact fp32 output."""
    sd, x, ref, _, _ = _case(scale, shape, B)
    emu = _bf16_emulation_errors(scale, shape, B)
    eng = HipLocalizerV11(sd, input_shape=shape, device=dev, precision="bf16")
    assert eng.precision == "bf16"
    got = eng.forward(x.to(dev)).cpu()
    err = row_errors(got, ref)
    print(f"yolo11_parity bf16 yolo11{scale} {shape[0]}x{shape[1]} B={B}: device box {err[0]:.3e} score {err[1]:.3e} | "
          f"cpu bf16 emulation box {emu[0]:.3e} score {emu[1]:.3e} | ratio box {err[0] / emu[0]:.2f} score {err[1] / emu[1]:.2f} | bound 2 x the emulation")
    assert err[0] < 2 * emu[0] and err[1] < 2 * emu[1], (err, emu)
    assert torch.equal(got, eng.forward(x.to(dev)).cpu())
    exact = HipLocalizerV11(sd, input_shape=shape, device=dev).forward(x.to(dev)).cpu()
    assert not torch.equal(got, exact)
    eng.set_option("bf16_operands", 0)
    assert torch.equal(eng.forward(x.to(dev)).cpu(), exact)


def test_arch_keyword_and_engine_choice(dev):
    """EffLocalizer picks the engine from the DFL key: model.23 -> YOLO11, model.22 -> YOLOv8, neither -> YOLOv5; arch must agree with
    the tensors; the other engines refuse a YOLO11 dict with the messages they always had."""
    sd = init_yolo11_state_dict(2, "n", seed=0)
    assert HipLocalizerV11(sd, input_shape=(64, 64), device=dev, arch="yolo11n").arch == "yolo11n"
    for wrong in ("yolo11s", "yolov11n", "yolov8n", "yolov5n"):
        with pytest.raises(ValueError, match="the state dict is yolo11n"):
            EffLocalizer(sd, input_shape=(64, 64), device=dev, arch=wrong)
    loc = EffLocalizer(sd, input_shape=(64, 64), device=dev, arch="yolo11n", precision="bf16", call_size_invariant=True)
    assert type(loc._eng_net) is HipLocalizerV11 and loc._eng_net.precision == "bf16" and loc.call_size_invariant is True
    assert type(EffLocalizer(init_yolov8_state_dict(2, "n", seed=1), input_shape=(64, 64), device=dev)._eng_net) is HipLocalizerV8
    assert type(EffLocalizer(init_yolov5_state_dict(2, "n", seed=1), input_shape=(64, 64), device=dev)._eng_net) is HipLocalizer
    with pytest.raises(ValueError, match="state dict has no 'model.24.m.0.bias'"):
        HipLocalizer(sd, input_shape=(64, 64), device=dev)
    with pytest.raises(ValueError, match="not an ultralytics YOLOv8"):
        HipLocalizerV8(sd, input_shape=(64, 64), device=dev)
    m = init_yolo11_state_dict(2, "m", seed=0)
    with pytest.raises(ValueError, match="the state dict is yolo11m"):
        EffLocalizer(m, input_shape=(64, 64), device=dev, arch="yolo11l")


def test_more_tokens_than_the_cap_are_refused(dev):
    from effocr_amd._lib import EffOCRHipError
    sd = init_yolo11_state_dict(2, "n", seed=0)
    with pytest.raises(EffOCRHipError, match="1640 tokens"):
        HipLocalizerV11(sd, input_shape=(1312, 1280), device=dev)


def _shift_class_bias(sd, scores, conf, k, cls=None):
    """Adds one constant to the class biases (of class ``cls``, or of all) so that ``conf`` falls half way (in logits) between the k-th
    and the (k+1)-th largest of ``scores`` (computed with the biases as they are): a random-weight head then keeps a handful of boxes
    instead of none or all, and no candidate sits on the threshold."""
    z = torch.sort(torch.logit(scores.double().reshape(-1).clamp(1e-12, 1 - 1e-12)), descending=True).values
    shift = math.log(conf / (1 - conf)) - 0.5 * (z[k - 1].item() + z[k].item())
    for l in range(3):
        b = sd[f"model.23.cv3.{l}.2.bias"]
        if cls is None:
            b += shift
        else:
            b[cls] += shift


@pytest.mark.parametrize("scale", "ns")
def test_efflocalizer_checkpoint_end_to_end(dev, tmp_path, scale):
    """EffLocalizer(path to a yolo11 .pt): a synthetic line image as uint8 array, as file and pre-letterboxed give the same boxes; they are
    the restated non_max_suppression (oracle/yolo_ref.py) of the engine's own predictions bit for bit (the comparison
    tests/test_gpu_yolov8.py makes), and they are the boxes the CPU reference's predictions give through that NMS: as many, the same
    classes, coordinates within the fp32 box bound of the 320-pixel input and confidences within the score bound."""
    from PIL import Image
    conf, iou, shape = 0.4, 0.3, (320, 320)
    sd = init_yolo11_state_dict(2, scale, seed=4)
    rng = np.random.default_rng(5)
    im = (rng.integers(0, 256, (48, 400, 3)) // 64 * 64).astype(np.uint8)
    pre = Y.load_localizer_img(im, shape, bgr=False)
    with torch.no_grad():
        _shift_class_bias(sd, yolo11_forward(sd, torch.from_numpy(pre), scale, dtype=torch.float32)[..., 5:].max(-1).values, conf, 300)
        kept_cpu = Y.non_max_suppression(yolo11_forward(sd, torch.from_numpy(pre), scale, dtype=torch.float32), conf, iou, max_det=1000)[0]
    assert 5 <= kept_cpu.shape[0] < 1000, kept_cpu.shape
    path = tmp_path / f"yolo11{scale}_line.pt"
    torch.save(sd, path)
    loc = EffLocalizer(str(path), iou_thresh=iou, conf_thresh=conf, device=dev, input_shape=shape)
    assert type(loc._eng_net) is HipLocalizerV11 and loc._eng_net.arch == "yolo11" + scale
    png = tmp_path / "line.png"
    Image.fromarray(im).save(png)
    outs = loc([im, str(png), pre])
    assert len(outs) == 3 and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    eng = loc._eng_net
    x = torch.cat([eng.letterbox(im, bgr=False)] * 3)
    pred = eng.forward(x)[0:1].cpu()
    assert torch.equal(outs[0], Y.non_max_suppression(pred, conf, iou, max_det=1000)[0])
    assert outs[0].shape == kept_cpu.shape, (outs[0].shape, kept_cpu.shape)
    assert torch.equal(outs[0][:, 5], kept_cpu[:, 5])
    assert (outs[0][:, :4] - kept_cpu[:, :4]).abs().max().item() < BOX_REL * 320
    assert (outs[0][:, 4] - kept_cpu[:, 4]).abs().max().item() < SCORE_ABS


def test_run_effocr_with_yolo11n(dev):
    """Three 4096 x 256 lines through ONE run_effocr call with a yolo11n localizer and the vit_tiny_test recognizer: the strings are the
    ones the restated pipeline (oracle/run_effocr_ref.py) gives when fed the boxes of the CPU reference localizer (yolo11_forward in
    float32 -> the restated NMS)."""
    from effocr_amd.knn import FaissKNN, IndexFlatIP
    from effocr_amd.pipeline import run_effocr
    from effocr_amd.recognizer_engine import EffRecognizer
    from effocr_amd.transforms import PairedTransform
    from effocr_amd.weights import init_state_dict
    from oracle import run_effocr_ref as R
    from oracle.crop_transform_ref import paired_transform
    from oracle.encoders_ref import encoder_forward, l2_normalize

    conf, iou, arch, size = 0.5, 0.3, "vit_tiny_test", 64
    chars = list("aenrwuosvcxzTHEQUICKBROWN-") + [chr(0x4E00 + i) for i in range(200)]
    rng = np.random.default_rng(11)
    lines = [(rng.integers(0, 256, (256, 4096, 3)) // 32 * 32).astype(np.uint8) for _ in range(3)]
    loc_sd = init_yolo11_state_dict(2, "n", seed=2)
    pre = torch.from_numpy(np.concatenate([Y.load_localizer_img(im, (640, 640), bgr=False) for im in lines]))
    with torch.no_grad():
        scores = yolo11_forward(loc_sd, pre, "n", dtype=torch.float32)
        _shift_class_bias(loc_sd, scores[..., 5], conf, 400, cls=0)          # characters: a few hundred candidates over the three lines
        _shift_class_bias(loc_sd, scores[..., 6], conf, 30, cls=1)           # words: a few
        ref_pred = yolo11_forward(loc_sd, pre, "n", dtype=torch.float32)
    ref_results = [Y.non_max_suppression(ref_pred[i:i + 1], conf, iou, max_det=1000)[0] for i in range(3)]
    loc = EffLocalizer(loc_sd, iou_thresh=iou, conf_thresh=conf, device=dev)
    assert loc._eng_net.arch == "yolo11n"
    enc_sd = init_state_dict(arch, seed=1, img_size=size)
    rec = EffRecognizer(enc_sd, arch=arch, precision="fp32", img_size=size, device=dev)
    tf = PairedTransform(size=size, device=dev)
    crops = []
    for im, res in zip(lines, ref_results):
        for bb in sorted(res[res[:, 5] == 0][:, :4], key=lambda x: x[0]):
            x0, _, x1, _ = torch.round(bb)
            x0, x1 = int(round(x0.item() * 4096 / 640)), int(round(x1.item() * 4096 / 640))
            c = im[0:256, max(x0, 0):x1, :]
            if c.shape[1] > 0:
                crops.append(c)
    keep = crops[:48]
    assert len(keep) >= 5, len(keep)
    xs = torch.stack([torch.from_numpy(np.asarray(paired_transform(c, size=size), dtype=np.float32)) for c in keep])
    emb = l2_normalize(encoder_forward(arch, enc_sd, xs)).numpy()
    distract = np.random.default_rng(5).standard_normal((len(chars) - emb.shape[0], emb.shape[1])).astype(np.float32)
    distract /= np.linalg.norm(distract, axis=1, keepdims=True)
    index = np.concatenate([emb, distract]).astype(np.float32)
    knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False, device=dev)
    knn.train(torch.from_numpy(index))
    got, _ = run_effocr(lines, loc, rec, tf, "en", knn_func=knn, candidate_chars=chars, anchor_margin=0.15)
    want, _ = R.run_effocr_ref(lines, loc_sd, arch, enc_sd, index, chars, "en", localizer_results=ref_results, anchor_margin=0.15,
                               conf_thresh=conf, iou_thresh=iou, size=size)
    assert list(got.keys()) == [0, 1, 2]
    for i in range(3):
        assert got[i] == want[i], (i, got[i], want[i])
    assert sum(len(w) for w in want if w) >= 5
