"""-m gpu: the YOLOv5 n / s / m / l / x localizers on the device against tests/yolov5_ref.py (the functional restatement of every
scale, checked against oracle/yolo_modules.py on the host) — network parity in both operand modes, determinism, batch independence,
the channel padding of n / m / x (stem, model.2), nc = 1, yolov5s bit for bit against a digest recorded before the other scales
existed, EffLocalizer from a checkpoint file and run_effocr with an n and an m localizer against the oracle driver."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from effocr_amd.localizer_engine import EffLocalizer, HipLocalizer, init_yolov5_state_dict, init_yolov5s_state_dict
from oracle import yolo_ref as Y
from tests.yolov5_ref import yolov5_forward

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "yolov5s_digest.json")
SCALES = "nsmlx"
_REF = {}


def _busy(nc, scale, seed, obj=5.5, cls=1.5):
    sd = init_yolov5_state_dict(nc, scale, seed=seed)
    for l in range(3):
        b = sd[f"model.24.m.{l}.bias"].view(3, nc + 5)
        b[:, 4] += obj
        b[:, 5:] += cls
    return sd


def _case(scale, shape, B, nc=2):
    """(state dict, input, CPU reference output), computed once per case."""
    key = (scale, shape, B, nc)
    if key not in _REF:
        sd = _busy(nc, scale, seed=1)
        x = torch.rand(B, 3, *shape, generator=torch.Generator().manual_seed(3))
        with torch.no_grad():
            _REF[key] = (sd, x, yolov5_forward(sd, x, scale))
    return _REF[key]


def _close(got, ref, box_rel, prob):
    err = (got - ref).abs()
    return (err[..., :4].max() / ref[..., :4].abs().max()).item() < box_rel and err[..., 4:].max().item() < prob


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape,B", [((640, 640), 1), ((64, 96), 3)])
def test_network_matches_reference(dev, scale, shape, B):
    """fp32 operands: boxes within 2e-4 of the input size, probabilities within 2e-4 (what yolov5s meets); deterministic; the
    im2col stem (direct_stem = 0) agrees too."""
    sd, x, ref = _case(scale, shape, B)
    eng = HipLocalizer(sd, input_shape=shape, device=dev)
    assert eng.arch == f"yolov5{scale}"
    got = eng.forward(x.to(dev)).cpu()
    assert got.shape == ref.shape == (B, eng.num_predictions, 7)
    assert _close(got, ref, 2e-4, 2e-4), ((got - ref).abs()[..., :4].max().item(), (got - ref).abs()[..., 4:].max().item())
    assert torch.equal(got, eng.forward(x.to(dev)).cpu())
    eng.set_option("direct_stem", 0)
    alt = eng.forward(x.to(dev)).cpu()
    assert _close(alt, ref, 2e-4, 2e-4)


@pytest.mark.parametrize("scale", SCALES)
def test_image_does_not_depend_on_its_batch(dev, scale):
    """An image gives the same bits alone or in a batch.  (At 64 x 96 every layer keeps its split-K choice across these batch sizes; at
    640 x 640 the deep layers' choice follows the tile count, DESIGN.md "YOLOv5 scales".)"""
    sd, x, _ = _case(scale, (64, 96), 3)
    eng = HipLocalizer(sd, input_shape=(64, 96), device=dev)
    full = eng.forward(x.to(dev)).cpu()
    for i in range(3):
        assert torch.equal(eng.forward(x[i:i + 1].to(dev)).cpu()[0], full[i])
    assert torch.equal(eng.forward(x[1:3].to(dev)).cpu(), full[1:3])


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape,B", [((640, 640), 1), ((64, 96), 3)])
def test_bf16_operands(dev, scale, shape, B):
    """precision="bf16": boxes within 1 px, probabilities within 5e-3; it is another path, and switching the option back on the same
    handle restores the exact fp32 output."""
    sd, x, ref = _case(scale, shape, B)
    eng = HipLocalizer(sd, input_shape=shape, device=dev, precision="bf16")
    got = eng.forward(x.to(dev)).cpu()
    err = (got - ref).abs()
    assert err[..., :4].max().item() < 1.0 and err[..., 4:].max().item() < 5e-3, (err[..., :4].max().item(), err[..., 4:].max().item())
    assert torch.equal(got, eng.forward(x.to(dev)).cpu())
    exact = HipLocalizer(sd, input_shape=shape, device=dev).forward(x.to(dev)).cpu()
    assert not torch.equal(got, exact)
    eng.set_option("bf16_operands", 0)
    assert torch.equal(eng.forward(x.to(dev)).cpu(), exact)


@pytest.mark.parametrize("scale", "nm")
def test_single_class(dev, scale):
    """nc = 1: 18 head channels, padded to 20 inside."""
    sd = init_yolov5_state_dict(1, scale, seed=2)
    eng = HipLocalizer(sd, input_shape=(64, 64), device=dev)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(7))
    got = eng.forward(x.to(dev)).cpu()
    with torch.no_grad():
        ref = yolov5_forward(sd, x, scale)
    assert got.shape == ref.shape == (2, 252, 6)
    assert _close(got, ref, 2e-4, 2e-4)


def test_arch_keyword_must_agree(dev):
    sd = init_yolov5_state_dict(2, "n", seed=0)
    assert HipLocalizer(sd, input_shape=(64, 64), device=dev, arch="yolov5n").arch == "yolov5n"
    with pytest.raises(ValueError, match="yolov5n"):
        HipLocalizer(sd, input_shape=(64, 64), device=dev, arch="yolov5s")


def test_yolov5s_is_bitwise_unchanged(dev):
    """The digests of tests/golden/yolov5s_digest.json were recorded on the tree before the other scales: yolov5s's output must
    still be those bytes, in both operand modes."""
    want = json.load(open(GOLDEN))["digests"]
    sd = init_yolov5s_state_dict(2, seed=0)
    for shape, B in (((640, 640), 2), ((64, 96), 3)):
        x = torch.rand(B, 3, *shape, generator=torch.Generator().manual_seed(11)).to(dev)
        for prec in ("fp32", "bf16"):
            y = HipLocalizer(sd, input_shape=shape, device=dev, precision=prec).forward(x).cpu().contiguous()
            key = f"nc2_seed0_{shape[0]}x{shape[1]}_B{B}_{prec}"
            assert list(y.shape) == want[key]["shape"]
            assert hashlib.sha256(y.numpy().tobytes()).hexdigest() == want[key]["sha256"], key


def _check_localizer(loc, images, i, got, sd, scale, conf, iou):
    """``got`` (EffLocalizer's rows for ``images[i]``) is the restated non_max_suppression of the device network's own output, row for
    row, and that output is the reference network's within the parity bounds.  The network runs on the same batch as in the call: at
    640 x 640 the split-K choice of the deep layers follows the launch's tile count, so an image's bits may depend on its batch size
    there (as for yolov5s).  (Comparing box SETS against the CPU network instead depends on boxes that sit on a threshold: a dense
    random-weight head has hundreds of them.)"""
    eng = loc._eng_net
    x = torch.cat([eng.letterbox(im, bgr=False) for im in images])
    pred = eng.forward(x)[i:i + 1].cpu()
    assert torch.equal(got, Y.non_max_suppression(pred, conf, iou, max_det=1000)[0])
    with torch.no_grad():
        ref = yolov5_forward(sd, x[i:i + 1].cpu(), scale)
    assert _close(pred, ref, 2e-4, 2e-4)


def test_efflocalizer_yolov5m_checkpoint_end_to_end(dev, tmp_path):
    """EffLocalizer(path to a yolov5m .pt): uint8 image, its file and the pre-letterboxed array give the same boxes, and they are the
    restated non_max_suppression of the network's output (same NMS rules as yolov5s), the network within the parity bounds."""
    from PIL import Image
    sd = _busy(2, "m", seed=4)
    path = tmp_path / "yolov5m_line.pt"
    torch.save(sd, path)
    loc = EffLocalizer(str(path), iou_thresh=0.3, conf_thresh=0.4, device=dev)
    assert loc._eng_net.arch == "yolov5m"
    rng = np.random.default_rng(5)
    im = (rng.integers(0, 256, (48, 400, 3)) // 64 * 64).astype(np.uint8)
    png = tmp_path / "line.png"
    Image.fromarray(im).save(png)
    pre = Y.load_localizer_img(im, (640, 640), bgr=False)
    outs = loc([im, str(png), pre])
    assert len(outs) == 3 and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert outs[0].shape[0] > 5
    _check_localizer(loc, [im, im, im], 0, outs[0], sd, "m", 0.4, 0.3)


@pytest.mark.parametrize("scale", "nm")
def test_run_effocr_with_scale(dev, scale):
    """Three 4096 x 256 lines (BASELINE configs[4]) through run_effocr with a yolov5n / yolov5m localizer: the first line's boxes are
    the restated NMS of the device network (itself within the parity bounds), and the oracle driver fed the device localizer's boxes produces the same strings (tests/test_gpu_pipeline.py
    for yolov5s)."""
    from effocr_amd.knn import FaissKNN, IndexFlatIP
    from effocr_amd.pipeline import run_effocr
    from effocr_amd.recognizer_engine import EffRecognizer
    from effocr_amd.transforms import PairedTransform
    from effocr_amd.weights import init_state_dict
    from oracle import run_effocr_ref as R
    from oracle.crop_transform_ref import paired_transform
    from oracle.encoders_ref import encoder_forward, l2_normalize

    chars = list("aenrwuosvcxzTHEQUICKBROWN-") + [chr(0x4E00 + i) for i in range(200)]
    loc_sd = init_yolov5_state_dict(2, scale, seed=2)
    for l in range(3):
        b = loc_sd[f"model.24.m.{l}.bias"].view(3, 7)
        b[:, 4] += 5.5
        b[:, 5] += 2.5
        b[:, 6] += 2.4
    loc = EffLocalizer(loc_sd, iou_thresh=0.05, conf_thresh=0.5, device=dev)
    enc_sd = init_state_dict("vit_small_patch16_224", seed=1, img_size=224)
    rec = EffRecognizer(enc_sd, arch="vit_small_patch16_224", precision="fp32", img_size=224, device=dev)
    tf = PairedTransform(size=224, device=dev)
    rng = np.random.default_rng(11)
    lines = [(rng.integers(0, 256, (256, 4096, 3)) // 32 * 32).astype(np.uint8) for _ in range(3)]
    dev_results = loc.run(lines)
    _check_localizer(loc, lines, 0, dev_results[0], loc_sd, scale, 0.5, 0.05)
    crops = []
    for im, res in zip(lines, dev_results):
        for bb in sorted(res[res[:, 5] == 0][:, :4], key=lambda x: x[0]):
            x0, _, x1, _ = torch.round(bb)
            x0, x1 = int(round(x0.item() * 4096 / 640)), int(round(x1.item() * 4096 / 640))
            c = im[0:256, x0:x1, :]
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
                               anchor_margin=0.15)
    assert list(got.keys()) == [0, 1, 2]
    for i in range(3):
        assert got[i] == want[i], (i, got[i], want[i])
    assert sum(len(w) for w in want if w) >= 5
