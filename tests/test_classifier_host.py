"""-m "not gpu": the FFNN classifier's host side — timm head tables, checkpoints, the float64 restatement, the ClassifierRecognizer
glue against the reference's recorded FFNN runs, and libeffocr_head.so's ABI and argument checks (no GPU needed for any of them)."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from effocr_amd import _lib
from effocr_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
ARCHS = [("resnet18", 32), ("vit_small_patch16_224", 224), ("vit_base_patch16_224", 224), ("vit_tiny_test", 64),
         ("convnext_tiny", 32), ("mobilenetv3_small_050", 32)]


def learnable(arch, n, img=224):
    return sum(math.prod(s) for k, s in W.param_shapes(arch, img, num_classes=n).items() if not k.endswith(("running_mean", "running_var")))


@pytest.mark.parametrize("arch,total", [("resnet18", 11_689_512), ("vit_small_patch16_224", 22_050_664),
                                        ("vit_base_patch16_224", 86_567_656), ("convnext_tiny", 28_589_128)])
def test_head_tables_match_timms_published_totals(arch, total):
    assert learnable(arch, 1000) == total


def test_mobilenetv3_head_is_the_builders_classifier():
    assert learnable("mobilenetv3_small_050", 1000) == W.mobilenetv3_num_learnable("mobilenetv3_small_050", 1000)
    assert W.param_shapes("mobilenetv3_small_050", num_classes=10) == W._mobilenetv3_shapes("mobilenetv3_small_050", 10)


@pytest.mark.parametrize("arch,img", ARCHS)
def test_head_keys_shapes_and_num_classes(arch, img):
    sd = W.init_state_dict(arch, seed=2, img_size=img, num_classes=37)
    wk, bk = W.head_keys(arch)
    assert list(sd)[-2:] == [wk, bk]
    assert tuple(sd[wk].shape) == (37, W.embed_dim(arch)) and tuple(sd[bk].shape) == (37,)
    assert W.infer_num_classes(sd) == 37 and W.infer_num_classes({"net." + k: v for k, v in sd.items()}) == 37
    plain = W.init_state_dict(arch, seed=2, img_size=img)
    assert W.infer_num_classes(plain) == 0
    # the encoder's seeded stream is the same with and without a head
    assert list(plain) == list(sd)[:-2] and all(torch.equal(plain[k], sd[k]) for k in plain)
    W.check_state_dict(arch, sd, img, num_classes=37)
    W.check_state_dict(arch, sd, img)                     # a head is allowed where none is asked for
    with pytest.raises(ValueError, match="missing"):
        W.check_state_dict(arch, plain, img, num_classes=37)
    with pytest.raises(ValueError, match="shape"):
        W.check_state_dict(arch, sd, img, num_classes=36)
    assert W.infer_arch(sd) == arch or arch in ("vit_tiny_test",)


def test_head_init_has_its_own_stream():
    a = W.init_head("vit_small_patch16_224", 50, seed=1)
    b = W.init_head("vit_small_patch16_224", 50, seed=1)
    c = W.init_head("vit_small_patch16_224", 50, seed=2)
    assert torch.equal(a["head.weight"], b["head.weight"]) and not torch.equal(a["head.weight"], c["head.weight"])
    assert abs(a["head.weight"].std().item() * 384 ** 0.5 - 1) < 0.05


def test_checkpoint_round_trip_with_net_keys(tmp_path):
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.encoders import AutoEncoderFactory
    arch, img, N = "vit_tiny_test", 64, 12
    sd = W.init_state_dict(arch, seed=5, img_size=img, num_classes=N)
    W.save_checkpoint(sd, tmp_path / "enc_best.pth")
    raw = torch.load(tmp_path / "enc_best.pth", weights_only=True)
    assert all(k.startswith("net.") for k in raw) and "net.head.weight" in raw
    m = AutoClassifierFactory("timm", arch, N, img_size=img).load(str(tmp_path / "enc_best.pth"))
    assert all(torch.equal(m.state_dict()["net." + k], v) for k, v in sd.items())
    assert sum(p.numel() for p in m.parameters()) == learnable(arch, N, img)
    assert {k for k, _ in m.named_parameters()} == {"net." + k for k in sd}
    # an encoder checkpoint that carries a head still loads as an encoder, as before
    enc = AutoEncoderFactory("timm", arch, img_size=img).load(str(tmp_path / "enc_best.pth"))
    assert "net.head.weight" in enc.state_dict()
    # a classifier refuses a checkpoint without a head, or with another class count
    W.save_checkpoint(W.init_state_dict(arch, seed=5, img_size=img), tmp_path / "nohead.pth")
    with pytest.raises(ValueError):
        AutoClassifierFactory("timm", arch, N, img_size=img).load(str(tmp_path / "nohead.pth"))
    with pytest.raises(ValueError):
        AutoClassifierFactory("timm", arch, N + 1, img_size=img).load(str(tmp_path / "enc_best.pth"))


def test_unsupported_backends_and_archs_raise():
    from effocr_amd.classifiers import AutoClassifierFactory
    with pytest.raises(NotImplementedError):
        AutoClassifierFactory("hf", "microsoft/beit-base-patch16-224", 10)
    with pytest.raises(NotImplementedError):
        AutoClassifierFactory("timm", "xcit_small_12_p8_224", 10)
    with pytest.raises(ValueError):
        AutoClassifierFactory("timm", "resnet18", 0)


@pytest.mark.parametrize("arch,img", [a for a in ARCHS if a[0] != "vit_base_patch16_224"])
def test_float64_restatement_equals_an_nn_module_tree(arch, img):
    """classifier_ref.logits64 (encoder restatement, then the head) against a torch.nn.Module tree: the same encoder restatement
    wrapped as a module, followed by an nn.Linear loaded strict=True from timm's head keys."""
    from classifier_ref import embedding64, logits64
    N = 19
    sd = W.init_state_dict(arch, seed=6, img_size=img, num_classes=N)
    wk, bk = W.head_keys(arch)

    class Enc(torch.nn.Module):
        def forward(self, x):
            return embedding64(arch, sd, x)
    net = torch.nn.Sequential(Enc(), torch.nn.Linear(W.embed_dim(arch), N).double())
    net[1].load_state_dict({"weight": sd[wk], "bias": sd[bk]}, strict=True)
    x = torch.randn(2, 3, img, img, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        want = net(x.double())
    got = logits64(arch, sd, x)
    assert got.dtype == torch.float64 and torch.allclose(got, want, rtol=1e-12, atol=1e-12)


class _RecordedClassifier:
    """Stands in for AutoClassifier: predict() = argmax of the logits the reference's run produced for this line."""
    img_size = 224

    def __init__(self):
        self.logits = None

    def predict(self, crops):
        assert crops.shape[0] == self.logits.shape[0]
        return torch.from_numpy(self.logits).argmax(-1)


class _ZeroTransform:
    def boxes(self, image, boxes, already_int=False):
        return torch.zeros(len(boxes), 3, 8, 8)


def test_classifier_recognizer_glue_reproduces_the_references_ffnn_infer():
    from effocr_amd.pipeline import ClassifierRecognizer, read_class_map
    from effocr_amd.postprocess import LinePostprocessor, LineRecognizer
    from test_ref_golden import infer_case_inputs
    meta = read_class_map(os.path.join(G, "ref_ffnn.json"))              # (plain json.load)
    arr = np.load(os.path.join(G, "ref_ffnn.npz"))
    clf = _RecordedClassifier()
    rec = ClassifierRecognizer(clf, meta["class_map"])
    assert rec.recongizer_encoder is clf
    spaces = 0
    for ci, c in enumerate(meta["infer"]):
        im, result = infer_case_inputs(c)
        clf.logits = arr[f"logits_{ci}"] if f"logits_{ci}" in arr else None
        post = LinePostprocessor(lang=c["lang"], vertical=c["vertical"], anchor_margin=c["anchor_margin"])
        out, nns, cb, wb = LineRecognizer(rec, post, char_transform=_ZeroTransform()).infer(im, result)
        assert (out, nns) == (c["output"], c["output_nns"])
        if cb is not None:
            assert [[float(v) for v in b] for b in cb] == c["char_bboxes"]
            assert clf.logits.argmax(-1).tolist() == c["ids"]
            spaces += nns.count("")
    assert spaces >= 1
    clf.logits = arr["logits_0"]
    cmap = dict(meta["class_map"])
    del cmap[str(meta["space_id"])]
    with pytest.raises(KeyError):
        ClassifierRecognizer(clf, cmap)(torch.zeros(clf.logits.shape[0], 3, 8, 8))


# -- libeffocr_head.so -------------------------------------------------------------------------------------------------------
def test_head_library_exports_its_header_and_versions_agree():
    src = open(os.path.join(ROOT, "include", "effocr_head.h")).read()
    declared = sorted(set(re.findall(r"\b(effocr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert len(declared) == 4
    raw = ctypes.CDLL(_lib.HEAD_SO_PATH)
    for n in declared:
        assert hasattr(raw, n), f"{n} declared in effocr_head.h but not exported"
    assert sorted(_lib.HEAD_EXPORTS) == declared
    v = int(re.search(r"#define\s+EFFOCR_HEAD_ABI_VERSION\s+(\d+)", src).group(1))
    assert _lib.head_lib().effocr_head_abi_version() == v == _lib.HEAD_ABI_VERSION
    _lib.lib()
    assert not set(declared) & set(_lib.EXPORTS)                       # the product library's ABI is untouched
    assert not hasattr(ctypes.CDLL(_lib.SO_PATH), "effocr_classifier_head")


def test_product_library_stays_under_its_cap():
    assert os.path.getsize(os.path.join(ROOT, "effocr_amd", "libeffocr_hip.so")) < 7.2e6


def test_head_argument_checks_without_a_gpu():
    L = _lib.head_lib()
    p = ctypes.c_void_p(4096)                                          # never dereferenced: every call below is refused first
    assert L.effocr_classifier_head_workspace_bytes(16, 30813) == 16 * 482 * 8
    assert L.effocr_classifier_head_workspace_bytes(0, 10) == 0

    def call(B=4, d=384, N=10, lo=p, ids=p, ws=p, nb=1 << 20, emb=p, w=p):
        return L.effocr_classifier_head(emb, B, d, w, p, N, lo, ids, ws, ctypes.c_size_t(nb), None)
    for kw, msg in [(dict(d=382), b"multiple of 4"), (dict(d=4100), b"multiple of 4"), (dict(d=0), b"multiple of 4"),
                    (dict(N=0), b"n_classes"), (dict(B=-1), b"batch"), (dict(lo=None, ids=None), b"both NULL"),
                    (dict(N=200, nb=8), b"workspace"), (dict(N=10, nb=8), b"workspace"), (dict(emb=ctypes.c_void_p(4100)), b"aligned"),
                    (dict(w=None), b"NULL")]:
        assert call(**kw) == -1, kw
        assert msg in L.effocr_head_last_error(), (kw, L.effocr_head_last_error())
    assert call(B=0) == 0                                               # an empty batch is a valid call that launches nothing
