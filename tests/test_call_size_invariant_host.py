"""Call-size-invariant mode, host side (no GPU): the library option on the three kinds of handle, and the ``call_size_invariant`` keyword
on its way from every factory to the handle.  Creating a handle and setting an option touch host memory only; the engines' device work
(require_gpu, the weight blob, streams) is replaced by a recording stand-in for the library, so what is asserted is the call each
constructor makes."""
import contextlib
import ctypes

import pytest
import torch

from effocr_amd import _lib
from effocr_amd import encoders as E
from effocr_amd.weights import init_state_dict

OPTION = b"call_size_invariant"


def _encoder(L, arch, img):
    h = ctypes.c_void_p()
    assert L.effocr_encoder_create(arch.encode(), img, _lib.PREC["fp16"], ctypes.byref(h)) == 0, L.effocr_last_error()
    return h


@pytest.mark.parametrize("arch,img", [("vit_small_patch16_224", 224), ("resnet18", 32)])
def test_encoder_option(hip_lib, arch, img):
    h = _encoder(hip_lib, arch, img)
    try:
        assert hip_lib.effocr_encoder_set_option(h, OPTION, 1) == 0, hip_lib.effocr_last_error()
        assert hip_lib.effocr_encoder_set_option(h, OPTION, 0) == 0, hip_lib.effocr_last_error()
        for bad in (2, -1):
            assert hip_lib.effocr_encoder_set_option(h, OPTION, bad) == -1            # EFFOCR_EINVAL
            assert hip_lib.effocr_last_error().decode() == "set_option: call_size_invariant must be 0 or 1"
        # the workspace a caller allocates is the same in both modes (the scratch sizing does not move with the option)
        sizes = [hip_lib.effocr_encoder_workspace_bytes(h, b) for b in (1, 6, 64)]
        assert hip_lib.effocr_encoder_set_option(h, OPTION, 1) == 0
        assert [hip_lib.effocr_encoder_workspace_bytes(h, b) for b in (1, 6, 64)] == sizes
    finally:
        hip_lib.effocr_encoder_destroy(h)


def test_localizer_option(hip_lib):
    h = ctypes.c_void_p()
    assert hip_lib.effocr_localizer_create(b"yolov5s", 2, 320, 320, ctypes.byref(h)) == 0, hip_lib.effocr_last_error()
    try:
        assert hip_lib.effocr_localizer_set_option(h, OPTION, 1) == 0, hip_lib.effocr_last_error()
        assert hip_lib.effocr_localizer_set_option(h, OPTION, 0) == 0, hip_lib.effocr_last_error()
        assert hip_lib.effocr_localizer_set_option(h, OPTION, 2) == -1
        assert hip_lib.effocr_last_error().decode() == "localizer_set_option: call_size_invariant must be 0 or 1"
    finally:
        hip_lib.effocr_localizer_destroy(h)


class _Recorder:
    """Stands in for a loaded library: every entry point returns 0 (no parameters, no weight bytes) and is recorded by name."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn

    def options(self, entry):
        return [(a[1], a[2]) for n, a in self.calls if n == entry]


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "require_gpu", lambda device=None: torch.device("cpu"))
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    for loader in ("lib", "swin_lib", "resnet_lib", "mnv3_lib", "effnet_lib"):
        monkeypatch.setattr(_lib, loader, lambda rec=rec: rec)
    return rec


ENC_OPT = "effocr_encoder_set_option"
ON = [(OPTION, 1)]


@pytest.mark.parametrize("arch,img", [("vit_small_patch16_224", 224), ("vit_base_patch16_224", 224), ("resnet18", 32)])
def test_keyword_reaches_the_encoder_handle(recorder, arch, img):
    sd = init_state_dict(arch, seed=0, img_size=img)
    enc = E.HipEncoder(arch, sd, img_size=img)
    assert recorder.options(ENC_OPT) == [] and enc.call_size_invariant is False          # off by default: the handle is not touched
    enc = E.HipEncoder(arch, sd, img_size=img, call_size_invariant=True)
    assert recorder.options(ENC_OPT) == ON and enc.call_size_invariant is True
    enc.set_option("call_size_invariant", 0)
    assert recorder.options(ENC_OPT) == ON + [(OPTION, 0)] and enc.call_size_invariant is False
    with pytest.raises(AttributeError):
        enc.call_size_invariant = True                                                    # read-only
    del recorder.calls[:]
    enc = E.make_encoder(arch, sd, img_size=img, call_size_invariant=True)
    assert recorder.options(ENC_OPT) == ON and enc.call_size_invariant is True


def test_keyword_through_the_factories(recorder, monkeypatch):
    from effocr_amd import recognizer_engine as RE
    from effocr_amd.classifiers import AutoClassifierFactory
    arch, img = "resnet18", 32
    auto = E.AutoEncoderFactory("timm", arch, img_size=img, call_size_invariant=True)(device="cpu")
    assert auto.call_size_invariant is True and recorder.options(ENC_OPT) == ON
    assert E.AutoEncoderFactory("timm", arch, img_size=img)(device="cpu").call_size_invariant is False
    del recorder.calls[:]
    clf = AutoClassifierFactory("timm", arch, 7, img_size=img, call_size_invariant=True)(device="cpu")
    assert clf.call_size_invariant is True and recorder.options(ENC_OPT) == ON
    del recorder.calls[:]
    monkeypatch.setattr(RE, "_Lane", lambda device: object())                             # (a lane owns a HIP stream)
    sd = init_state_dict(arch, seed=0, img_size=img)
    rec = RE.EffRecognizer(sd, arch=arch, img_size=img, call_size_invariant=True)
    assert rec.call_size_invariant is True and recorder.options(ENC_OPT) == ON
    assert RE.EffRecognizer(sd, arch=arch, img_size=img).call_size_invariant is False


def test_keyword_reaches_the_localizer_handle(recorder):
    from effocr_amd.localizer_engine import EffLocalizer, HipLocalizer, init_yolov5s_state_dict
    sd = init_yolov5s_state_dict(2, seed=0)
    entry = "effocr_localizer_set_option"
    loc = HipLocalizer(sd, input_shape=(320, 320))
    assert loc.call_size_invariant is False and (OPTION, 1) not in recorder.options(entry)
    loc = HipLocalizer(sd, input_shape=(320, 320), call_size_invariant=True)
    assert loc.call_size_invariant is True and recorder.options(entry)[-1] == (OPTION, 1)
    del recorder.calls[:]
    eff = EffLocalizer(sd, input_shape=(320, 320), call_size_invariant=True)
    assert eff.call_size_invariant is True and recorder.options(entry)[-1] == (OPTION, 1)
    assert EffLocalizer(sd, input_shape=(320, 320)).call_size_invariant is False


@pytest.mark.parametrize("arch,img", [("swin_tiny_patch4_window7_224", 224), ("resnet34", 32), ("mobilenetv3_small_075", 32),
                                      ("efficientnet_b0", 32), ("convnext_tiny", 32), ("mobilenetv3_small_050", 32)])
@pytest.mark.parametrize("kw", [False, True])
def test_engines_that_always_had_the_property(recorder, arch, img, kw):
    """The family encoders and convnext_tiny / mobilenetv3_small_050 accept the keyword, ignore it and report True."""
    enc = E.make_encoder(arch, init_state_dict(arch, seed=0, img_size=img), img_size=img, call_size_invariant=kw)
    assert enc.call_size_invariant is True
    assert not [n for n, _ in recorder.calls if n.endswith("set_option")]
    if isinstance(enc, E._FamilyEncoder):
        with pytest.raises(ValueError, match="has no option 'call_size_invariant'"):       # as for every other option name
            enc.set_option("call_size_invariant", 1)
