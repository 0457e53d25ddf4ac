"""The seven encoder-family libraries share their handle plumbing (effocr_amd/csrc/enc_core.hpp): the messages their entry points leave in
last_error are pinned here byte for byte, as each family's own API file worded them before the plumbing was shared.  No GPU is needed:
create and set_param touch host memory only, and upload and reset_status refuse the cases below before they make a device call."""
import ctypes

import numpy as np
import pytest

from effocr_amd import _lib

# family -> (an architecture, a valid img_size, the first parameter of its table and its size, the last parameter, a refused img_size,
#            the code and the message of that refusal, the message for an unknown architecture)
FAMILIES = {
    "swin": ("swin_tiny_patch4_window7_224", 224, "patch_embed.proj.weight", 4608, "norm.bias", 192, -2,
             "swin_create: img_size must be 224 (the reference builds swin_tiny_patch4_window7_224 at timm's default size; other sizes "
             "change the window grid)",
             "swin_create: unsupported architecture 'nope'"),
    "resnet": ("resnet34", 32, "conv1.weight", 9408, "layer4.2.bn2.running_var", 40, -1,
               "resnet_create: img_size must be a positive multiple of 32",
               "resnet_create: unsupported architecture 'nope' (resnet34, resnet50)"),
    "mnv3": ("mobilenetv3_small_075", 32, "conv_stem.weight", 432, "conv_head.bias", 40, -1,
             "mnv3_create: img_size must be a multiple of 32 in [32, 224]",
             "mnv3_create: unsupported architecture 'nope' (mobilenetv3_small_050, mobilenetv3_small_075, mobilenetv3_small_100, "
             "mobilenetv3_large_100)"),
    "effnet": ("efficientnet_b0", 32, "conv_stem.weight", 864, "bn2.running_var", 40, -1,
               "effnet_create: img_size must be a multiple of 32 in [32, 224]",
               "effnet_create: unsupported architecture 'nope' (efficientnet_b0, tf_efficientnet_b0)"),
    "beit": ("beit_tiny_test", 32, "cls_token", 128, "fc_norm.bias", 40, -1,
             "beit_create: img_size must be a multiple of 16 from 16 to 224",
             "beit_create: unsupported architecture 'nope'"),
    "vit8": ("vit8_tiny_test", 16, "cls_token", 128, "norm.bias", 12, -1,
             "vit8_create: img_size must be a multiple of 8 from 8 to 224",
             "vit8_create: unsupported architecture 'nope'"),
    "bit": ("resnetv2_50x1_bitm", 32, "stem.conv.weight", 9408, "norm.bias", 40, -1,
            "bit_create: img_size must be a positive multiple of 32",
            "bit_create: unsupported architecture 'nope' (resnetv2_50x1_bitm, resnetv2_101x1_bitm)"),
}
RESET_STATUS = ["beit", "bit", "effnet", "vit8"]         # the families that export effocr_<family>_reset_status


class _Family:
    def __init__(self, fam):
        self.fam = fam
        self.L = getattr(_lib, f"{fam}_lib")()

    def __getattr__(self, name):
        return getattr(self.L, f"effocr_{self.fam}_{name}")

    def error(self):
        return self.last_error().decode()

    def make(self, arch, img, prec=_lib.PREC["fp16"]):
        h = ctypes.c_void_p()
        return self.create(arch.encode(), img, prec, ctypes.byref(h)), h


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_create_messages(fam):
    arch, img, _, _, _, bad_img, bad_img_rc, bad_img_msg, bad_arch_msg = FAMILIES[fam]
    F = _Family(fam)
    rc, _ = F.make("nope", img)
    assert (rc, F.error()) == (-2, bad_arch_msg)
    rc, _ = F.make(arch, img, prec=7)
    assert (rc, F.error()) == (-1, f"{fam}_create: unknown precision")
    rc, _ = F.make(arch, bad_img)
    assert (rc, F.error()) == (bad_img_rc, bad_img_msg)


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_set_param_and_upload_messages(fam):
    arch, img, first, first_numel, last = FAMILIES[fam][:5]
    F = _Family(fam)
    rc, h = F.make(arch, img)
    assert rc == 0, F.error()
    try:
        n = F.num_params(h)
        names = [F.param_name(h, i).decode() for i in range(n)]
        numels = [F.param_numel(h, i) for i in range(n)]
        assert (names[0], numels[0], names[-1]) == (first, first_numel, last)
        zeros = np.zeros(max(numels), dtype=np.float32)
        zp = ctypes.c_void_p(zeros.ctypes.data)

        assert F.set_param(h, b"nope.weight", zp, 5) == -1
        assert F.error() == f"{fam}_set_param: unknown parameter 'nope.weight'"
        assert F.set_param(h, first.encode(), zp, 5) == -1
        assert F.error() == f"{fam}_set_param: '{first}' expects {first_numel} elements, got 5"

        # upload: a host buffer stands in for the device blob; both refusals come before any device call
        nbytes = F.weights_bytes(h)
        dummy = ctypes.create_string_buffer(16)
        assert F.upload(h, dummy, nbytes - 1) == -3
        assert F.error() == f"{fam}_upload: weight buffer too small"
        for name, numel in zip(names[:-1], numels[:-1]):
            assert F.set_param(h, name.encode(), zp, numel) == 0, F.error()
        assert F.upload(h, dummy, nbytes) == -5
        assert F.error() == f"{fam}_upload: parameter '{last}' was never set"
    finally:
        F.destroy(h)


@pytest.mark.parametrize("fam", RESET_STATUS)
def test_reset_status_null_workspace(fam):
    arch, img = FAMILIES[fam][:2]
    F = _Family(fam)
    rc, h = F.make(arch, img)
    assert rc == 0, F.error()
    try:
        assert F.reset_status(h, None, None) == -1             # refused before any device call
        assert F.error() == f"{fam}_reset_status: NULL argument"
        assert F.reset_status(None, None, None) == -1
        assert F.error() == f"{fam}_reset_status: NULL argument"
    finally:
        F.destroy(h)
