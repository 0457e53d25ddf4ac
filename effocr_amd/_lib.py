"""ctypes binding of libeffocr_hip.so (include/effocr_hip.h) — the only door to the HIP kernels.

There is deliberately no fallback: if the shared library is missing or a call fails, an exception
is raised.  Nothing here (or anywhere in ``effocr_amd``) imports ``oracle/``.
"""
import ctypes
import os
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
# EFFOCR_HIP_LIB: A/B experiments only (tools/): another build of the SAME library; the product default is the in-tree .so
SO_PATH = os.environ.get("EFFOCR_HIP_LIB") or os.path.join(_HERE, "libeffocr_hip.so")
# the product library + the kernels only A/B switches reach (row-panel GEMM, fused MLP without the projection phase): `make AB=1`.
# Never loaded by the engines on their own; tests that compare those paths switch to it with use_library().
SO_PATH_AB = os.path.join(_HERE, "libeffocr_hip_ab.so")

ABI_VERSION = 9          # == EFFOCR_ABI_VERSION of include/effocr_hip.h (tests/test_cabi.py checks the pair)
PREC = {"bf16": 0, "fp16": 1, "fp32": 2}
EPI = {"bias": 0, "bias_gelu": 1, "bias_resid": 2}

_lock = threading.Lock()
_lib = None
_loaded = {}             # path -> handle (use_library switches between them)


class EffOCRHipError(RuntimeError):
    pass


def build(force=False, verbose=False, ab=True):
    """Compile every HIP source for gfx950 into effocr_amd/libeffocr_hip.so (hipcc cross-compiles without a GPU) and, with ``ab``,
    the A/B build effocr_amd/libeffocr_hip_ab.so the tests of the alternative kernel paths load.  Returns the product library's path."""
    so = os.path.join(_HERE, "libeffocr_hip.so")
    for extra, target in (([], so),) + (((["AB=1"], SO_PATH_AB),) if ab else ()):
        cmd = ["make", "-C", _CSRC, "-j", str(min(16, os.cpu_count() or 1))] + extra
        if force and not extra:                                # the AB link reuses the objects the first pass just rebuilt
            cmd.append("-B")
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if verbose or res.returncode != 0:
            print(res.stdout)
        if res.returncode != 0 or not os.path.exists(target):
            raise EffOCRHipError(f"building {os.path.basename(target)} failed:\n" + res.stdout[-4000:])
    return so


def use_library(path=None):
    """Switch the process to another build of the library (tests: SO_PATH_AB) — or back to the default with ``None``.  Engine objects
    keep the handle they were created with, so objects made before and after a switch do not mix.  Returns the previous path."""
    global _lib, SO_PATH, EXPORTS
    with _lock:
        prev = SO_PATH
        SO_PATH = path or os.environ.get("EFFOCR_HIP_LIB") or os.path.join(_HERE, "libeffocr_hip.so")
        if SO_PATH != prev:
            _lib = _loaded.get(SO_PATH)
            if _lib is not None:
                EXPORTS = sorted(_declare(_lib).keys())
    return prev


def _declare(lib):
    c = ctypes
    vp, i32, i64, sz, f32p, i64p = c.c_void_p, c.c_int, c.c_int64, c.c_size_t, c.c_void_p, c.c_void_p
    sig = {
        "effocr_abi_version": (i32, []),
        "effocr_last_error": (c.c_char_p, []),
        "effocr_encoder_create": (i32, [c.c_char_p, i32, i32, c.POINTER(vp)]),
        "effocr_encoder_destroy": (None, [vp]),
        "effocr_encoder_embed_dim": (i32, [vp]),
        "effocr_encoder_num_params": (i32, [vp]),
        "effocr_encoder_param_name": (c.c_char_p, [vp, i32]),
        "effocr_encoder_param_numel": (i64, [vp, i32]),
        "effocr_encoder_set_param": (i32, [vp, c.c_char_p, vp, i64]),
        "effocr_encoder_weights_bytes": (sz, [vp]),
        "effocr_encoder_upload": (i32, [vp, vp, sz]),
        "effocr_encoder_workspace_bytes": (sz, [vp, i32]),
        "effocr_encoder_forward": (i32, [vp, f32p, i32, f32p, i32, vp, sz, vp]),
        "effocr_encoder_forward_ex": (i32, [vp, vp, i32, i32, f32p, i32, vp, sz, vp]),
        "effocr_encoder_check_status": (i32, [vp, vp, vp]),
        "effocr_encoder_reset_status": (i32, [vp, vp, vp]),
        "effocr_clock_sample": (i32, [vp, vp]),
        "effocr_encoder_set_chunk": (i32, [vp, i32]),
        "effocr_encoder_set_option": (i32, [vp, c.c_char_p, i32]),
        "effocr_op_ln_linear": (i32, [i32, i32, f32p, f32p, f32p, c.c_float, vp, f32p, f32p, vp, i32, i32, i32, vp]),
        "effocr_encoder_profile_begin": (i32, [vp, i32, c.c_char_p]),
        "effocr_encoder_profile_collect": (i32, [vp]),
        "effocr_encoder_profile_get": (i32, [vp, i32, c.POINTER(c.c_char_p), c.POINTER(c.c_double), c.POINTER(i32),
                                             c.POINTER(c.c_double)]),
        "effocr_encoder_profile_clock": (i32, [vp, i32, c.POINTER(c.c_double)]),
        "effocr_knn_workspace_bytes": (sz, [i64, i64, i32, i32]),
        "effocr_knn_ip_topk": (i32, [f32p, i64, f32p, i64, i32, i32, f32p, i64p, vp, sz, vp]),
        "effocr_knn_screen_workspace_bytes": (sz, [i64, i64, i32, i32]),
        "effocr_knn_set_option": (i32, [c.c_char_p, i32]),
        "effocr_knn_screen_flag_offset": (sz, [i64, i64, i32, i32]),
        "effocr_knn_ip_topk_screened": (i32, [f32p, i64, f32p, vp, i64, i32, i32, c.c_float, f32p, i64p, vp, sz, vp]),
        "effocr_convert_bf16": (i32, [f32p, i64, vp, vp]),
        "effocr_bf16_blocked_bytes": (sz, [i64, i32]),
        "effocr_convert_bf16_blocked": (i32, [f32p, i64, i32, vp, vp]),
        "effocr_knn_ip_topk_screened2": (i32, [f32p, i64, f32p, vp, vp, i64, i32, i32, c.c_float, f32p, i64p, vp, sz, vp]),
        "effocr_l2_normalize": (i32, [f32p, i64, i32, f32p, vp]),
        "effocr_gather_rows": (i32, [f32p, i64p, i64, i32, f32p, vp]),
        "effocr_crop_transform": (i32, [vp, i32, i32, i64, vp, i32, i32, i32, c.POINTER(c.c_float), c.POINTER(c.c_float),
                                        c.POINTER(c.c_float), f32p, vp]),
        "effocr_crop_transform_batch": (i32, [vp, i32, i64, i32, i32, i64, vp, i64, i32, i32, c.POINTER(c.c_float), c.POINTER(c.c_float),
                                              c.POINTER(c.c_float), f32p, vp]),
        "effocr_crop_transform_batch_ex": (i32, [vp, i32, i64, i32, i32, i64, vp, i64, i32, i32, c.POINTER(c.c_float), c.POINTER(c.c_float),
                                                 c.POINTER(c.c_float), i32, vp, vp]),
        "effocr_localizer_create": (i32, [c.c_char_p, i32, i32, i32, c.POINTER(vp)]),
        "effocr_localizer_destroy": (None, [vp]),
        "effocr_localizer_num_params": (i32, [vp]),
        "effocr_localizer_param_name": (c.c_char_p, [vp, i32]),
        "effocr_localizer_param_numel": (i64, [vp, i32]),
        "effocr_localizer_set_param": (i32, [vp, c.c_char_p, vp, i64]),
        "effocr_localizer_weights_bytes": (sz, [vp]),
        "effocr_localizer_upload": (i32, [vp, vp, sz]),
        "effocr_localizer_set_option": (i32, [vp, c.c_char_p, i32]),
        "effocr_localizer_num_predictions": (i64, [vp]),
        "effocr_localizer_num_outputs": (i32, [vp]),
        "effocr_localizer_workspace_bytes": (sz, [vp, i32]),
        "effocr_localizer_forward": (i32, [vp, f32p, i32, f32p, vp, sz, vp]),
        "effocr_letterbox": (i32, [vp, i32, i32, i64, i32, i32, i32, i32, i32, i32, i32, f32p, vp]),
        "effocr_nms_workspace_bytes": (sz, [i32, i32]),
        "effocr_nms_batch_workspace_bytes": (sz, [i32, i32, i32]),
        "effocr_nms": (i32, [f32p, i32, i32, c.c_float, c.c_float, i32, i32, c.c_float, i32, f32p, vp, vp, sz, vp]),
        "effocr_nms_batch": (i32, [f32p, i32, i32, i32, c.c_float, c.c_float, i32, i32, c.c_float, i32, f32p, vp, vp, sz, vp]),
        "effocr_parse_char_boxes": (i32, [f32p, vp, i32, i32, i32, i32, i32, i32, f32p, vp, vp, vp, vp]),
        "effocr_op_linear": (i32, [i32, i32, vp, vp, f32p, f32p, vp, i32, i32, i32, vp]),
        "effocr_op_layernorm": (i32, [i32, f32p, i64, i32, f32p, f32p, c.c_float, vp, vp]),
        "effocr_op_attention": (i32, [i32, vp, vp, i32, i32, i32, vp]),
        "effocr_op_linear_blocked": (i32, [i32, i32, vp, vp, f32p, f32p, vp, i32, i32, i32, i32, vp]),
        "effocr_op_mlp_blocked": (i32, [i32, f32p, f32p, f32p, c.c_float, vp, f32p, vp, f32p, f32p, i32, i32, i32, i32, vp, sz, vp]),
        "effocr_op_mlp_ln_blocked": (i32, [i32, f32p, f32p, f32p, c.c_float, vp, f32p, vp, f32p, f32p, f32p, f32p, vp, i32, i32, i32, i32, vp, sz, vp]),
        "effocr_op_proj_mlp_blocked": (i32, [i32, f32p, vp, vp, f32p, f32p, f32p, c.c_float, vp, f32p, vp, f32p, f32p, i32, i32, i32, i32, vp, sz, vp]),
        "effocr_op_qkv_attn_blocked": (i32, [i32, vp, vp, f32p, vp, i32, i32, i32, i32, vp]),
        "effocr_op_layernorm_blocked": (i32, [i32, f32p, i64, i32, f32p, f32p, c.c_float, vp, vp]),
    }
    for name, (res, args) in sig.items():
        if os.environ.get("EFFOCR_HIP_LIB") and not hasattr(lib, name):
            # A/B against an older build of the SAME ABI (tools/ab_bench.sh): a symbol added since is absent — calling it must fail
            # loudly, never run with ctypes' default int signature
            def _absent(*a, _n=name, **k):
                raise EffOCRHipError(f"{_n} is not exported by the library EFFOCR_HIP_LIB points at")
            setattr(lib, name, _absent)
            continue
        fn = getattr(lib, name)            # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return sig


EXPORTS = None


def lib():
    """Load (once) and return the ctypes handle; raises if the extension has not been built."""
    global _lib, EXPORTS
    with _lock:
        if _lib is None:
            if not os.path.exists(SO_PATH):
                raise EffOCRHipError(
                    f"{SO_PATH} not found: the HIP extension is required (no CPU fallback). "
                    "Run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C effocr_amd/csrc`.")
            handle = ctypes.CDLL(SO_PATH)
            EXPORTS = sorted(_declare(handle).keys())
            # the override keeps the ABI check: an older-or-equal version only behind a second, explicit flag (A/B runs against the
            # previous round's build), and never a newer or foreign one
            got = handle.effocr_abi_version()
            older_ok = bool(os.environ.get("EFFOCR_HIP_LIB")) and os.environ.get("EFFOCR_HIP_ALLOW_OLDER_ABI") == "1" and 0 < got <= ABI_VERSION
            if got != ABI_VERSION and not older_ok:
                raise EffOCRHipError(f"libeffocr_hip.so ABI version {got} != {ABI_VERSION} expected by this package: rebuild (make -C effocr_amd/csrc)")
            _lib = _loaded[SO_PATH] = handle
    return _lib


# The optional capabilities ship as shared objects of their own, because libeffocr_hip.so is at its size cap (DESIGN.md "Library split"):
# each has its own header, ABI version and last_error, exports effocr_<prefix>_* and is bound by <prefix>_lib() below.  None of their
# functions is part of EXPORTS (the product library's ABI, checked against effocr_hip.h).
_family = {}             # prefix -> handle


def _load_family(so_path, prefix, abi_version, signatures, label):
    """Load (once) and return the ctypes handle of the library at ``so_path``; raises if it is missing or its ABI version differs."""
    with _lock:
        handle = _family.get(prefix)
        if handle is None:
            if not os.path.exists(so_path):
                raise EffOCRHipError(f"{so_path} not found: the {label} library is required (no CPU fallback). "
                                     "Run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C effocr_amd/csrc`.")
            handle = ctypes.CDLL(so_path)
            for name, (res, args) in signatures.items():
                fn = getattr(handle, name)           # AttributeError if the symbol is not exported
                fn.restype, fn.argtypes = res, args
            got = getattr(handle, f"effocr_{prefix}_abi_version")()
            if got != abi_version:
                raise EffOCRHipError(f"{os.path.basename(so_path)} ABI version {got} != {abi_version} expected by this package: rebuild "
                                     "(make -C effocr_amd/csrc)")
            _family[prefix] = handle
    return handle


def _family_check(prefix):
    def check(rc, what=""):
        if rc != 0:
            msg = getattr(globals()[f"{prefix}_lib"](), f"effocr_{prefix}_last_error")()
            raise EffOCRHipError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")
    check.__name__ = f"{prefix}_check"
    return check


# libeffocr_head.so (include/effocr_head.h): the FFNN classifier head.
HEAD_SO_PATH = os.path.join(_HERE, "libeffocr_head.so")
HEAD_ABI_VERSION = 1     # == EFFOCR_HEAD_ABI_VERSION of include/effocr_head.h
HEAD_EXPORTS = ("effocr_head_abi_version", "effocr_head_last_error", "effocr_classifier_head_workspace_bytes",
                "effocr_classifier_head")


def _head_signatures():
    c = ctypes
    return {
        "effocr_head_abi_version": (c.c_int, []),
        "effocr_head_last_error": (c.c_char_p, []),
        "effocr_classifier_head_workspace_bytes": (c.c_size_t, [c.c_int64, c.c_int]),
        "effocr_classifier_head": (c.c_int, [c.c_void_p, c.c_int64, c.c_int, c.c_void_p, c.c_void_p, c.c_int, c.c_void_p,
                                             c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]),
    }


def head_lib():
    return _load_family(HEAD_SO_PATH, "head", HEAD_ABI_VERSION, _head_signatures(), "classifier head")


# libeffocr_swin.so (include/effocr_swin.h): the Swin-T encoder (it carries its own copy of the GEMMs, hidden).
SWIN_SO_PATH = os.path.join(_HERE, "libeffocr_swin.so")
SWIN_ABI_VERSION = 1     # == EFFOCR_SWIN_ABI_VERSION of include/effocr_swin.h


def _encoder_signatures(prefix):
    """The entry points every encoder-family library exports (csrc/enc_core.hpp holds their shared bodies)."""
    c = ctypes
    vp, i32, i64, sz = c.c_void_p, c.c_int, c.c_int64, c.c_size_t
    return {f"effocr_{prefix}_{k}": v for k, v in {
        "abi_version": (i32, []),
        "last_error": (c.c_char_p, []),
        "create": (i32, [c.c_char_p, i32, i32, c.POINTER(vp)]),
        "destroy": (None, [vp]),
        "embed_dim": (i32, [vp]),
        "num_params": (i32, [vp]),
        "param_name": (c.c_char_p, [vp, i32]),
        "param_numel": (i64, [vp, i32]),
        "set_param": (i32, [vp, c.c_char_p, vp, i64]),
        "weights_bytes": (sz, [vp]),
        "upload": (i32, [vp, vp, sz]),
        "workspace_bytes": (sz, [vp, i32]),
        "set_chunk": (i32, [vp, i32]),
        "forward": (i32, [vp, vp, i32, vp, i32, vp, sz, vp]),
        "check_status": (i32, [vp, vp, vp]),
    }.items()}


def _swin_signatures():
    c = ctypes
    vp, i32, i64 = c.c_void_p, c.c_int, c.c_int64
    sig = _encoder_signatures("swin")
    sig["effocr_swin_op_stem"] = (i32, [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp])             # test entry points
    sig["effocr_swin_op_layernorm"] = (i32, [i32, vp, i64, i32, i32, vp, vp, vp, vp])
    sig["effocr_swin_op_merge"] = (i32, [i32, vp, i32, i32, i32, i32, vp, vp, vp, vp])
    sig["effocr_swin_op_window_attention"] = (i32, [i32, vp, i32, i32, i32, i32, i32, vp, vp, vp])
    sig["effocr_swin_op_head"] = (i32, [vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp])
    sig["effocr_swin_op_linear"] = (i32, [i32, i32, vp, vp, vp, vp, vp, i64, i32, i32, vp])
    return sig


SWIN_EXPORTS = tuple(sorted(_swin_signatures()))


def swin_lib():
    return _load_family(SWIN_SO_PATH, "swin", SWIN_ABI_VERSION, _swin_signatures(), "Swin encoder")


# libeffocr_resnet.so (include/effocr_resnet.h): the ResNet-34 / ResNet-50 encoders (it carries its own copy of resnet18's fp32
# convolution pipeline, hidden).
RESNET_SO_PATH = os.path.join(_HERE, "libeffocr_resnet.so")
RESNET_ABI_VERSION = 1     # == EFFOCR_RESNET_ABI_VERSION of include/effocr_resnet.h
RESNET_EXPORTS = tuple(sorted(_encoder_signatures("resnet")))


def resnet_lib():
    return _load_family(RESNET_SO_PATH, "resnet", RESNET_ABI_VERSION, _encoder_signatures("resnet"), "ResNet encoder")


# libeffocr_mnv3.so (include/effocr_mnv3.h): the MobileNetV3 small_075 / small_100 / large_100 encoders (a forward of its own,
# activations in HBM between blocks).
MNV3_SO_PATH = os.path.join(_HERE, "libeffocr_mnv3.so")
MNV3_ABI_VERSION = 1     # == EFFOCR_MNV3_ABI_VERSION of include/effocr_mnv3.h


def _mnv3_signatures():
    c = ctypes
    vp, i32, i64 = c.c_void_p, c.c_int, c.c_int64
    sig = _encoder_signatures("mnv3")
    sig["effocr_mnv3_op_stem"] = (i32, [vp, i32, i32, vp, vp, vp, vp])                          # test entry points
    sig["effocr_mnv3_op_dw"] = (i32, [vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp])
    sig["effocr_mnv3_op_se_gate"] = (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp])
    sig["effocr_mnv3_op_pw"] = (i32, [i32, vp, i64, i32, vp, i32, vp, vp, i32, i32, vp, vp, vp])
    sig["effocr_mnv3_op_pool"] = (i32, [vp, i32, i32, i32, vp, vp])
    sig["effocr_mnv3_op_finish"] = (i32, [vp, i32, i32, i32, vp, vp])
    return sig


MNV3_EXPORTS = tuple(sorted(_mnv3_signatures()))


def mnv3_lib():
    return _load_family(MNV3_SO_PATH, "mnv3", MNV3_ABI_VERSION, _mnv3_signatures(), "MobileNetV3 encoder")


# libeffocr_effnet.so (include/effocr_effnet.h): the EfficientNet-B0 encoders efficientnet_b0 / tf_efficientnet_b0 (its own stem,
# depthwise and squeeze-excite kernels, plus a hidden copy of libeffocr_mnv3.so's pointwise GEMM).
EFFNET_SO_PATH = os.path.join(_HERE, "libeffocr_effnet.so")
EFFNET_ABI_VERSION = 1     # == EFFOCR_EFFNET_ABI_VERSION of include/effocr_effnet.h


def _effnet_signatures():
    c = ctypes
    vp, i32 = c.c_void_p, c.c_int
    sig = _encoder_signatures("effnet")
    sig["effocr_effnet_forward"] = (i32, [vp, vp, i32, i32, vp, i32, vp, c.c_size_t, vp])      # (the crop type after the crops)
    sig["effocr_effnet_reset_status"] = (i32, [vp, vp, vp])
    sig["effocr_effnet_op_tiles"] = (i32, [i32])                                                # test entry points
    sig["effocr_effnet_op_stem"] = (i32, [vp, i32, i32, i32, vp, vp, vp, vp])
    sig["effocr_effnet_op_dw_se"] = (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp])
    return sig


EFFNET_EXPORTS = tuple(sorted(_effnet_signatures()))


def effnet_lib():
    return _load_family(EFFNET_SO_PATH, "effnet", EFFNET_ABI_VERSION, _effnet_signatures(), "EfficientNet encoder")


# libeffocr_beit.so (include/effocr_beit.h): the BEiT base encoders beit_base_patch16_224 / beitv2_base_patch16_224 (attention with a
# relative-position bias; it carries its own copies of the GEMMs and of the ViT helper kernels, hidden).
BEIT_SO_PATH = os.path.join(_HERE, "libeffocr_beit.so")
BEIT_ABI_VERSION = 1     # == EFFOCR_BEIT_ABI_VERSION of include/effocr_beit.h


def _beit_signatures():
    c = ctypes
    vp, i32 = c.c_void_p, c.c_int
    sig = _encoder_signatures("beit")
    sig["effocr_beit_reset_status"] = (i32, [vp, vp, vp])
    sig["effocr_beit_op_attn"] = (i32, [vp, vp, i32, i32, i32, i32, vp, vp])                    # test entry point
    return sig


BEIT_EXPORTS = tuple(sorted(_beit_signatures()))


def beit_lib():
    return _load_family(BEIT_SO_PATH, "beit", BEIT_ABI_VERSION, _beit_signatures(), "BEiT encoder")


# libeffocr_bit.so (include/effocr_bit.h): the BiT ResNetV2 encoders resnetv2_50x1_bitm / resnetv2_101x1_bitm (GroupNorm + ReLU, stem pool
# and head kernels of its own; it carries its own copies of the ResNet paths' convolutions, hidden).
BIT_SO_PATH = os.path.join(_HERE, "libeffocr_bit.so")
BIT_ABI_VERSION = 1     # == EFFOCR_BIT_ABI_VERSION of include/effocr_bit.h


def _bit_signatures():
    c = ctypes
    vp, i32, sz = c.c_void_p, c.c_int, c.c_size_t
    sig = _encoder_signatures("bit")
    sig["effocr_bit_reset_status"] = (i32, [vp, vp, vp])
    sig["effocr_bit_op_groupnorm_relu"] = (i32, [i32, vp, i32, i32, i32, vp, vp, vp, vp, sz, vp])   # test entry points
    sig["effocr_bit_op_stem_pool"] = (i32, [i32, vp, i32, i32, i32, i32, vp, vp])
    sig["effocr_bit_op_head"] = (i32, [i32, vp, i32, i32, i32, vp, vp, i32, vp, vp, vp])
    return sig


BIT_EXPORTS = tuple(sorted(_bit_signatures()))


def bit_lib():
    return _load_family(BIT_SO_PATH, "bit", BIT_ABI_VERSION, _bit_signatures(), "BiT ResNetV2 encoder")


# libeffocr_vit8.so (include/effocr_vit8.h): the patch-8 ViT encoders vit_small_patch8_224 / vit_base_patch8_224 (attention that streams
# its key tiles, an 8x8 patch im2col; it carries its own copies of the GEMMs and of the ViT helper kernels, hidden).
VIT8_SO_PATH = os.path.join(_HERE, "libeffocr_vit8.so")
VIT8_ABI_VERSION = 1     # == EFFOCR_VIT8_ABI_VERSION of include/effocr_vit8.h


def _vit8_signatures():
    c = ctypes
    vp, i32 = c.c_void_p, c.c_int
    sig = _encoder_signatures("vit8")
    sig["effocr_vit8_reset_status"] = (i32, [vp, vp, vp])
    sig["effocr_vit8_op_attn"] = (i32, [vp, i32, i32, i32, i32, vp, vp])                        # test entry points
    sig["effocr_vit8_op_patch_embed"] = (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp])
    return sig


VIT8_EXPORTS = tuple(sorted(_vit8_signatures()))


def vit8_lib():
    return _load_family(VIT8_SO_PATH, "vit8", VIT8_ABI_VERSION, _vit8_signatures(), "patch-8 ViT encoder")


# libeffocr_levit.so (include/effocr_levit.h): the LeViT encoders levit_128s / levit_128 / levit_192 / levit_256 / levit_384 (attention with
# narrow queries and keys, a per-head offset bias and a strided-query form, a 3x3 stem; it carries its own copies of the GEMMs, hidden).
LEVIT_SO_PATH = os.path.join(_HERE, "libeffocr_levit.so")
LEVIT_ABI_VERSION = 1     # == EFFOCR_LEVIT_ABI_VERSION of include/effocr_levit.h


def _levit_signatures():
    c = ctypes
    vp, i32, i64 = c.c_void_p, c.c_int, c.c_int64
    sig = _encoder_signatures("levit")
    sig["effocr_levit_reset_status"] = (i32, [vp, vp, vp])
    sig["effocr_levit_op_attention"] = (i32, [vp, i64, i32, i32, vp, i64, i32, i32, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp])   # test entry points
    sig["effocr_levit_op_stem_conv"] = (i32, [vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, vp, i32, i32, vp])
    return sig


LEVIT_EXPORTS = tuple(sorted(_levit_signatures()))


def levit_lib():
    return _load_family(LEVIT_SO_PATH, "levit", LEVIT_ABI_VERSION, _levit_signatures(), "LeViT encoder")


# libeffocr_regnet.so (include/effocr_regnet.h): the RegNetX / RegNetY encoders regnetx_002 ... regnety_016 (a grouped 3x3 convolution, a
# squeeze-excite gate, a ReLU stem, shortcut rows and a ReLU of its own, plus a hidden copy of libeffocr_mnv3.so's pointwise GEMM).
REGNET_SO_PATH = os.path.join(_HERE, "libeffocr_regnet.so")
REGNET_ABI_VERSION = 1     # == EFFOCR_REGNET_ABI_VERSION of include/effocr_regnet.h


def _regnet_signatures():
    c = ctypes
    vp, i32, i64, sz = c.c_void_p, c.c_int, c.c_int64, c.c_size_t
    sig = _encoder_signatures("regnet")
    sig["effocr_regnet_reset_status"] = (i32, [vp, vp, vp])
    sig["effocr_regnet_op_tiles"] = (i32, [i32])                                                # test entry points
    sig["effocr_regnet_op_gconv_weight_bytes"] = (sz, [i32, i32, i32])
    sig["effocr_regnet_op_pack_gconv"] = (i32, [i32, i32, i32, vp, vp])
    sig["effocr_regnet_op_gconv"] = (i32, [i32, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp])
    sig["effocr_regnet_op_se_gate"] = (i32, [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp])
    sig["effocr_regnet_op_stem"] = (i32, [vp, i32, i32, vp, vp, vp, vp])
    sig["effocr_regnet_op_gather2"] = (i32, [vp, i32, i32, i32, vp, vp])
    sig["effocr_regnet_op_relu"] = (i32, [vp, i64, vp])
    return sig


REGNET_EXPORTS = tuple(sorted(_regnet_signatures()))


def regnet_lib():
    return _load_family(REGNET_SO_PATH, "regnet", REGNET_ABI_VERSION, _regnet_signatures(), "RegNet encoder")


# libeffocr_pvt.so (include/effocr_pvt.h): the PVTv2 encoders pvt_v2_b0 ... pvt_v2_b5 (attention over at most 49 spatially reduced keys, a
# depthwise 3x3 + GELU on token rows, overlapping patch embeddings and the reduction as implicit GEMMs, a GEMM for its narrow widths).
PVT_SO_PATH = os.path.join(_HERE, "libeffocr_pvt.so")
PVT_ABI_VERSION = 1     # == EFFOCR_PVT_ABI_VERSION of include/effocr_pvt.h


def _pvt_signatures():
    c = ctypes
    vp, i32 = c.c_void_p, c.c_int
    sig = _encoder_signatures("pvt")
    sig["effocr_pvt_reset_status"] = (i32, [vp, vp, vp])
    sig["effocr_pvt_op_attention"] = (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp])      # test entry points
    sig["effocr_pvt_op_dwconv_gelu"] = (i32, [vp, i32, i32, i32, i32, vp, vp, i32, vp, vp])
    sig["effocr_pvt_op_stem"] = (i32, [vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp])
    sig["effocr_pvt_op_conv_ln"] = (i32, [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp])
    return sig


PVT_EXPORTS = tuple(sorted(_pvt_signatures()))


def pvt_lib():
    return _load_family(PVT_SO_PATH, "pvt", PVT_ABI_VERSION, _pvt_signatures(), "PVTv2 encoder")


# libeffocr_yolov8.so (include/effocr_yolov8.h): the YOLOv8 localizers yolov8n / s / m / l / x (a builder, a 3x3 stem and a distribution
# decode of its own; it carries its own copies of the implicit-GEMM convolution and of the YOLOv5 engine's data-movement kernels, hidden).
# Letterbox and NMS stay the product library's.
YOLOV8_SO_PATH = os.path.join(_HERE, "libeffocr_yolov8.so")
YOLOV8_ABI_VERSION = 1     # == EFFOCR_YOLOV8_ABI_VERSION of include/effocr_yolov8.h


def _yolov8_signatures():
    c = ctypes
    vp, i32, i64, sz = c.c_void_p, c.c_int, c.c_int64, c.c_size_t
    return {f"effocr_yolov8_{k}": v for k, v in {
        "abi_version": (i32, []),
        "last_error": (c.c_char_p, []),
        "create": (i32, [c.c_char_p, i32, i32, i32, c.POINTER(vp)]),
        "destroy": (None, [vp]),
        "num_params": (i32, [vp]),
        "param_name": (c.c_char_p, [vp, i32]),
        "param_numel": (i64, [vp, i32]),
        "set_param": (i32, [vp, c.c_char_p, vp, i64]),
        "weights_bytes": (sz, [vp]),
        "upload": (i32, [vp, vp, sz]),
        "set_option": (i32, [vp, c.c_char_p, i32]),
        "num_predictions": (i64, [vp]),
        "num_outputs": (i32, [vp]),
        "workspace_bytes": (sz, [vp, i32]),
        "forward": (i32, [vp, vp, i32, vp, vp, sz, vp]),
        # the two op entry points tests/test_gpu_localizer_ops.py calls (libeffocr_yolo11.so has none for these kernels)
        "op_decode": (i32, [vp, i32, vp, i32, vp, i32, i32, i32, i32, c.c_float, i64, i64, vp]),
        "op_stem": (i32, [vp, vp, i32, vp, vp] + [i32] * 9 + [vp]),
    }.items()}


YOLOV8_EXPORTS = tuple(sorted(_yolov8_signatures()))


def yolov8_lib():
    return _load_family(YOLOV8_SO_PATH, "yolov8", YOLOV8_ABI_VERSION, _yolov8_signatures(), "YOLOv8 localizer")


# libeffocr_yolo11.so (include/effocr_yolo11.h): the YOLO11 localizers yolo11n / s / m / l / x (a builder, an attention kernel and a
# depthwise 3x3 kernel of its own; the convolution, the YOLOv5 data-movement kernels and the YOLOv8 stem and decode compiled in again,
# hidden) and the two op entry points its kernel tests call.  Letterbox and NMS stay the product library's.
YOLO11_SO_PATH = os.path.join(_HERE, "libeffocr_yolo11.so")
YOLO11_ABI_VERSION = 1     # == EFFOCR_YOLO11_ABI_VERSION of include/effocr_yolo11.h
YOLO11_MAX_TOKENS = 1600   # == EFFOCR_YOLO11_MAX_TOKENS


def _yolo11_signatures():
    c = ctypes
    vp, i32 = c.c_void_p, c.c_int
    sig = {k.replace("effocr_yolov8_", "effocr_yolo11_"): v for k, v in _yolov8_signatures().items() if "_op_" not in k}
    sig["effocr_yolo11_op_attention"] = (i32, [vp, i32, i32, i32, i32, vp, vp])
    sig["effocr_yolo11_op_dwconv3x3"] = (i32, [vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, i32, vp])
    return sig


YOLO11_EXPORTS = tuple(sorted(_yolo11_signatures()))


def yolo11_lib():
    return _load_family(YOLO11_SO_PATH, "yolo11", YOLO11_ABI_VERSION, _yolo11_signatures(), "YOLO11 localizer")


head_check = _family_check("head")
swin_check = _family_check("swin")
resnet_check = _family_check("resnet")
mnv3_check = _family_check("mnv3")
effnet_check = _family_check("effnet")
beit_check = _family_check("beit")
bit_check = _family_check("bit")
vit8_check = _family_check("vit8")
yolov8_check = _family_check("yolov8")
yolo11_check = _family_check("yolo11")
levit_check = _family_check("levit")
regnet_check = _family_check("regnet")
pvt_check = _family_check("pvt")


def check(rc, what="", handle=None):
    """``handle``: the library the failing call was made through (engines pass the one they were created with — last_error is
    per shared object, and use_library() may have switched the process default since)."""
    if rc != 0:
        msg = (handle or lib()).effocr_last_error()
        raise EffOCRHipError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")


def ptr(t):
    """Device/host pointer of a torch tensor (or None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def current_stream(device):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_gpu(device=None):
    """Resolve ``device`` to a concrete GPU.  ``None`` and an index-less ``"cuda"`` mean torch's CURRENT device — the semantics
    of the reference's default ``--device cuda`` (infer_effocr.py:439,178) — so that with one process per GPU
    (``torch.cuda.set_device(LOCAL_RANK)``) every engine of a rank lands on that rank's GPU, never on a literal GPU 0."""
    import torch
    if not torch.cuda.is_available():
        raise EffOCRHipError("no ROCm GPU visible: the EffOCR HIP path has no CPU fallback")
    d = torch.device("cuda" if device is None else device)
    if d.type != "cuda":
        raise EffOCRHipError(f"device {device!r} is not a GPU: the EffOCR HIP path has no CPU fallback")
    if d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d
