"""ctypes binding of effocr_amd/libeffocr_convops.so, the TEST-ONLY operator library (csrc/convops_api.hip): thin wrappers over the
convolution, pooling and data-movement launchers of resnet.hip, resnet16.hip and yolo.hip, the ConvNeXt launchers of convnext.hip, the
linears of convnext_forward (gemm.hip, gemm2.hip) and the non-GEMM launchers of the ViT path (patch.hip, vit_ops.hip, qkvattn.hip and
EPI_PATCH of both GEMMs: effocr_convops_vit_*).  `make` builds it next to the product
libraries (``__graft_entry__.build()``); a missing library is an error here — no skip, no fallback."""

import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO_PATH = os.path.join(ROOT, "effocr_amd", "libeffocr_convops.so")
ABI_VERSION = 4
PREC_BF16, PREC_FP16, PREC_FP32 = 0, 1, 2
PREC = {"bf16": PREC_BF16, "fp16": PREC_FP16, "fp32": PREC_FP32}
OK, EINVAL, EUNSUPPORTED = 0, -1, -2

_c = ctypes
_vp, _i, _sz, _i64, _f = _c.c_void_p, _c.c_int, _c.c_size_t, _c.c_int64, _c.c_float
SIGNATURES = {
    "effocr_convops_abi_version": (_i, []),
    "effocr_convops_last_error": (_c.c_char_p, []),
    "effocr_convops_device_cus": (_i, []),
    "effocr_convops_last_dispatch": (None, [_c.POINTER(_i), _c.POINTER(_i)]),
    # in, w, bias, resid, out, B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW, relu, in_ld, in_off, out_ld, out_off, res_ld, res_off, silu,
    # partial, partial_bytes, w16, stream
    "effocr_convops_conv2d": (_i, [_vp] * 5 + [_i] * 19 + [_vp, _sz, _vp, _vp]),
    # prec, in, w, bias, resid, out, B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW, relu, stream
    "effocr_convops_conv16": (_i, [_i] + [_vp] * 5 + [_i] * 12 + [_vp]),
    "effocr_convops_im2col_conv1": (_i, [_vp, _vp] + [_i] * 5 + [_vp]),                    # x, col, B, H, W, OH, OW
    "effocr_convops_im2col_nchw": (_i, [_vp, _vp] + [_i] * 11 + [_vp]),                    # x, col, B, Cin, H, W, KH, KW, stride, pad, OH, OW, kpad
    "effocr_convops_maxpool3x3s2": (_i, [_vp, _vp] + [_i] * 6 + [_vp]),                    # in, out, B, H, W, C, OH, OW
    "effocr_convops_avgpool": (_i, [_vp, _vp] + [_i] * 4 + [_vp]),                         # in, out, B, HW, C, l2norm
    "effocr_convops_stem6x6s2": (_i, [_vp, _vp, _i, _vp, _vp, _vp] + [_i] * 8 + [_vp]),    # x, w, w_ld, wt, bias, out, B, H, W, OH, OW, out_ld, out_off, silu
    "effocr_convops_stem6x6s2_g16": (_i, [_vp, _vp, _i, _vp, _vp] + [_i] * 9 + [_vp]),     # x, wt, wt_ld, bias, out, B, H, W, OH, OW, out_ld, out_off, cout, cout_st
    "effocr_convops_upsample2x": (_i, [_vp, _i, _i, _vp, _i, _i] + [_i] * 4 + [_vp]),      # in, in_ld, in_off, out, out_ld, out_off, B, H, W, C
    "effocr_convops_maxpool5": (_i, [_vp, _i, _i, _vp, _i, _i] + [_i] * 4 + [_vp]),
    # raw, raw_ld, pred, B, ny, nx, na, no, stride, anchors_px (HOST, 2 * na floats), total, row0
    "effocr_convops_yolo_decode": (_i, [_vp, _i, _vp] + [_i] * 5 + [_f, _c.POINTER(_f), _i64, _i64, _vp]),
    "effocr_convops_im2col16": (_i, [_i, _vp, _vp] + [_i] * 5 + [_vp]),                    # prec, x, col, B, H, W, OH, OW
    "effocr_convops_maxpool16": (_i, [_i, _vp, _vp] + [_i] * 6 + [_vp]),                   # prec, in, out, B, H, W, C, OH, OW
    "effocr_convops_avgpool16": (_i, [_i, _vp, _vp] + [_i] * 4 + [_vp, _vp]),              # prec, in, emb, B, HW, C, l2norm, status
    "effocr_convops_cnx_stem": (_i, [_vp, _i, _i] + [_vp] * 4 + [_i, _vp, _vp]),           # img, B, S, wt, bias, lnw, lnb, C0, x
    "effocr_convops_cnx_dwconv_ln": (_i, [_i, _vp] + [_i] * 5 + [_vp] * 6),                # prec, x, B, H, W, C, Cp, w, bias, lnw, lnb, out
    "effocr_convops_cnx_ln_s2d": (_i, [_i, _vp] + [_i] * 5 + [_vp] * 4),                   # prec, x, B, H, W, C, Cp, lnw, lnb, out
    "effocr_convops_cnx_head": (_i, [_vp] + [_i] * 4 + [_vp, _vp, _i, _vp, _vp, _vp]),     # x, B, HW, C, Cp, lnw, lnb, l2norm, emb, status
    "effocr_convops_linear": (_i, [_i, _i] + [_vp] * 6 + [_i] * 3 + [_vp]),                # precision, epilogue, x, w, bias, resid, scale, out, m, n, k
    "effocr_convops_vit_patch_embed": (_i, [_i, _vp] + [_i] * 4 + [_vp] * 5 + [_i, _i, _vp]),   # prec, x, x16, B, H, W, wb, bias, pos, cls, out, D, P
    "effocr_convops_vit_patch_embed_last_dispatch": (None, [_c.POINTER(_i), _c.POINTER(_i)]),
    "effocr_convops_vit_im2col16": (_i, [_i, _vp] + [_i] * 4 + [_vp, _vp]),                # prec, x, x16, B, H, W, col
    "effocr_convops_vit_patch_gemm": (_i, [_i] + [_vp] * 5 + [_i] * 4 + [_vp]),            # prec, col, w, bias, pos, out, B, P, D, blk_out
    "effocr_convops_vit_set_cls": (_i, [_vp, _vp] + [_i] * 4 + [_vp, _vp]),                # cls_pos0, x, B, T, D, blocked, status_zero
    "effocr_convops_vit_gather_cls": (_i, [_vp, _vp] + [_i] * 3 + [_vp] * 3),              # x, att, B, T, D, xc, ac
    "effocr_convops_vit_qkv_attn": (_i, [_i] + [_vp] * 4 + [_i] * 3 + [_i64, _i, _i, _vp]),   # prec, xn, wb, bias, out, B, T, D, rows_alloc, cls_only, hsplit
    "effocr_convops_vit_qkv_attn_last_dispatch": (_i, [_i, _c.POINTER(_i)]),
    "effocr_convops_vit_final_norm": (_i, [_vp] + [_i] * 3 + [_vp, _vp, _f, _i, _i, _vp, _vp, _vp]),   # x, B, T, D, gamma, beta, eps, l2norm, blocked, emb, status
}
EXPORTS = sorted(SIGNATURES)

_lib = None


def lib():
    """The loaded library with every wrapper declared; raises when the library or one of its symbols is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(f"{SO_PATH} is missing: build it with python -c 'import __graft_entry__ as g; g.build()'")
        L = ctypes.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)                              # AttributeError: a wrapper that is not exported
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def last_error():
    return lib().effocr_convops_last_error().decode()


def last_dispatch():
    """(channel tile, K split) of this thread's last effocr_convops_conv2d launch."""
    nw, ks = _i(0), _i(0)
    lib().effocr_convops_last_dispatch(ctypes.byref(nw), ctypes.byref(ks))
    return nw.value, ks.value


def patch_last_dispatch():
    """(slice width, grid) of this thread's last effocr_convops_vit_patch_embed launch."""
    dw, grid = _i(0), _i(0)
    lib().effocr_convops_vit_patch_embed_last_dispatch(ctypes.byref(dw), ctypes.byref(grid))
    return dw.value, grid.value


def qkv_attn_last_dispatch():
    """One (D, token tiles, class-token form, P.V steps, head split, grid) per launch of this thread's last effocr_convops_vit_qkv_attn."""
    buf = (_i * 6)()
    n = lib().effocr_convops_vit_qkv_attn_last_dispatch(0, buf)
    out = []
    for k in range(min(n, 2)):
        lib().effocr_convops_vit_qkv_attn_last_dispatch(k, buf)
        out.append(tuple(buf))
    assert n == len(out), f"{n} launches recorded, room for 2"
    return out


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())
