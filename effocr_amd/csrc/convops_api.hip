// C ABI of libeffocr_convops.so — a TEST-ONLY library (DESIGN.md "Operator parity (convolutions and pools)").  Thin wrappers over the
// convolution, pooling and data-movement launchers of resnet.hip, resnet16.hip and yolo.hip, over the ConvNeXt launchers of convnext.hip,
// over the linears of convnext_forward (gemm.hip, gemm2.hip) and over the non-GEMM launchers of the ViT path (patch.hip, vit_ops.hip,
// qkvattn.hip: effocr_convops_vit_*), which this library compiles once more with hidden visibility, so that tests/test_gpu_convops.py,
// tests/test_gpu_convnext_ops.py, tests/test_gpu_vit_ops.py and (yolo.hip's Detect decode) tests/test_gpu_localizer_ops.py compare each
// kernel on its own with a float64 reference.  No product library
// exports these and no product code loads this one: libeffocr_hip.so is at its size cap (DESIGN.md "Library split").
// All device pointers are caller-owned, `stream` is a hipStream_t (NULL = the default stream); every call returns 0 or a negative
// EFFOCR_E* code (include/effocr_hip.h) whose message effocr_convops_last_error() holds for the calling thread.
#include "../../include/effocr_hip.h"
#include "enc_core.hpp"
#include "resnet16.hpp"

#include <algorithm>
#include <string>

#define CONVOPS_API extern "C" __attribute__((visibility("default")))
#define EFFOCR_CONVOPS_ABI_VERSION 4

namespace effocr {

extern thread_local int convops_last_nw, convops_last_ksplit;   // resnet.hip under -DEFFOCR_CONVOPS
extern thread_local int convops_patch_dw, convops_patch_grid;   // patch.hip, likewise
extern thread_local int convops_qa_launches, convops_qa_last[2][6];   // qkvattn.hip, likewise

}  // namespace effocr

using namespace effocr;

CONVOPS_API int effocr_convops_abi_version(void) { return EFFOCR_CONVOPS_ABI_VERSION; }
CONVOPS_API const char* effocr_convops_last_error(void) { return g_err.c_str(); }
CONVOPS_API int effocr_convops_device_cus(void) { return device_cus(); }
// channel tile (32 / 64 / 128) and K split of the calling thread's last effocr_convops_conv2d launch (0, 0 before the first)
CONVOPS_API void effocr_convops_last_dispatch(int* nw, int* ksplit) {
  if (nw) *nw = convops_last_nw;
  if (ksplit) *ksplit = convops_last_ksplit;
}

// resnet.hip conv2d_nhwc: every field of ConvArgs (kernels.hpp) but ksplit, which the dispatcher sets
CONVOPS_API int effocr_convops_conv2d(const float* in, const float* w, const float* bias, const float* resid, float* out, int B, int H, int W, int Cin,
                                      int Cout, int KH, int KW, int stride, int pad, int OH, int OW, int relu, int in_ld, int in_off, int out_ld,
                                      int out_off, int res_ld, int res_off, int silu, float* partial, size_t partial_bytes, const void* w16,
                                      void* stream) {
  convops_last_nw = 0; convops_last_ksplit = 0;
  if (!in || !bias || !out || (!w && !w16)) return fail(EFFOCR_EINVAL, "convops_conv2d: NULL argument");
  if (B < 0 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || KH < 1 || KW < 1 || stride < 1 || pad < 0 || OH < 0 || OW < 0 || (in_ld | in_off | out_ld | out_off | res_ld | res_off) < 0)
    return fail(EFFOCR_EINVAL, "convops_conv2d: bad shape");
  if (relu && silu) return fail(EFFOCR_EINVAL, "convops_conv2d: relu and silu are exclusive");
  if (OH > 0 && ((OH - 1) * stride - pad >= H || (OH - 1) * stride - pad + KH < 1)) return fail(EFFOCR_EINVAL, "convops_conv2d: OH outside the input");
  if (OW > 0 && ((OW - 1) * stride - pad >= W || (OW - 1) * stride - pad + KW < 1)) return fail(EFFOCR_EINVAL, "convops_conv2d: OW outside the input");
  if ((in_ld && in_off + Cin > in_ld) || (out_ld && out_off + Cout > out_ld) || (res_ld && res_off + Cout > res_ld) || (!in_ld && in_off) ||
      (!out_ld && out_off) || (!res_ld && res_off))
    return fail(EFFOCR_EINVAL, "convops_conv2d: a channel slice outside its row");
  ConvArgs a{};
  a.in = in; a.w = w; a.bias = bias; a.resid = resid; a.out = out;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad; a.OH = OH; a.OW = OW; a.relu = relu;
  a.in_ld = in_ld; a.in_off = in_off; a.out_ld = out_ld; a.out_off = out_off; a.res_ld = res_ld; a.res_off = res_off;
  a.silu = silu; a.partial = partial; a.partial_bytes = partial ? partial_bytes : 0; a.ksplit = 0; a.w16 = w16;
  return conv2d_nhwc(a, static_cast<hipStream_t>(stream));
}

// resnet16.hip rn_conv16: Conv16Args + prec (0 = bf16, 1 = f16)
CONVOPS_API int effocr_convops_conv16(int prec, const void* in, const void* w, const float* bias, const void* resid, void* out, int B, int H, int W,
                                      int Cin, int Cout, int KH, int KW, int stride, int pad, int OH, int OW, int relu, void* stream) {
  if (prec != PREC_BF16 && prec != PREC_FP16) return fail(EFFOCR_EINVAL, "convops_conv16: prec must be bf16 (0) or f16 (1)");
  if (!in || !w || !bias || !out) return fail(EFFOCR_EINVAL, "convops_conv16: NULL argument");
  if (B < 0 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || KH < 1 || KW < 1 || stride < 1 || pad < 0 || OH < 0 || OW < 0) return fail(EFFOCR_EINVAL, "convops_conv16: bad shape");
  if (OH > 0 && ((OH - 1) * stride - pad >= H || (OH - 1) * stride - pad + KH < 1)) return fail(EFFOCR_EINVAL, "convops_conv16: OH outside the input");
  if (OW > 0 && ((OW - 1) * stride - pad >= W || (OW - 1) * stride - pad + KW < 1)) return fail(EFFOCR_EINVAL, "convops_conv16: OW outside the input");
  Conv16Args a{};
  a.in = in; a.w = w; a.bias = bias; a.resid = resid; a.out = out;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad; a.OH = OH; a.OW = OW; a.relu = relu;
  return rn_conv16(prec, a, static_cast<hipStream_t>(stream));
}

CONVOPS_API int effocr_convops_im2col_conv1(const float* x, float* col, int B, int H, int W, int OH, int OW, void* stream) {
  if (!x || !col) return fail(EFFOCR_EINVAL, "convops_im2col_conv1: NULL argument");
  return im2col_conv1(x, col, B, H, W, OH, OW, static_cast<hipStream_t>(stream));
}
CONVOPS_API int effocr_convops_im2col_nchw(const float* x, float* col, int B, int Cin, int H, int W, int KH, int KW, int stride, int pad, int OH, int OW,
                                           int kpad, void* stream) {
  if (!x || !col) return fail(EFFOCR_EINVAL, "convops_im2col_nchw: NULL argument");
  return im2col_nchw(x, col, B, Cin, H, W, KH, KW, stride, pad, OH, OW, kpad, static_cast<hipStream_t>(stream));
}
CONVOPS_API int effocr_convops_maxpool3x3s2(const float* in, float* out, int B, int H, int W, int C, int OH, int OW, void* stream) {
  if (!in || !out) return fail(EFFOCR_EINVAL, "convops_maxpool3x3s2: NULL argument");
  if (C < 4 || C % 4) return fail(EFFOCR_EUNSUPPORTED, "convops_maxpool3x3s2: C must be a multiple of 4");
  return maxpool3x3s2_nhwc(in, out, B, H, W, C, OH, OW, static_cast<hipStream_t>(stream));
}
CONVOPS_API int effocr_convops_avgpool(const float* in, float* out, int B, int HW, int C, int l2norm, void* stream) {
  if (!in || !out) return fail(EFFOCR_EINVAL, "convops_avgpool: NULL argument");
  return global_avgpool_nhwc(in, out, B, HW, C, l2norm, static_cast<hipStream_t>(stream));
}
CONVOPS_API int effocr_convops_stem6x6s2(const float* x, const float* w, int w_ld, const float* wt, const float* bias, float* out, int B, int H, int W,
                                         int OH, int OW, int out_ld, int out_off, int silu, void* stream) {
  if (!x || !w || !bias || !out) return fail(EFFOCR_EINVAL, "convops_stem6x6s2: NULL argument");
  return stem6x6s2_nchw(x, w, w_ld, wt, bias, out, B, H, W, OH, OW, out_ld, out_off, silu, static_cast<hipStream_t>(stream));
}
CONVOPS_API int effocr_convops_stem6x6s2_g16(const float* x, const float* wt, int wt_ld, const float* bias, float* out, int B, int H, int W, int OH,
                                             int OW, int out_ld, int out_off, int cout, int cout_st, void* stream) {
  if (!x || !wt || !bias || !out) return fail(EFFOCR_EINVAL, "convops_stem6x6s2_g16: NULL argument");
  return stem6x6s2_g16_nchw(x, wt, wt_ld, bias, out, B, H, W, OH, OW, out_ld, out_off, cout, cout_st, static_cast<hipStream_t>(stream));
}
CONVOPS_API int effocr_convops_upsample2x(const float* in, int in_ld, int in_off, float* out, int out_ld, int out_off, int B, int H, int W, int C,
                                          void* stream) {
  if (!in || !out) return fail(EFFOCR_EINVAL, "convops_upsample2x: NULL argument");
  return upsample2x_nhwc(in, in_ld, in_off, out, out_ld, out_off, B, H, W, C, static_cast<hipStream_t>(stream));
}
CONVOPS_API int effocr_convops_maxpool5(const float* in, int in_ld, int in_off, float* out, int out_ld, int out_off, int B, int H, int W, int C,
                                        void* stream) {
  if (!in || !out) return fail(EFFOCR_EINVAL, "convops_maxpool5: NULL argument");
  return maxpool5_nhwc(in, in_ld, in_off, out, out_ld, out_off, B, H, W, C, static_cast<hipStream_t>(stream));
}

CONVOPS_API int effocr_convops_im2col16(int prec, const float* x, void* col, int B, int H, int W, int OH, int OW, void* stream) {
  if (prec != PREC_BF16 && prec != PREC_FP16) return fail(EFFOCR_EINVAL, "convops_im2col16: prec must be bf16 (0) or f16 (1)");
  if (!x || !col) return fail(EFFOCR_EINVAL, "convops_im2col16: NULL argument");
  return rn_im2col16(prec, x, col, B, H, W, OH, OW, static_cast<hipStream_t>(stream));
}
CONVOPS_API int effocr_convops_maxpool16(int prec, const void* in, void* out, int B, int H, int W, int C, int OH, int OW, void* stream) {
  if (prec != PREC_BF16 && prec != PREC_FP16) return fail(EFFOCR_EINVAL, "convops_maxpool16: prec must be bf16 (0) or f16 (1)");
  if (!in || !out) return fail(EFFOCR_EINVAL, "convops_maxpool16: NULL argument");
  return rn_maxpool16(prec, in, out, B, H, W, C, OH, OW, static_cast<hipStream_t>(stream));
}
// prec: the element type of `in` (0 = bf16, 1 = f16, 2 = fp32); status: optional device int, ORed with 1 on a non-finite embedding
CONVOPS_API int effocr_convops_avgpool16(int prec, const void* in, float* emb, int B, int HW, int C, int l2norm, int* status, void* stream) {
  if (prec < 0 || prec > 2) return fail(EFFOCR_EINVAL, "convops_avgpool16: unknown element type");
  if (!in || !emb) return fail(EFFOCR_EINVAL, "convops_avgpool16: NULL argument");
  return rn_avgpool(prec, in, emb, B, HW, C, l2norm, status, static_cast<hipStream_t>(stream));
}

// ---- ConvNeXt (convnext.hip; layouts: kernels.hpp).  A shape the launcher refuses keeps the launcher's own code.
CONVOPS_API int effocr_convops_cnx_stem(const float* img, int B, int S, const float* wt, const float* bias, const float* lnw, const float* lnb, int C0,
                                        float* x, void* stream) {
  if (!img || !wt || !bias || !lnw || !lnb || !x) return fail(EFFOCR_EINVAL, "convops_cnx_stem: NULL argument");
  if (B < 0 || S < 0 || C0 < 0) return fail(EFFOCR_EINVAL, "convops_cnx_stem: negative size");
  return cnx_stem(img, B, S, wt, bias, lnw, lnb, C0, x, static_cast<hipStream_t>(stream));
}
CONVOPS_API int effocr_convops_cnx_dwconv_ln(int prec, const float* x, int B, int H, int W, int C, int Cp, const float* w, const float* bias,
                                             const float* lnw, const float* lnb, void* out, void* stream) {
  if (!x || !w || !bias || !lnw || !lnb || !out) return fail(EFFOCR_EINVAL, "convops_cnx_dwconv_ln: NULL argument");
  if (B < 0 || H < 1 || W < 1 || C < 1 || Cp < 1) return fail(EFFOCR_EINVAL, "convops_cnx_dwconv_ln: bad shape");
  return cnx_dwconv_ln(prec, x, B, H, W, C, Cp, w, bias, lnw, lnb, out, static_cast<hipStream_t>(stream));
}
CONVOPS_API int effocr_convops_cnx_ln_s2d(int prec, const float* x, int B, int H, int W, int C, int Cp, const float* lnw, const float* lnb, void* out,
                                          void* stream) {
  if (!x || !lnw || !lnb || !out) return fail(EFFOCR_EINVAL, "convops_cnx_ln_s2d: NULL argument");
  if (B < 0 || H < 1 || W < 1 || C < 1 || Cp < 1) return fail(EFFOCR_EINVAL, "convops_cnx_ln_s2d: bad shape");
  return cnx_ln_s2d(prec, x, B, H, W, C, Cp, lnw, lnb, out, static_cast<hipStream_t>(stream));
}
// status: optional device int, ORed with 1 on a non-finite embedding
CONVOPS_API int effocr_convops_cnx_head(const float* x, int B, int HW, int C, int Cp, const float* lnw, const float* lnb, int l2norm, float* emb,
                                        int* status, void* stream) {
  if (!x || !lnw || !lnb || !emb) return fail(EFFOCR_EINVAL, "convops_cnx_head: NULL argument");
  if (B < 0 || HW < 0 || C < 1 || Cp < 1) return fail(EFFOCR_EINVAL, "convops_cnx_head: bad shape");
  return cnx_head(x, B, HW, C, Cp, lnw, lnb, l2norm, emb, status, static_cast<hipStream_t>(stream));
}
// A linear of convnext_forward, dispatched as its `lin` lambda does (api.hip): gemm2_nt where gemm2_supported, gemm_nt otherwise.  Dense rows
// (ldx = ldw = k, ldo = ldr = n).  epilogue: 1 bias + GELU (out in the operand type), 5 bias (fp32 out), 4 fp32 out = resid + scale[n] (acc +
// bias[n]), resid may be out.
CONVOPS_API int effocr_convops_linear(int precision, int epilogue, const void* x, const void* w, const float* bias, const float* resid,
                                      const float* scale, void* out, int m, int n, int k, void* stream) {
  if (precision != PREC_BF16 && precision != PREC_FP16 && precision != PREC_FP32) return fail(EFFOCR_EINVAL, "convops_linear: unknown precision");
  if (epilogue != EPI_BIAS_GELU && epilogue != EPI_BIAS_F32 && epilogue != EPI_BIAS_SCALE_RESID)
    return fail(EFFOCR_EINVAL, "convops_linear: unknown epilogue (1 bias + GELU, 4 bias, layer scale + residual, 5 bias with fp32 output)");
  if (!x || !w || !bias || !out) return fail(EFFOCR_EINVAL, "convops_linear: NULL argument");
  if (epilogue == EPI_BIAS_SCALE_RESID && (!resid || !scale)) return fail(EFFOCR_EINVAL, "convops_linear: epilogue 4 needs resid and scale");
  if (m < 0 || n < 1 || k < 1) return fail(EFFOCR_EINVAL, "convops_linear: bad shape");
  if ((int64_t)m * std::max(n, k) >= (int64_t)1 << 31) return fail(EFFOCR_EUNSUPPORTED, "convops_linear: m * max(n, k) beyond 32-bit GEMM indices");
  GemmArgs g{};
  g.X = x; g.ldx = k; g.W = w; g.ldw = k; g.bias = bias; g.out = out; g.ldo = n; g.M = m; g.N = n; g.K = k;
  if (epilogue == EPI_BIAS_SCALE_RESID) { g.resid = resid; g.ldr = n; g.scale = scale; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  return gemm2_supported(precision, n, k) ? gemm2_nt(precision, epilogue, g, s) : gemm_nt(precision, epilogue, g, s);
}

// ---- the ViT path (patch.hip, vit_ops.hip, qkvattn.hip, EPI_PATCH of gemm.hip / gemm2.hip; layouts: kernels.hpp).  Buffers in the
// fragment-blocked layout must be addressable up to the next multiple of 32 rows.  A shape the launcher refuses keeps the launcher's own code.
// patch.hip patch_embed_fused: every field of PatchArgs + prec (0 = bf16, 1 = f16); cls may be NULL (the class-token rows stay as they are)
CONVOPS_API int effocr_convops_vit_patch_embed(int prec, const void* x, int x16, int B, int H, int W, const void* wb, const float* bias, const float* pos,
                                               const float* cls, float* out, int D, int P, void* stream) {
  convops_patch_dw = 0; convops_patch_grid = 0;
  if (!x || !wb || !bias || !pos || !out) return fail(EFFOCR_EINVAL, "convops_vit_patch_embed: NULL argument");
  if (B < 0 || H < 16 || W < 16 || D < 1 || P < 1) return fail(EFFOCR_EINVAL, "convops_vit_patch_embed: bad shape");
  if ((int64_t)B * (P + 1) >= (int64_t)1 << 31 || (int64_t)B * 3 * H * W >= (int64_t)1 << 40) return fail(EFFOCR_EUNSUPPORTED, "convops_vit_patch_embed: batch too large");
  PatchArgs a{};
  a.x = x; a.B = B; a.H = H; a.W = W; a.x16 = x16 ? 1 : 0; a.Wb = wb; a.bias = bias; a.pos = pos; a.cls = cls; a.out = out; a.D = D; a.P = P;
  return patch_embed_fused(prec, a, static_cast<hipStream_t>(stream));
}
// slice width (128 / 256 / 384) and grid of the calling thread's last effocr_convops_vit_patch_embed launch (0, 0: nothing was launched)
CONVOPS_API void effocr_convops_vit_patch_embed_last_dispatch(int* dw, int* grid) {
  if (dw) *dw = convops_patch_dw;
  if (grid) *grid = convops_patch_grid;
}
// vit_ops.hip im2col_patch16: crops [B,3,H,W] (fp32, or with x16 already prec's 16-bit type) -> patch rows [B * (H/16) * (W/16)][768] in prec's type
CONVOPS_API int effocr_convops_vit_im2col16(int prec, const void* x, int x16, int B, int H, int W, void* col, void* stream) {
  if (!x || !col) return fail(EFFOCR_EINVAL, "convops_vit_im2col16: NULL argument");
  if (B < 0 || H < 16 || W < 16) return fail(EFFOCR_EINVAL, "convops_vit_im2col16: bad shape");
  return im2col_patch16(prec, x, x16 ? 1 : 0, B, H, W, col, static_cast<hipStream_t>(stream));
}
// EPI_PATCH dispatched as vit_forward does (api.hip): gemm2_nt where gemm2_supported(prec, D, 768), gemm_nt otherwise.  col [B * P][768] and w
// [D][768] in prec's type, dense rows; fp32 out rows img * (P + 1) + 1 + p = acc + pos[1 + p] + bias, row-major [.][D] or (blk_out, gemm2 only)
// fragment-blocked; the class-token rows are not written.
CONVOPS_API int effocr_convops_vit_patch_gemm(int prec, const void* col, const void* w, const float* bias, const float* pos, float* out, int B, int P,
                                              int D, int blk_out, void* stream) {
  if (prec != PREC_BF16 && prec != PREC_FP16 && prec != PREC_FP32) return fail(EFFOCR_EINVAL, "convops_vit_patch_gemm: unknown precision");
  if (!col || !w || !bias || !pos || !out) return fail(EFFOCR_EINVAL, "convops_vit_patch_gemm: NULL argument");
  if (B < 0 || P < 1 || D < 1) return fail(EFFOCR_EINVAL, "convops_vit_patch_gemm: bad shape");
  if ((int64_t)B * (P + 1) * std::max(D, 768) >= (int64_t)1 << 31) return fail(EFFOCR_EUNSUPPORTED, "convops_vit_patch_gemm: rows * max(D, 768) beyond 32-bit GEMM indices");
  const bool g2 = gemm2_supported(prec, D, 768);
  if (blk_out && !g2) return fail(EFFOCR_EUNSUPPORTED, "convops_vit_patch_gemm: only gemm2 (16-bit operands, D % 128 == 0) writes the fragment-blocked layout");
  GemmArgs g{};
  g.X = col; g.ldx = 768; g.W = w; g.ldw = 768; g.bias = bias; g.out = out; g.ldo = D; g.pos = pos; g.M = B * P; g.N = D; g.K = 768; g.P = P;
  g.blk_out = blk_out ? 1 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return g2 ? gemm2_nt(prec, EPI_PATCH, g, s) : gemm_nt(prec, EPI_PATCH, g, s);
}
// vit_ops.hip set_cls_rows: row img * T of x [B * T][D] fp32 (row-major or blocked) = cls_pos0; status_zero (optional device int) is set to 0
CONVOPS_API int effocr_convops_vit_set_cls(const float* cls_pos0, float* x, int B, int T, int D, int blocked, int* status_zero, void* stream) {
  if (!cls_pos0 || !x) return fail(EFFOCR_EINVAL, "convops_vit_set_cls: NULL argument");
  if (B < 0 || T < 1 || D < 4 || D % 4) return fail(EFFOCR_EINVAL, "convops_vit_set_cls: bad shape (D must be a multiple of 4)");
  return set_cls_rows(cls_pos0, x, B, T, D, blocked ? 1 : 0, status_zero, static_cast<hipStream_t>(stream));
}
// vit_ops.hip gather_cls_rows_blocked: rows img * T of x (fp32 blocked) and att (16-bit blocked) -> rows img of xc / ac (blocked, B rows)
CONVOPS_API int effocr_convops_vit_gather_cls(const float* x, const void* att, int B, int T, int D, float* xc, void* ac, void* stream) {
  if (!x || !att || !xc || !ac) return fail(EFFOCR_EINVAL, "convops_vit_gather_cls: NULL argument");
  if (B < 0 || T < 1 || D < 8 || D % 8) return fail(EFFOCR_EINVAL, "convops_vit_gather_cls: bad shape (D must be a multiple of 8)");
  return gather_cls_rows_blocked(x, att, B, T, D, xc, ac, static_cast<hipStream_t>(stream));
}
// qkvattn.hip qkv_attn_fused: every field of QkvAttnArgs a caller sets (img0 is the launcher's) + prec
CONVOPS_API int effocr_convops_vit_qkv_attn(int prec, const void* xn, const void* wb, const float* bias, void* out, int B, int T, int D, int64_t rows_alloc,
                                            int cls_only, int hsplit, void* stream) {
  convops_qa_launches = 0;
  std::fill(&convops_qa_last[0][0], &convops_qa_last[0][0] + 12, 0);
  if (!xn || !wb || !bias || !out) return fail(EFFOCR_EINVAL, "convops_vit_qkv_attn: NULL argument");
  if (B < 0 || T < 1 || D < 1 || rows_alloc < 0 || hsplit < 0) return fail(EFFOCR_EINVAL, "convops_vit_qkv_attn: bad shape");
  QkvAttnArgs a{};
  a.xn = xn; a.Wb = wb; a.bias = bias; a.out = out; a.B = B; a.T = T; a.D = D; a.rows_alloc = rows_alloc; a.cls_only = cls_only ? 1 : 0; a.hsplit = hsplit;
  return qkv_attn_fused(prec, a, static_cast<hipStream_t>(stream));
}
// launches of the calling thread's last effocr_convops_vit_qkv_attn (0 .. 2: the split tail of a batch is a second one); out6 (optional) takes
// launch `which`: {D, token tiles, 1 = class-token form, P.V steps (13: short tail, 14), head split, grid}
CONVOPS_API int effocr_convops_vit_qkv_attn_last_dispatch(int which, int* out6) {
  if (out6 && which >= 0 && which < 2) std::copy(convops_qa_last[which], convops_qa_last[which] + 6, out6);
  return convops_qa_launches;
}
// vit_ops.hip final_cls_norm: LayerNorm of row img * T of x (fp32, row-major or blocked) (+ F.normalize) -> emb [B][D]; status: optional device
// int, ORed with 1 on a non-finite embedding
CONVOPS_API int effocr_convops_vit_final_norm(const float* x, int B, int T, int D, const float* gamma, const float* beta, float eps, int l2norm,
                                              int blocked, float* emb, int* status, void* stream) {
  if (!x || !gamma || !beta || !emb) return fail(EFFOCR_EINVAL, "convops_vit_final_norm: NULL argument");
  if (B < 0 || T < 1 || D < 1) return fail(EFFOCR_EINVAL, "convops_vit_final_norm: bad shape");
  return final_cls_norm(x, B, T, D, gamma, beta, eps, l2norm ? 1 : 0, blocked ? 1 : 0, emb, status, static_cast<hipStream_t>(stream));
}

// ---- the YOLOv5 Detect decode (yolo.hip yolo_decode): raw [B * ny * nx][raw_ld] (channel an * no + o) -> rows row0 .. row0 + na * ny * nx
// of pred [B][total][no]; anchors_px: the level's na (w, h) pairs in input pixels, on the HOST.  na != 3 keeps the launcher's own code.
CONVOPS_API int effocr_convops_yolo_decode(const float* raw, int raw_ld, float* pred, int B, int ny, int nx, int na, int no, float stride,
                                           const float* anchors_px, int64_t total, int64_t row0, void* stream) {
  if (!raw || !pred || !anchors_px) return fail(EFFOCR_EINVAL, "convops_yolo_decode: NULL argument");
  if (B < 0 || ny < 1 || nx < 1 || na < 1 || no < 5 || (int64_t)raw_ld < (int64_t)na * no) return fail(EFFOCR_EINVAL, "convops_yolo_decode: bad shape");
  if (total < 1 || row0 < 0 || row0 + (int64_t)na * ny * nx > total) return fail(EFFOCR_EINVAL, "convops_yolo_decode: the level's rows do not fit the prediction tensor");
  return yolo_decode(raw, raw_ld, pred, B, ny, nx, na, no, stride, anchors_px, total, row0, static_cast<hipStream_t>(stream));
}
