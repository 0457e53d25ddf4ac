// Host-side core of the residual nets (ResNet-34/50, BiT ResNetV2), on top of enc_core.hpp: a convolution's geometry, the fp32 / 16-bit
// dispatcher, the weight relayout, the stem as im2col + 1x1, the four-buffer workspace with its rotation and the index guard.
// No kernel: include it from the family's *_api.hip after enc_core.hpp's rules (one translation unit per library).
#pragma once
#include "enc_core.hpp"
#include "resnet16.hpp"

namespace effocr {

constexpr int RES_STEM_K32 = 160;   // fp32 stem im2col columns (resnet.hip's im2col_conv1: 147 taps padded to 5 K-stages of 32)

// one convolution: geometry and blob offset of its weights [cout][kpad] in the operand type (kpad = k * k * cin, the stem's padded)
struct ConvGeom { int cin, cout, k, stride, pad, kpad; size_t w_off; };

// torch [Cout,Cin,KH,KW] -> [Cout][KH][KW][Cin] (Cin fastest), zero-padded to kpad columns; output channel co becomes
// (w - mean[co]) * scale[co], computed in double and rounded once to fp32.
static inline std::vector<float> relayout_ohwi(const std::vector<float>& w, const ConvGeom& c, const std::vector<double>& mean,
                                               const std::vector<double>& scale) {
  std::vector<float> wd((size_t)c.cout * c.kpad, 0.f);
  for (int co = 0; co < c.cout; ++co)
    for (int ky = 0; ky < c.k; ++ky)
      for (int kx = 0; kx < c.k; ++kx)
        for (int cc = 0; cc < c.cin; ++cc) {
          const float v = w[(((size_t)co * c.cin + cc) * c.k + ky) * c.k + kx];
          wd[(size_t)co * c.kpad + (ky * c.k + kx) * c.cin + cc] = (float)(((double)v - mean[co]) * scale[co]);
        }
  return wd;
}

// the integer fields ConvArgs and Conv16Args name alike
template <typename Args>
static inline void conv_geometry(Args& a, const ConvGeom& c, int B, int H, int W, int OH, int OW, int relu) {
  a.B = B; a.H = H; a.W = W; a.Cin = c.kpad / (c.k * c.k); a.Cout = c.cout; a.KH = c.k; a.KW = c.k; a.stride = c.stride; a.pad = c.pad;
  a.OH = OH; a.OW = OW; a.relu = relu;
}
// one convolution with the epilogue + bias [cout], + residual, ReLU.  16-bit modes: resnet16.hip's kernel; fp32: resnet.hip's with no
// split-K scratch (its split count would depend on the number of output pixels, i.e. on the call size).
static inline int launch_conv(int prec, const char* wdev, const ConvGeom& c, const float* bias, const void* in, int B, int H, int W, int OH,
                              int OW, const void* resid, int relu, void* out, hipStream_t s) {
  if (prec == PREC_FP32) {
    ConvArgs a{};
    a.in = static_cast<const float*>(in); a.w = reinterpret_cast<const float*>(wdev + c.w_off);
    a.bias = bias; a.resid = static_cast<const float*>(resid); a.out = static_cast<float*>(out);
    conv_geometry(a, c, B, H, W, OH, OW, relu);
    return conv2d_nhwc(a, s);
  }
  Conv16Args a{};
  a.in = in; a.w = wdev + c.w_off; a.bias = bias; a.resid = resid; a.out = out;
  conv_geometry(a, c, B, H, W, OH, OW, relu);
  return rn_conv16(prec, a, s);
}

// the 7x7/2 stem of B crops of H x H: im2col into `col`, then its rows as a 1x1 convolution over B * (H/2)^2 "images" of one pixel
static inline int stem_as_1x1(int prec, const char* wdev, ConvGeom stem, const float* bias, const float* x, void* col, int B, int H, int relu,
                              void* out, hipStream_t s) {
  const int OH = H / 2;
  const int rc = prec == PREC_FP32 ? im2col_conv1(x, static_cast<float*>(col), B, H, H, OH, OH, s) : rn_im2col16(prec, x, col, B, H, H, OH, OH, s);
  if (rc) return rc;
  stem.k = 1; stem.stride = 1; stem.pad = 0;
  return launch_conv(prec, wdev, stem, bias, col, B * OH * OH, 1, 1, 1, 1, nullptr, relu, out, s);
}

// Workspace of one sub-batch of B crops: the status word, `extra_bytes` of the family's own, and four activation buffers, each as large as
// the largest activation (the stem's output, S/2 x S/2 x 64, equals the first stage's output S/4 x S/4 x 256).  The stem's im2col rows
// overlay buffers 1-3, which are free until the pool.
struct ResWs { size_t status, extra, buf[4], total; };
static inline ResWs res_ws(int B, int img, int stem_kpad, size_t es, size_t extra_bytes) {
  const size_t s2 = (size_t)(img / 2) * (img / 2);
  const size_t act = align_up((size_t)B * s2 * 64 * es, 256);
  const size_t col = (size_t)B * s2 * stem_kpad * es;
  Alloc a; ResWs w;
  w.status = a.take(256);                   // int32 status word at workspace offset 0 (enc_check_status)
  w.extra = a.take(extra_bytes);
  w.buf[0] = a.take(act);
  const size_t rest = a.take(std::max(3 * act, col));
  for (int i = 1; i < 4; ++i) w.buf[i] = rest + (size_t)(i - 1) * act;
  w.total = a.off;
  return w;
}
// the three buffers a block may write while buffer `cur` holds its input
static inline void free_bufs(int cur, int t[3]) {
  for (int i = 0, n = 0; i < 4; ++i) if (i != cur) t[n++] = i;
}

// the kernels index with 32 bits: the largest array of a sub-batch is the stem's im2col [chunk (S/2)^2][kpad]
static inline bool res_index_ok(int chunk, int img, int stem_kpad) {
  return (int64_t)chunk * (img / 2) * (img / 2) * stem_kpad < (int64_t)1 << 31;
}

}  // namespace effocr
