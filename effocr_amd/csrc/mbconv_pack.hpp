// What the two MBConv families (mnv3g_api.hip, effnet_api.hip) share on the host: the squeeze-excite parameter names, the blob layout of a
// pointwise weight and the BatchNorm fold.  The block tables, the squeeze-excite packing and the forwards are each family's own.
#pragma once
#include "enc_core.hpp"

#include <math.h>

namespace effocr {

struct ConvOff { size_t w = 0, b = 0; };                 // blob offsets of one convolution's weight and bias

// timm SqueezeExcite of block `p`: c channels, reduced to r
static inline void add_se(EncoderCore* e, const std::string& p, int c, int r) {
  e->add_param(p + ".se.conv_reduce.weight", (int64_t)r * c); e->add_param(p + ".se.conv_reduce.bias", r);
  e->add_param(p + ".se.conv_expand.weight", (int64_t)c * r); e->add_param(p + ".se.conv_expand.bias", c);
}

static inline size_t pw_bytes(int prec, int N, int K) {
  if (prec == PREC_FP32) return (size_t)N * K * 4;
  return (size_t)align_up(N, 16) * align_up(K, 16) * 2;       // zero-padded to whole 16 x 16 MFMA tiles
}
// pointwise weight [N][K] fp32 -> the blob: fp32 as it is, else rounded once to the operand type inside a zeroed [N16][K16] frame
static inline void put_pw(int prec, std::vector<char>& blob, size_t off, const float* w, int N, int K) {
  if (prec == PREC_FP32) { memcpy(blob.data() + off, w, (size_t)N * K * 4); return; }
  const int Kp = (int)align_up(K, 16);
  uint16_t* d = reinterpret_cast<uint16_t*>(blob.data() + off);   // (the blob starts zeroed)
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) d[(size_t)n * Kp + k] = prec == PREC_BF16 ? f32_to_bf16(w[(size_t)n * K + k]) : f32_to_f16(w[(size_t)n * K + k]);
}

// check_status in f16 mode, both families
constexpr const char* MBCONV_FP16_OVERFLOW =
    "forward: non-finite embedding — an f16 operand overflowed (an activation beyond 65504) or the input was not finite; use "
    "precision bf16 or fp32 for this checkpoint";

static inline int out_size(int H, int stride) { return (H - 1) / stride + 1; }   // k x k, pad k / 2 (or TensorFlow SAME)

// A BatchNorm (eval) folded into the conv in front of it in fp32: w' = w g / sqrt(v + eps), b' = beta - m g / sqrt(v + eps); the folded
// conv goes into the blob as a pointwise weight (pw) or tap-major [taps][C] fp32 (depthwise and stem), its bias as fp32.
struct BnFolder {
  const EncoderCore* e;
  std::vector<char>& blob;
  float eps;
  std::vector<float> wf, bf;

  void fold(const std::string& w, const std::string& bn) {
    const auto& W = e->P(w);
    const auto& g = e->P(bn + ".weight"); const auto& be = e->P(bn + ".bias");
    const auto& m = e->P(bn + ".running_mean"); const auto& v = e->P(bn + ".running_var");
    const size_t C = g.size(), per = W.size() / C;
    wf.resize(W.size()); bf.resize(C);
    for (size_t c = 0; c < C; ++c) {
      const float sc = g[c] / sqrtf(v[c] + eps);
      for (size_t k = 0; k < per; ++k) wf[c * per + k] = W[c * per + k] * sc;
      bf[c] = be[c] - m[c] * sc;
    }
  }
  void pw(const ConvOff& c, const std::string& w, const std::string& bn, int N, int K) {
    fold(w, bn); put_pw(e->prec, blob, c.w, wf.data(), N, K); put_f32(blob, c.b, bf.data(), bf.size());
  }
  void tapmajor(const ConvOff& c, const std::string& w, const std::string& bn, int C, int taps) {
    fold(w, bn);
    float* d = reinterpret_cast<float*>(blob.data() + c.w);
    for (int ch = 0; ch < C; ++ch)
      for (int t = 0; t < taps; ++t) d[(size_t)t * C + ch] = wf[(size_t)ch * taps + t];
    put_f32(blob, c.b, bf.data(), bf.size());
  }
};

}  // namespace effocr
