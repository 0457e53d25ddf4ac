// Internal launcher interface of libeffocr_resnet.so's 16-bit ResNet path (resnet16.hip -> resnet_api.hip).  Every kernel computes an
// output pixel (or a crop's embedding) from that crop's inputs alone, in a fixed order: embeddings do not depend on the call size.
#pragma once
#include "common.hpp"

namespace effocr {

constexpr int RN_STEM_K16 = 192;   // stem im2col columns in the 16-bit modes: 7*7*3 = 147 taps padded to 3 K-stages of 64

struct Conv16Args {
  const void* in;       // NHWC [B,H,W,Cin] in the operand type
  const void* w;        // [Cout][KH*KW*Cin] in the operand type, BN folded, K = (ky, kx, ci) with ci fastest
  const float* bias;    // [Cout] folded BN shift
  const void* resid;    // optional NHWC [B,OH,OW,Cout] in the operand type, added before the ReLU
  void* out;            // NHWC [B,OH,OW,Cout] in the operand type
  int B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW, relu;
};
// prec: PREC_FP16 or PREC_BF16.  Cin % 64 == 0, Cout % 64 == 0.
int rn_conv16(int prec, const Conv16Args& a, hipStream_t s);
// stem im2col straight from the fp32 NCHW crops: col [B*OH*OW][RN_STEM_K16] in the operand type ((ky*7+kx)*3 + c, zero padded)
int rn_im2col16(int prec, const float* x, void* col, int B, int H, int W, int OH, int OW, hipStream_t s);
// max_pool2d(3, 2, 1) on NHWC in the operand type
int rn_maxpool16(int prec, const void* in, void* out, int B, int H, int W, int C, int OH, int OW, hipStream_t s);
// global average pool of NHWC [B][HW][C] (prec's type: bf16, f16 or fp32) in fp32 -> emb [B][C] fp32 (+ F.normalize); ORs 1 into *status
// on a non-finite embedding.  C % 256 == 0, C <= 2048.
int rn_avgpool(int prec, const void* in, float* emb, int B, int HW, int C, int l2norm, int* status, hipStream_t s);

}  // namespace effocr
