// Internal launcher interface of libeffocr_mnv3.so (mnv3g.hip -> mnv3g_api.hip): the MobileNetV3 forward whose activations live in HBM
// between blocks, fp32 and channels-last [crop][pixel][C].  Every launcher enqueues ONE kernel on the stream and returns an EFFOCR_* code.
// Every kernel computes a crop's values from that crop's data alone, in an order fixed by the shapes: no float atomics, one kernel form
// for every call size.
#pragma once
#include "common.hpp"
#include "kernels.hpp"

namespace effocr {

enum { MG_ACT_NONE = 0, MG_ACT_RELU = 1, MG_ACT_HS = 2, MG_ACT_SILU = 3 };   // SILU: libeffocr_effnet.so's forward only
constexpr int MG_STEM_C = 16;          // stem channels of every supported width (fixed 16 below 0.75, make_divisible(16 m) = 16 up to 1.0)

// stem: x [B,3,S,S] fp32 NCHW -> out [B,S/2,S/2,16] = hard-swish(conv3x3/2 pad 1 (x; w [27][16] tap-major, BN folded) + b)
int mg_stem(const float* x, int B, int S, const float* w, const float* b, float* out, hipStream_t s);

// depthwise k x k (3 or 5), stride 1 or 2, pad k/2: in [B,H,H,C] -> out [B,Ho,Ho,C] = act(conv + b); w [k*k][C] tap-major fp32; C % 4 == 0
int mg_dw(const float* in, int B, int H, int C, int k, int stride, const float* w, const float* b, int act, float* out, int Ho, hipStream_t s);

// squeeze-excite gate of one crop per workgroup: means of t [B,HW,C] over the pixels (fixed order) -> ReLU(wr m + br) [R] ->
// gate [B,C] = hardsigmoid(we h + be).  wr [R][C], we [C][R] fp32.
int mg_se_gate(const float* t, int B, int HW, int C, int R, const float* wr, const float* br, const float* we, const float* be, float* gate,
               hipStream_t s);

// pointwise conv as a GEMM: out [M,N] = act((a [M,K] * (gate ? gate[row / HW][k] : 1)) . w[N,K]^T + bias) (+ resid [M,N]).
// prec 16-bit: w is [Npad16][Kpad16] of the operand type (zero padded), MFMA 16x16x16 with the activation as hi + lo parts;
// fp32: w is [N][K] fp32, one FMA chain per output, k ascending.  K % 4 == 0, N % 4 == 0.
int mg_pw(int prec, const float* a, int64_t M, int K, const void* w, int N, const float* bias, const float* gate, int HW, int act,
          const float* resid, float* out, hipStream_t s);

// global average pool: t [B,HW,C] -> out [B,C], pixels summed in order
int mg_pool(const float* t, int B, int HW, int C, float* out, hipStream_t s);

// in place on emb [B,D]: F.normalize when l2 != 0; a non-finite value ORs 1 into *status
int mg_finish(float* emb, int B, int D, int l2, int* status, hipStream_t s);

}  // namespace effocr
