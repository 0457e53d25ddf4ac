// Internal launcher interface of libeffocr_vit8.so (vit8.hip -> vit8_api.hip).  Every kernel computes a crop's rows from that crop's
// inputs alone, in a fixed order: embeddings do not depend on the call size or the chunking.
#pragma once
#include "common.hpp"

namespace effocr {

constexpr int VIT8_PATCH = 8, VIT8_PATCH_K = 3 * VIT8_PATCH * VIT8_PATCH;   // 8x8 patches: im2col rows of K = 192
constexpr int VIT8_MAX_W = 28;                           // patches per side at 224^2: T = W^2 + 1 <= 785 tokens
constexpr int VIT8_MAX_T = 1024;                         // vit8_attention itself takes any 1 <= T <= 1024

// Tile sizes of vit8_attention (tests/test_gpu_vit8.py places its token counts around them)
constexpr int VIT8_QBLK = 128;                           // queries per workgroup, every mode (16-bit: 4 waves x 32; fp32: 128 threads x 1)
constexpr int VIT8_KTILE16 = 64;                         // keys per tile, 16-bit modes (two 32-key MFMA sub-tiles)
constexpr int VIT8_KTILE32 = 32;                         // keys per tile, fp32 mode

// Streaming multi-head attention, head dim 64:  out = softmax(q k^T / 8) v  for any T from 1 to VIT8_MAX_T, without the T x T scores ever
// leaving the registers.
//   qkv [B*T][3*heads*64] in prec's type (q | k | v, feature = which * D + h * 64 + d; beit_attention's layout)
//   out [B*T][heads*64] in prec's type (feature = h * 64 + d)
// One workgroup per (crop, head, block of VIT8_QBLK queries).  It walks the key tiles in ascending order with a running row maximum m
// and row sum l (online softmax), rescaling on EVERY tile (no deferred-rescale threshold):
//   m' = max(m, max_j s_j)   alpha = exp((m - m') / 8)   p_j = exp((s_j - m') / 8)   l = alpha l + sum_j p_j   O = alpha O + P V
// with s = q . k the raw dot product.  Keys at or beyond T in the last tile score -inf: their weight is exactly 0 (and their K / V rows
// are staged as zeros, never read from the next crop).  Query slots at or beyond T repeat row T - 1 and are not stored.
// Rounding points of the 16-bit modes (tests/vit8_ref.py: attention_emulated restates them):
//   - q, k, v arrive in the operand type; s, m, l, alpha and the O accumulator are fp32;
//   - p_j is rounded to the operand type for the P V MFMA; l sums the UNROUNDED fp32 p_j;
//   - O / l is rounded once to the operand type on the store.
// fp32 mode: the same walk in plain fp32 arithmetic, one query per thread.
int vit8_attention(int prec, const void* qkv, int B, int T, int heads, void* out, hipStream_t s);

// Patch embedding for 8x8 patches: x [B,3,img,img] fp32 NCHW -> im2col rows col [B*P][192] in prec's type (k = c*64 + ky*8 + kx, the conv
// weight's own flattening) -> GEMM with w [D][192] (prec's type) + bias [D] + pos[1 + p] into rows b*T + 1 + p of the fp32 residual stream
// out [B*T][D]; row b*T = cls_pos0 (cls_token + pos[0], pre-added).  P = (img/8)^2, T = P + 1, pos [T][D] fp32.
int vit8_patch_embed(int prec, const float* x, int B, int img, int D, const void* w, const float* bias, const float* cls_pos0,
                     const float* pos, void* col, float* out, hipStream_t s);

}  // namespace effocr
