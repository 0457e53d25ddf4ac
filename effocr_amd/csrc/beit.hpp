// Internal launcher interface of libeffocr_beit.so (beit.hip -> beit_api.hip).  Every kernel computes a crop's rows from that crop's
// inputs alone, in a fixed order: embeddings do not depend on the call size or the chunking.
#pragma once
#include "common.hpp"

namespace effocr {

constexpr int BEIT_MAX_W = 14;                           // patches per side at 224^2: T = W^2 + 1 <= 197 tokens, 7 key tiles of 32

// entries of one head's relative-position bias table for a W x W patch grid: (2W-1)^2 patch offsets + cls->any, any->cls, cls->cls
__host__ __device__ static inline int beit_table_entries(int W) { return (2 * W - 1) * (2 * W - 1) + 3; }

// Multi-head attention with BEiT's additive relative-position bias, head dim 64, T = W^2 + 1 tokens (token 0 = cls, token 1 + y W + x =
// patch (y, x)):  out = softmax(q k^T / 8 + table[index(i, j)][h]) v
//   qkv   [B*T][3*heads*64] in prec's type (q | k | v, feature = which * D + h * 64 + d)
//   table [beit_table_entries(W)][heads] fp32
//   out   [B*T][heads*64] in prec's type (feature = h * 64 + d)
// 16-bit modes: MFMA tiles, softmax and bias in fp32; fp32 mode: plain fp32 arithmetic.
int beit_attention(int prec, const void* qkv, const float* table, int B, int W, int heads, void* out, hipStream_t s);

// head: mean over the T - 1 patch tokens of x [B*T][D] fp32 (cls excluded, ascending token order), LayerNorm fc_norm (+ F.normalize)
// -> emb [B][D]; ORs 1 into *status on a non-finite embedding
int beit_head(const float* x, int B, int T, int D, const float* lnw, const float* lnb, float eps, int l2norm, float* emb, int* status,
              hipStream_t s);

}  // namespace effocr
