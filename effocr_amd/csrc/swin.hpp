// Internal launcher interface of libeffocr_swin.so (swin.hip -> swin_api.hip).  Every kernel computes a token (or a crop's embedding)
// from that crop's inputs alone, in a fixed order: embeddings do not depend on the call size or the chunking.
#pragma once
#include "common.hpp"

namespace effocr {

// patch_embed: 4x4/s4 conv (wt: [48 taps (c, ky, kx)][128] fp32) + LayerNorm over C0 <= 128 -> x [B*(S/4)^2][128] fp32 (pad channels 0)
int swin_stem(const float* img, int B, int S, const float* wt, const float* bias, const float* lnw, const float* lnb, int C0, float eps,
              float* x, hipStream_t s);
// LayerNorm over the C real channels of x [M][Cp] fp32 -> out [M][Cp] in prec's type (pad channels 0)
int swin_layernorm(int prec, const float* x, int64_t M, int C, int Cp, const float* lnw, const float* lnb, float eps, void* out, hipStream_t s);
// patch merging: 2x2 gather in timm's order + LayerNorm over 4C -> out [B*(H/2)^2][4C] in prec's type
int swin_merge(int prec, const float* x, int B, int H, int C, int Cp, const float* lnw, const float* lnb, float eps, void* out, hipStream_t s);
// 7x7 (shifted-)window attention, head dim 32: qkv [B*H*H][3][Cp] -> out [B*H*H][Cp] (prec's type; pad channels 0);
// table: relative_position_bias_table [169][C / 32] fp32; shift 0 (W-MSA) or 3 (SW-MSA)
int swin_window_attention(int prec, const void* qkv, int B, int H, int C, int Cp, int shift, const float* table, void* out, hipStream_t s);
// final LayerNorm of every token, mean over the HW tokens (+ F.normalize) -> emb [B][C]; ORs 1 into *status on a non-finite embedding
int swin_head(const float* x, int B, int HW, int C, int Cp, const float* lnw, const float* lnb, float eps, int l2norm, float* emb, int* status,
              hipStream_t s);

}  // namespace effocr
