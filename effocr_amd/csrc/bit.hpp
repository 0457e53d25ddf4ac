// Internal launcher interface of libeffocr_bit.so's own kernels (bit.hip -> bit_api.hip): what a BiT ResNetV2 needs beyond the
// convolutions of resnet16.hip / resnet.hip.  Activations are NHWC [B][HW][C] in prec's type (bf16, f16 or fp32).  Every kernel computes a
// crop's values from that crop's data alone, in an order the geometry (HW, C) fixes: results do not depend on the call size.
#pragma once
#include "common.hpp"

namespace effocr {

constexpr int BIT_GROUPS = 32;        // GroupNorm groups of every BiT norm
constexpr float BIT_GN_EPS = 1e-5f;
constexpr int BIT_GN_TILE = 16384;    // elements (pixels x channels) of one statistics / apply tile

// pixels per GroupNorm tile and tiles per crop: functions of the geometry alone
static inline int bit_gn_tile_pixels(int C) { return BIT_GN_TILE / C > 0 ? BIT_GN_TILE / C : 1; }
static inline int bit_gn_tiles(int HW, int C) { const int tp = bit_gn_tile_pixels(C); return (HW + tp - 1) / tp; }
constexpr int BIT_GN_REC = 4;         // floats per (tile, group) record: mean - shift, M2, shift, unused
// bytes of the per-tile partial statistics of B crops
static inline size_t bit_gn_scratch_bytes(int B, int HW, int C) { return (size_t)B * bit_gn_tiles(HW, C) * BIT_GROUPS * BIT_GN_REC * sizeof(float); }

// out = relu(GroupNorm_32(in) * gamma + beta), rounded once to prec's type; out may alias in.  C % 64 == 0, C <= 2048.
// partial: bit_gn_scratch_bytes(B, HW, C) bytes of scratch.
int bit_groupnorm_relu(int prec, const void* in, void* out, int B, int HW, int C, const float* gamma, const float* beta, float* partial,
                       hipStream_t s);
// max_pool2d(constant_pad(in, 1, value 0), 3, 2): zero padding takes part in the maximum.  C % 8 == 0.
int bit_stem_pool(int prec, const void* in, void* out, int B, int H, int W, int C, int OH, int OW, hipStream_t s);
// emb [B][C] fp32 = mean over HW of relu(GroupNorm_32(in) * gamma + beta), all in fp32 (+ F.normalize when l2norm); ORs 1 into *status on a
// non-finite embedding.  C % 256 == 0, C <= 2048.
int bit_head(int prec, const void* in, float* emb, int B, int HW, int C, const float* gamma, const float* beta, int l2norm, int* status,
             hipStream_t s);

}  // namespace effocr
