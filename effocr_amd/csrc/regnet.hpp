// Internal launcher interface of libeffocr_regnet.so (regnet.hip -> regnet_api.hip): the RegNetX / RegNetY kernels that mnv3g.hip does not
// have.  Activations are fp32 channels-last [crop][pixel][C] in HBM between launches, as in mnv3g.hpp, whose mg_pw / mg_pool / mg_finish
// the forward also uses.  Every launcher enqueues ONE kernel on the stream and returns an EFFOCR_* code; every kernel computes a crop's
// values from that crop's data alone, in an order fixed by the shapes: no float atomics, one kernel form for every call size.
//
// The grouped 3x3 convolution (rg_gconv), 16-bit modes.  One wave computes RG_CH_TILE = 16 output channels x 16 output pixels on
// v_mfma_f32_16x16x16 with the weights as the A operand (as mg_pw), K walked as 9 taps x the 16-channel input tiles of the WINDOW of
// output tile ct: the input channels of every group that owns one of the tile's output channels, widened to whole 16-channel tiles,
//     lo = (16 ct / gw) gw,  hi = min(C, ((16 ct + 15) / gw + 1) gw),  input tiles lo / 16 .. ceil(hi / 16) - 1      (rg_window).
// The host packs the weight as [ct][tap][j < RG_NKT(gw)][16 out][16 in] with ZERO where the output and the input channel are in
// different groups (or outside C), so the MFMA sees a dense 16 x 16 block per (tap, input tile):
//     gw 16   the window is the tile's own group: 1 input tile, nothing wasted;
//     gw  8   two groups share a tile: 1 input tile, a block-diagonal weight, 1/2 of the MFMA work multiplies zeros (an odd group count
//             leaves the last tile half filled: its upper 8 rows and columns are zeros too);
//     gw 24   groups span tiles; output tiles repeat with period 3 (48 channels = 2 groups): tile 0 lies in group 0 (input 0..23, 2
//             tiles), tile 1 in groups 0 and 1 (input 0..47, 3 tiles), tile 2 in group 1 (input 24..47, 2 tiles): 7 input tiles where
//             4.5 hold weights, 5/14 = 36 % of the MFMA work multiplies zeros.
// Rounding points, 16-bit modes (tests/regnet_ref.py: gconv_emulated):
//     w16 = rn16(w)                              the BN-folded fp32 weight, rounded once on the host
//     x   = hi + lo,  hi = rn16(x), lo = rn16(x - hi)      the fp32 activation as two operands of the mode's type (two MFMAs per K step)
//     acc = sum over (tap, channel) of w16 hi + w16 lo     products exact, accumulated in fp32 from 0, taps then input tiles ascending
//     out = max(acc + bias, 0)                   fp32
// fp32 mode: one fp32 FMA chain per output from 0, taps ascending, the group's channels ascending inside a tap; then + bias, ReLU.
// A tap outside the map contributes an exact zero (operand 0, never a load).
#pragma once
#include "common.hpp"
#include "kernels.hpp"

namespace effocr {

constexpr int RG_STEM_C = 32;          // stem channels of every RegNetX / RegNetY
constexpr int RG_CH_TILE = 16;         // rg_gconv: output channels per wave (one MFMA tile)
constexpr int RG_PIX_TILE = 64;        // rg_gconv: output pixels per workgroup (row-major run inside a crop) = one tile of the tile sums
constexpr int RG_SE_MAXC = 1024, RG_SE_MAXR = 256;   // the gate kernel's LDS tables (widest: regnety_016, C 888, R 222)

// tiles of an Ho x Ho map: fixed by the map size alone
static inline int rg_tiles(int Ho) { return (Ho * Ho + RG_PIX_TILE - 1) / RG_PIX_TILE; }
// input tiles per output tile in the packed 16-bit weight
__host__ __device__ static inline int rg_nkt(int gw) { return gw == 24 ? 3 : 1; }
// the window of output tile ct: first input tile and their number (<= rg_nkt(gw))
__host__ __device__ static inline void rg_window(int gw, int C, int ct, int* kt0, int* nkt) {
  const int o0 = ct * RG_CH_TILE;
  const int lo = o0 / gw * gw;
  int hi = ((o0 + RG_CH_TILE - 1) / gw + 1) * gw;
  if (hi > C) hi = C;
  *kt0 = lo / 16;
  *nkt = (hi + 15) / 16 - lo / 16;
}
// bytes of the packed grouped weight: fp32 [9][C][gw]; 16-bit [ceil(C/16)][9][rg_nkt][16][16]
static inline size_t rg_gconv_bytes(int prec, int C, int gw) {
  if (prec == PREC_FP32) return (size_t)9 * C * gw * 4;
  return (size_t)((C + 15) / 16) * 9 * rg_nkt(gw) * 256 * 2;
}

// stem: x [B,3,S,S] fp32 NCHW -> out [B,S/2,S/2,32] = ReLU(conv3x3/2 pad 1 (x; w [27][32] tap-major, BN folded) + b)
int rg_stem(const float* x, int B, int S, const float* w, const float* b, float* out, hipStream_t s);

// grouped 3x3, pad 1, stride 1 or 2, + folded BN + ReLU: in [B,H,H,C] -> out [B,Ho,Ho,C], Ho = (H - 1) / stride + 1; gw 8, 16 or 24,
// C % gw == 0; w packed as above.  part != NULL: also part [B][rg_tiles(Ho)][C], the sum of the stored output over each run of 64
// pixels, pixels ascending.
int rg_gconv(int prec, const float* in, int B, int H, int C, int stride, int gw, const void* w, const float* bias, float* out, int Ho,
             float* part, hipStream_t s);

// squeeze-excite gate from the tile sums: mean[c] = (sum of part[b][t][c] over t ascending) / HW -> hid = ReLU(w1 mean + b1) [R] ->
// gate [B,C] = sigmoid(w2t^T hid + b2).  w1 [R][C], w2t [R][C] (fc2 TRANSPOSED) fp32.  One workgroup per crop.
int rg_se_gate(const float* part, int B, int NT, int HW, int C, int R, const float* w1, const float* b1, const float* w2t, const float* b2,
               float* gate, hipStream_t s);

// rows of the strided shortcut: in [B,H,H,C] -> out [B,Ho,Ho,C] = in at the even rows and columns, Ho = (H - 1) / 2 + 1; C % 4 == 0
int rg_gather2(const float* in, int B, int H, int C, float* out, hipStream_t s);

// x[i] = max(x[i], 0) in place (NaN stays NaN); n % 4 == 0
int rg_relu(float* x, int64_t n, hipStream_t s);

}  // namespace effocr
