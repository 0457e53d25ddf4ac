// Internal launcher interface of libeffocr_effnet.so (effnet.hip -> effnet_api.hip): the EfficientNet-B0 kernels that mnv3g.hip does not
// have.  Activations are fp32 channels-last [crop][pixel][C] in HBM between launches, as in mnv3g.hpp, whose mg_pw / mg_pool / mg_finish
// the forward also uses.  Every launcher enqueues ONE kernel on the stream and returns an EFFOCR_* code; every kernel computes a crop's
// values from that crop's data alone, in an order fixed by the shapes: no float atomics, one kernel form for every call size.
#pragma once
#include "common.hpp"
#include "kernels.hpp"

namespace effocr {

constexpr int EF_STEM_C = 32;          // stem channels of EfficientNet-B0
constexpr int EF_TILE = 16;            // the depthwise kernel's output tile is EF_TILE x EF_TILE pixels (edge tiles are partial)
constexpr int EF_SE_MAXC = 1152, EF_SE_MAXR = 48;   // the widest squeeze-excite of B0 (the gate kernel's LDS tables)

// tiles of an Ho x Ho map: fixed by the map size alone
static inline int ef_tiles(int Ho) { const int n = (Ho + EF_TILE - 1) / EF_TILE; return n * n; }

// stem: x [B,3,S,S] fp32 NCHW -> out [B,S/2,S/2,32] = SiLU(conv3x3/2 (x; w [27][32] tap-major, BN folded) + b); the input pixel of tap
// (ky, kx) is (2 oy + ky - padb, 2 ox + kx - padb): padb 1 = symmetric padding, 0 = TensorFlow SAME on an even map (0 before, 1 after)
int ef_stem(const float* x, int B, int S, int padb, const float* w, const float* b, float* out, hipStream_t s);

// depthwise k x k (3 or 5), stride 1 or 2, + folded BN + SiLU: in [B,H,H,C] -> out [B,Ho,Ho,C]; tap (ky, kx) reads input pixel
// (oy stride + ky - padb, ...), so padb = k/2 is symmetric padding and padb = k/2 - 1 TensorFlow SAME at stride 2 on an even map; any tap
// outside the map is skipped (k = 5 on 2x2 and 1x1 maps).  w [k*k][C] tap-major fp32; C % 4 == 0.
// Also writes part [B][ef_tiles(Ho)][C]: the sum of the OUTPUT over each 16 x 16 tile (tile index ty * ntx + tx), per channel, summed in a
// fixed order.
int ef_dw(const float* in, int B, int H, int C, int k, int stride, int padb, const float* w, const float* b, float* out, int Ho, float* part,
          hipStream_t s);

// squeeze-excite gate from the tile sums: mean[c] = (sum of part[b][t][c] over t ascending) / HW -> hid = SiLU(wr mean + br) [R] ->
// gate [B,C] = sigmoid(wet^T hid + be).  wr [R][C], wet [R][C] (conv_expand TRANSPOSED) fp32.  One workgroup per crop, no pixel is read:
// the reduce FC is spread over the waves (one hidden unit per wave at a time), the expand FC over the threads (one channel each).
int ef_se_gate(const float* part, int B, int NT, int HW, int C, int R, const float* wr, const float* br, const float* wet, const float* be,
               float* gate, hipStream_t s);

}  // namespace effocr
