// Internal launcher interface of libeffocr_pvt.so (pvt.hip -> pvt_api.hip).  Every kernel computes a crop's rows from that crop's inputs
// alone, in an order fixed by the shape: embeddings do not depend on the call size, the crop's position or the chunking.  No float atomics.
#pragma once
#include "common.hpp"

namespace effocr {

constexpr int PVT_MAX_KEYS = 49;                         // reduced keys per crop: (img / 32)^2 with img <= 224
constexpr int PVT_QBLK = 32;                             // query tile of pvt_attention: queries per wave pass (one 32-wide MFMA block)
constexpr int PVT_QCHUNK = 512;                          // queries per workgroup (4 waves x 4 passes); K and V are staged once per workgroup
constexpr int PVT_STEM_K = 160;                          // 3 * 7 * 7 = 147 taps of the stem, zero padded to a multiple of 16
constexpr int PVT_MAX_WIDTH = 512;                       // widest LayerNorm row (one wave per row, 8 columns per lane)

// PVTv2 attention over spatially reduced keys:  out = softmax(q k^T / sqrt(hd)) v  per (crop, head).
//   q   [B * N][heads * hd]      head h's queries at feature h * hd
//   kv  [B * M][2 * heads * hd]  head h's keys at h * hd, its values at heads * hd + h * hd;  1 <= M <= PVT_MAX_KEYS
//   out [B * N][heads * hd]      all three in prec's type; hd is 32 or 64
// 16-bit modes: one workgroup (4 waves) per (crop, head, PVT_QCHUNK queries).  K rows and V^T are staged in LDS once, padded with ZEROS to
// a multiple of 32 key slots — a slot at or beyond M is never read from memory — and every wave streams PVT_QBLK queries at a time through
// them: S^T = K Q^T on v_mfma_f32_32x32x16, the slots at or beyond M set to -inf (weight exactly 0), one maximum and one sum over all keys
// (no running rescale: at most two key tiles live in registers), O^T = V^T P^T on the same MFMA.
// Rounding points of the 16-bit modes (tests/pvt_ref.py: attention_emulated restates exactly these):
//   - q, k, v arrive in the operand type; q . k, the scaled score s = (q . k) * hd^-1/2, the maximum m, p = exp(s - m), the sum l of the
//     UNROUNDED p and the O accumulator are fp32;
//   - p is rounded to the operand type for the P V MFMA;
//   - O / l is rounded once to the operand type on the store.
// fp32 mode: K and V staged in LDS as fp32, one thread per (query, 32 values), two passes over the keys (maximum, then exp and sum) in plain
// fp32 arithmetic.
int pvt_attention(int prec, const void* q, const void* kv, int B, int N, int M, int heads, int hd, void* out, hipStream_t s);

// Depthwise 3x3 (stride 1, zero pad 1) + bias + exact (erf) GELU on token rows: in / out [B][H * W][C] in prec's type, channels last.
//   w [9][C] fp32, row ky * 3 + kx, values already rounded to prec's type; bias [C] fp32; C % 4 == 0
// fp32 products and sums (taps in ascending order, out-of-image taps skipped, bias last), GELU in fp32, one rounding on the store.  A tap
// outside the H x W grid of its own crop is never read.
int pvt_dwconv_gelu(int prec, const void* in, int B, int H, int W, int C, const float* w, const float* bias, void* out, hipStream_t s);

// Where the rows of a GEMM's activation operand come from.
enum { PVT_A_DENSE = 0,   // X [rows][K] in prec's type
       PVT_A_CONV = 1,    // implicit im2col of token rows [B][H * H][Cin] in prec's type: row (b, oy, ox), k = (ky * ksize + kx) * Cin + c reads
                          // token (oy * stride - pad + ky, ox * stride - pad + kx), zero outside the grid; Cin % 8 == 0.  3x3/2 pad 1: the
                          // down-sampling patch embedding; ksize = stride = sr, pad 0: the spatial reduction's non-overlapping gather
       PVT_A_STEM = 2 };  // the 7x7/4 pad-3 stem on fp32 NCHW crops [B][3][H][H]: k = (c * 7 + ky) * 7 + kx < 147 (zero up to PVT_STEM_K), every
                          // pixel rounded to prec's type as it is read
enum { PVT_EPI_OP = 0,    // out [rows][N] in prec's type = acc + bias (one rounding)
       PVT_EPI_F32 = 1,   // out fp32 = acc + bias
       PVT_EPI_RESID = 2 };   // out fp32 = resid + (acc + bias); resid may be out itself
struct PvtGemm {
  int amode;
  const void* X;                    // DENSE: [rows][K]; CONV: token rows; STEM: the crops
  int B, H, Cin, ksize, stride, pad;   // CONV / STEM geometry (H: input side; output side OH = (H + 2 pad - ksize) / stride + 1)
  const void* W;                    // [N][K] in prec's type, k in the operand's order
  const float* bias;                // [N]
  void* out; const float* resid;
  int64_t rows; int N, K;           // N % 32 == 0, K % 16 == 0
};
// out [rows][N] = epilogue(A [rows][K] . W [N][K]^T + bias).  One wave per 32 rows x 32 (N % 64 != 0) or 64 columns; both operands go
// from memory to MFMA fragments, K is reduced in ascending order in fp32 (v_mfma_f32_32x32x16 in the 16-bit modes, v_mfma_f32_32x32x2f32 in
// the fp32 mode): a row's result depends on (prec, N, K) and that row's inputs alone.
int pvt_gemm(int prec, int epi, const PvtGemm& g, hipStream_t s);

// LayerNorm over the C <= PVT_MAX_WIDTH columns (C % 4 == 0) of fp32 rows, one wave per row: mean, then the variance of the centred values,
// both fp32 in a fixed shuffle order; out in prec's type (out_f32 = 0, one rounding) or fp32 (out_f32 = 1; out may be x itself).
int pvt_layernorm(int prec, const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps, void* out, int out_f32,
                  hipStream_t s);

// emb [B][D] = mean over the T tokens of x [B * T][D] (ascending token order, fp32), F.normalize'd when l2norm; ORs 1 into *status (may be
// NULL) on a non-finite embedding.  D <= 1024.
int pvt_pool(const float* x, int B, int T, int D, int l2norm, float* emb, int* status, hipStream_t s);

}  // namespace effocr
