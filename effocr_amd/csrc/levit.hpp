// Internal launcher interface of libeffocr_levit.so (levit.hip -> levit_api.hip).  Every kernel computes a crop's rows from that crop's
// inputs alone, in a fixed order: embeddings do not depend on the call size or the chunking.
#pragma once
#include "common.hpp"

namespace effocr {

constexpr int LEVIT_MAX_R = 14;                          // token grid per side at 224^2: at most 196 keys per crop-head
constexpr int LEVIT_KTILE = 32;                          // keys per tile of levit_attention, 16-bit modes (one 32x32 MFMA block)
constexpr int LEVIT_KTAIL = 4;                           // 196 = 6 * 32 + 4: the key tail of the 14 x 14 grid
constexpr int LEVIT_QBLK = 32;                           // queries per wave pass, 16-bit modes (4 waves per workgroup)
// Token grids per side the attention tests walk: Tk = R^2 = 1, 4, 9, 16, 36, 49, 64, 196 — below, at and above LEVIT_KTILE and
// LEVIT_KTAIL, and every grid a supported crop size produces (img / 16 and its two halvings).
constexpr int LEVIT_TEST_GRIDS[] = {1, 2, 3, 4, 6, 7, 8, 14};

// grid side after a stride-2 sub-sampling of the tokens at even rows and columns
__host__ __device__ static inline int levit_sub(int R) { return (R - 1) / 2 + 1; }

// Where q, k and v of head h live: row t of a buffer of `ld` elements, feature h * hs + off.
struct LevitQKV {
  const void* q; int64_t ldq; int qhs, qoff;             // queries [B * Tq] rows
  const void* kv; int64_t ldkv; int khs, koff, voff;     // keys and values [B * Tk] rows (may be the query buffer)
};

// LeViT attention:  out = act( softmax(q k^T * kd^-0.5 + bias[h][|dy| R + |dx|]) v ), kd in {16, 32}, value width vd in {32, 64, 128}.
//   keys: the R x R grid (Tk = R^2, 1 <= R <= LEVIT_MAX_R), key j at (j / R, j % R)
//   queries: stride 1: the same grid (Tq = Tk); stride 2: the Rq x Rq grid, Rq = levit_sub(R), query i at (2 (i / Rq), 2 (i % Rq))
//   bias [heads][R^2] fp32, looked up by the absolute row and column offset between the query's position and the key's
//   out [B * Tq][heads * vd] in prec's type (feature = h * vd + d); act: 0 = none, 1 = hardswish x relu6(x + 3) / 6 (on the fp32 value)
// 16-bit modes: one workgroup per (crop, head, 64-wide slice of the values); K rows and V^T of the crop-head are staged in LDS once, each
// wave takes 32 queries at a time and walks the key tiles in ascending order with a running maximum m and sum l (online softmax),
// rescaling on every tile:
//   s_j = fma(q . k_j, kd^-0.5, bias)   m' = max(m, max_j s_j)   alpha = exp(m - m')   p_j = exp(s_j - m')   l = alpha l + sum_j p_j
//   O = alpha O + P V
// Keys at or beyond Tk score -inf: weight exactly 0, and their K / V rows are staged as zeros.  Query slots at or beyond Tq repeat row
// Tq - 1 and are not stored.
// Rounding points of the 16-bit modes (tests/levit_ref.py: attention_emulated restates them):
//   - q, k, v arrive in the operand type; q . k, s, m, l, alpha and the O accumulator are fp32;
//   - p_j is rounded to the operand type for the P V MFMA; l sums the UNROUNDED fp32 p_j;
//   - act(O / l) is rounded once to the operand type on the store.
// fp32 mode: the same recurrence key by key in plain fp32 arithmetic, one thread per (query, 32 values).
int levit_attention(int prec, const LevitQKV& a, const float* bias, int B, int R, int stride, int heads, int kd, int vd, int act, void* out,
                    hipStream_t s);

// 3x3 stride-2 pad-1 convolution + bias (+ hardswish), BatchNorm folded into wt / bias on the host.
//   in: nchw = 1: [B][Cin][H][H] fp32 (the crops; each value is rounded to prec's type as it is read); nchw = 0: [B][H * H][Cin] in prec's type
//   wt [9 * Cin][Cout] fp32, row (ky * 3 + kx) * Cin + c — values already rounded to prec's type; bias [Cout] fp32
//   out [B][OH * OH][ldo], OH = (H - 1) / 2 + 1, in prec's type or — out_f32 — fp32 (the residual stream): channels 0 .. Cout
//   (Cout % 4 == 0), zeros in the columns Cout .. ldo (the K padding of the GEMM that reads the rows)
// Products and sums are fp32 (taps in ascending (ky, kx, c) order, bias added last); the result is rounded once on the store.
int levit_conv3x3s2(int prec, const void* in, int nchw, int B, int H, int Cin, const float* wt, const float* bias, int Cout, int act, void* out,
                    int ldo, int out_f32, hipStream_t s);

// rows of the fp32 residual stream -> the operand type: out [B * Tq][D] = x [B * R * R][D] at the tokens a stride-`stride` sub-sampling keeps
// (stride 1: every row)
int levit_cast_rows(int prec, const float* x, int B, int R, int stride, int D, void* out, hipStream_t s);
// buf [n] (prec's type) <- hardswish(buf), computed in fp32 from the stored value and rounded once
int levit_hardswish(int prec, void* buf, int64_t n, hipStream_t s);
// emb [B][D] = mean over the T tokens of x [B * T][ldx] (ascending token order, fp32), F.normalize'd when l2norm; ORs 1 into *status
// (may be NULL) on a non-finite embedding
int levit_pool(const float* x, int B, int T, int D, int ldx, int l2norm, float* emb, int* status, hipStream_t s);

}  // namespace effocr
