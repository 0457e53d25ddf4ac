// MobileNetV3-Small encoder kernels on gfx950 (timm mobilenetv3_small_050 semantics; api.hip: mnv3_forward).
//
// Four launches per sub-batch (DESIGN.md "MobileNetV3-Small"):
//   mnv3_stem_ds  stem conv + blocks.0.0's depthwise conv per 8x8 tile of the S/4 map; the S/2 stem output lives in LDS only (its
//                 1-pixel halo is recomputed); writes the tile and its channel sums (SE squeeze partials).
//   mnv3_stage1   blocks.0.0's SE gate (partials summed in tile order) + conv_pw, blocks.1.0 and blocks.1.1 per 8x8 tile of the S/8
//                 map; the S/4 expansion of blocks.1.0 lives in LDS only (halos recomputed).
//   mnv3_tail     blocks.2.0 .. blocks.5.0 and the global average pool, one crop per workgroup, every activation in LDS.
//   mnv3_head     conv_head on the pooled vectors, 16 crops per workgroup, + bias, hard-swish, F.normalize, status.
// Activations in LDS are fp32, channels-last [pixel][C].  Pointwise convs are GEMMs over LDS (pw_lds): in the 16-bit modes
// v_mfma_f32_16x16x16 on the weights' 16-bit type, the fp32 activation split into a 16-bit high part and the 16-bit rounding of its
// remainder (two MFMAs per K step: only the weights carry the mode's rounding, not the ~24 activation hand-offs); an fp32 FMA
// chain in the fp32 mode.  Depthwise
// convs, the stem, SE, biases, activations and residual adds are fp32 FMAs.  Every sum runs in an order fixed by the shapes alone.
#include "common.hpp"
#include "kernels.hpp"

namespace effocr {
namespace {

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_HS = 2 };

// NaN-propagating maximum / minimum (IEEE 754-2019; v_maximum3_f32 / v_minimum3_f32), as torch's relu, hardswish and hardsigmoid: fmaxf and
// fminf return the operand that is not NaN, which turned a NaN crop into a finite embedding (DESIGN.md "NaN semantics")
__device__ __forceinline__ float max_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ float min_nan(float a, float b) { return __builtin_elementwise_minimum(a, b); }
__device__ __forceinline__ float hsig(float x) { return min_nan(max_nan(x + 3.0f, 0.0f), 6.0f) / 6.0f; }
__device__ __forceinline__ float act_f(float x, int a) {
  return a == ACT_RELU ? max_nan(x, 0.0f) : a == ACT_HS ? x * hsig(x) : x;
}

template <typename T> __device__ __forceinline__ const T* WP(const char* wb, uint32_t off) { return reinterpret_cast<const T*>(wb + off); }

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4e __attribute__((ext_vector_type(4)));

template <typename TW> struct Mfma16;
template <> struct Mfma16<_Float16> {
  typedef f16x4 V;
  static __device__ __forceinline__ void split(V& hi, V& lo, int j, float x) { const _Float16 h = (_Float16)x; hi[j] = h; lo[j] = (_Float16)(x - (float)h); }
  static __device__ __forceinline__ void setw(V& v, int j, _Float16 x) { v[j] = x; }
  static __device__ __forceinline__ f32x4e mma(V a, V b, f32x4e c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
};
template <> struct Mfma16<__bf16> {
  typedef s16x4 V;
  static __device__ __forceinline__ void split(V& hi, V& lo, int j, float x) {
    const __bf16 h = (__bf16)x;
    hi[j] = __builtin_bit_cast(short, h); lo[j] = __builtin_bit_cast(short, (__bf16)(x - (float)h));
  }
  static __device__ __forceinline__ void setw(V& v, int j, __bf16 x) { v[j] = __builtin_bit_cast(short, x); }
  static __device__ __forceinline__ f32x4e mma(V a, V b, f32x4e c) { return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0); }
};

// Pointwise conv as a GEMM over LDS, whole workgroup (blockDim.x a multiple of 64):
//   epi(p, n, sum_k (in[p * ldi + k] * (kscale ? kscale[k] : 1)) * W[n * K + k])   for p < P, n < N.
// 16-bit TW: 16x16 output tiles dealt round-robin over the waves, K in steps of 16 (zero-padded), the activation as hi + lo parts
// (Mfma16::split); lane l holds rows 4 (l / 16) + i,
// column l % 16 of its tile (the 16x16x16 MFMA layout).  fp32: one output per thread at a time, k in order.  Ends with a barrier.
template <typename TW, class Epi>
__device__ __forceinline__ void pw_lds(const float* in, int ldi, int P, int K, const TW* __restrict__ W, int N, const float* kscale, Epi epi) {
  if constexpr (sizeof(TW) == 4) {
    for (int idx = threadIdx.x; idx < P * N; idx += blockDim.x) {
      const int p = idx / N, n = idx - p * N;
      const float* a = in + p * ldi;
      const float* w = W + (size_t)n * K;
      float acc = 0.f;
      if (kscale) for (int k = 0; k < K; ++k) acc = fmaf(a[k] * kscale[k], w[k], acc);
      else for (int k = 0; k < K; ++k) acc = fmaf(a[k], w[k], acc);
      epi(p, n, acc);
    }
  } else {
    typedef Mfma16<TW> M;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int mt = (P + 15) >> 4, nt = (N + 15) >> 4;
    const int r16 = lane & 15, kq = 4 * (lane >> 4);
    for (int t = wave; t < mt * nt; t += nw) {
      const int tm = t / nt, tn = t - tm * nt;
      const int row = tm * 16 + r16, col = tn * 16 + r16;
      f32x4e acc = {0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < K; k0 += 16) {
        typename M::V a, al, b;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = k0 + kq + j;
          float av = 0.f;
          if (row < P && k < K) { av = in[row * ldi + k]; if (kscale) av *= kscale[k]; }
          M::split(a, al, j, av);
          M::setw(b, j, (col < N && k < K) ? W[(size_t)col * K + k] : (TW)0.f);
        }
        acc = M::mma(al, b, M::mma(a, b, acc));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = tm * 16 + kq + i;
        if (p < P && col < N) epi(p, col, acc[i]);
      }
    }
  }
  __syncthreads();
}

// Depthwise k x k conv over LDS: out[(oy * Wo + ox) * ldo + c] = act(b[c] + sum_{ky, kx} in[(iy * Wi + ix) * ldi + c] w[(ky k + kx) C + c])
// with iy = oy s + ky - pad (taps outside [0, Hi) x [0, Wi) are zero).  Taps summed in (ky, kx) order.  Ends with a barrier.
__device__ __forceinline__ void dw_lds(const float* in, int ldi, int Hi, int Wi, int C, const float* __restrict__ w, const float* __restrict__ b,
                                       int k, int s, int pad, int act, float* out, int ldo, int Ho, int Wo) {
  for (int idx = threadIdx.x; idx < Ho * Wo * C; idx += blockDim.x) {
    const int px = idx / C, c = idx - px * C;
    const int oy = px / Wo, ox = px - oy * Wo;
    float acc = b[c];
    for (int ky = 0; ky < k; ++ky) {
      const int iy = oy * s + ky - pad;
      if (iy < 0 || iy >= Hi) continue;
      for (int kx = 0; kx < k; ++kx) {
        const int ix = ox * s + kx - pad;
        if (ix < 0 || ix >= Wi) continue;
        acc = fmaf(in[(iy * Wi + ix) * ldi + c], w[(ky * k + kx) * C + c], acc);
      }
    }
    out[px * ldo + c] = act_f(acc, act);
  }
  __syncthreads();
}

// Squeeze-excite gate from the channel means m[C] (LDS): h = ReLU(Wr m + br), gate = hardsigmoid(We h + be) -> gate[C] (LDS).
__device__ __forceinline__ void se_gate(const float* m, int C, int R, const char* wb, const MnvBlock& bk, float* h, float* gate) {
  const float* wr = WP<float>(wb, bk.ser.w); const float* br = WP<float>(wb, bk.ser.b);
  const float* we = WP<float>(wb, bk.see.w); const float* be = WP<float>(wb, bk.see.b);
  for (int j = threadIdx.x; j < R; j += blockDim.x) {
    float a = br[j];
    for (int c = 0; c < C; ++c) a = fmaf(wr[j * C + c], m[c], a);
    h[j] = max_nan(a, 0.f);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float a = be[c];
    for (int j = 0; j < R; ++j) a = fmaf(we[c * R + j], h[j], a);
    gate[c] = hsig(a);
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------------------
// stem + blocks.0.0 depthwise.  Tile = 8 x 8 outputs of the S/4 map -> 17 x 17 stem outputs (S/2 map, zero outside it) -> 35 x 35
// image pixels.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int SR = 2 * MNV_T1 + 1, IR = 2 * SR + 1;
__global__ __launch_bounds__(256) void mnv3_stem_ds_kernel(const float* __restrict__ img, const char* __restrict__ wb, MnvNet net,
                                                            float* __restrict__ t0, float* __restrict__ part) {
  __shared__ float im[3][IR][IR];
  __shared__ float st[SR * SR * 16];
  __shared__ float o[MNV_T1 * MNV_T1 * 16];
  const int S = net.S, S2 = S / 2, S4 = S / 4, nt = (S4 + MNV_T1 - 1) / MNV_T1;
  const int64_t b = blockIdx.x / (nt * nt);
  const int tile = blockIdx.x - (int)b * nt * nt, ty = tile / nt, tx = tile - ty * nt;
  const int oy0 = ty * MNV_T1, ox0 = tx * MNV_T1;
  const int sy0 = 2 * oy0 - 1, sx0 = 2 * ox0 - 1;       // stem-map origin of the region
  const int iy0 = 2 * sy0 - 1, ix0 = 2 * sx0 - 1;       // image origin
  const float* ib = img + b * 3 * (int64_t)S * S;
  for (int i = threadIdx.x; i < 3 * IR * IR; i += blockDim.x) {
    const int c = i / (IR * IR), r = (i / IR) % IR, q = i % IR;
    const int y = iy0 + r, x = ix0 + q;
    im[c][r][q] = (y >= 0 && y < S && x >= 0 && x < S) ? ib[((int64_t)c * S + y) * S + x] : 0.f;
  }
  __syncthreads();
  const float* ws = WP<float>(wb, net.stem.w);          // [16][27] (c, ky, kx)
  const float* bs = WP<float>(wb, net.stem.b);
  for (int i = threadIdx.x; i < SR * SR * 16; i += blockDim.x) {
    const int px = i >> 4, c = i & 15, r = px / SR, q = px - r * SR;
    const int y = sy0 + r, x = sx0 + q;
    float v = 0.f;
    if (y >= 0 && y < S2 && x >= 0 && x < S2) {
      float a = bs[c];
      for (int ci = 0; ci < 3; ++ci)
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx) a = fmaf(im[ci][2 * r + ky][2 * q + kx], ws[c * 27 + ci * 9 + ky * 3 + kx], a);
      v = act_f(a, ACT_HS);
    }
    st[i] = v;
  }
  __syncthreads();
  const MnvBlock& bk = net.blk[0];
  dw_lds(st, 16, SR, SR, 16, WP<float>(wb, bk.dw.w), WP<float>(wb, bk.dw.b), 3, 2, 0, ACT_RELU, o, 16, MNV_T1, MNV_T1);
  for (int i = threadIdx.x; i < MNV_T1 * MNV_T1 * 16; i += blockDim.x) {
    const int px = i >> 4, c = i & 15, r = px / MNV_T1, q = px - r * MNV_T1;
    t0[((b * S4 + oy0 + r) * S4 + ox0 + q) * 16 + c] = o[i];
  }
  if (threadIdx.x < 16) {
    float a = 0.f;
    for (int px = 0; px < MNV_T1 * MNV_T1; ++px) a += o[px * 16 + threadIdx.x];
    part[(b * nt * nt + tile) * 16 + threadIdx.x] = a;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// blocks.0.0 SE + conv_pw, blocks.1.0, blocks.1.1 per 8 x 8 tile of the S/8 map.  Regions (edge): block 1.1 output 8, block 1.0
// output 10 (1-pixel halo), S/4 input 21.  Expansions outside the map are zeroed (they are the depthwise convs' zero padding).
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int R10 = MNV_T2 + 2, R21 = 2 * R10 + 1;
constexpr int S1_R0 = R21 * R21 * 16, S1_R1 = R21 * R21 * 8, S1_R2 = R21 * R21 * 40;
template <typename TW>
__global__ __launch_bounds__(256) void mnv3_stage1_kernel(const float* __restrict__ t0, const float* __restrict__ part,
                                                           const char* __restrict__ wb, MnvNet net, float* __restrict__ t1) {
  __shared__ float r0[S1_R0];
  __shared__ float r1[S1_R1];
  __shared__ float r2[S1_R2];
  __shared__ float sm[16], sh[8], sg[16];
  const int S = net.S, S4 = S / 4, S8 = S / 8, nt = (S8 + MNV_T2 - 1) / MNV_T2, nt1 = mnv3_tiles1(S);
  const int64_t b = blockIdx.x / (nt * nt);
  const int tile = blockIdx.x - (int)b * nt * nt, ty = tile / nt, tx = tile - ty * nt;
  const int Y0 = ty * MNV_T2, X0 = tx * MNV_T2;
  const int ay0 = 2 * (Y0 - 1) - 1, ax0 = 2 * (X0 - 1) - 1;   // S/4-map origin of the 21 x 21 region
  const MnvBlock& b0 = net.blk[0];
  const MnvBlock& b1 = net.blk[1];
  const MnvBlock& b2 = net.blk[2];
  // SE squeeze of blocks.0.0: the tiles' channel sums in tile order
  if (threadIdx.x < 16) {
    float a = 0.f;
    for (int t = 0; t < nt1; ++t) a += part[(b * nt1 + t) * 16 + threadIdx.x];
    sm[threadIdx.x] = a / (float)(S4 * S4);
  }
  __syncthreads();
  se_gate(sm, 16, b0.se, wb, b0, sh, sg);
  for (int i = threadIdx.x; i < R21 * R21 * 16; i += blockDim.x) {
    const int px = i >> 4, c = i & 15, r = px / R21, q = px - r * R21;
    const int y = ay0 + r, x = ax0 + q;
    r0[i] = (y >= 0 && y < S4 && x >= 0 && x < S4) ? t0[((b * S4 + y) * S4 + x) * 16 + c] : 0.f;
  }
  __syncthreads();
  auto in4 = [&](int p) { const int r = p / R21, q = p - r * R21, y = ay0 + r, x = ax0 + q; return y >= 0 && y < S4 && x >= 0 && x < S4; };
  auto in8 = [&](int p) { const int r = p / R10, q = p - r * R10, y = Y0 - 1 + r, x = X0 - 1 + q; return y >= 0 && y < S8 && x >= 0 && x < S8; };
  // blocks.0.0 conv_pw (+ bn2, no activation) on the gated depthwise output
  {
    const float* bb = WP<float>(wb, b0.pwl.b);
    pw_lds<TW>(r0, 16, R21 * R21, 16, WP<TW>(wb, b0.pwl.w), 8, sg, [&](int p, int n, float a) { r1[p * 8 + n] = a + bb[n]; });
  }
  // blocks.1.0: conv_pw + ReLU (zero outside the map), depthwise 3x3/s2 + ReLU, conv_pwl
  {
    const float* bb = WP<float>(wb, b1.pw.b);
    pw_lds<TW>(r1, 8, R21 * R21, 8, WP<TW>(wb, b1.pw.w), 40, nullptr,
               [&](int p, int n, float a) { r2[p * 40 + n] = in4(p) ? max_nan(a + bb[n], 0.f) : 0.f; });
  }
  dw_lds(r2, 40, R21, R21, 40, WP<float>(wb, b1.dw.w), WP<float>(wb, b1.dw.b), 3, 2, 0, ACT_RELU, r0, 40, R10, R10);
  {
    const float* bb = WP<float>(wb, b1.pwl.b);
    pw_lds<TW>(r0, 40, R10 * R10, 40, WP<TW>(wb, b1.pwl.w), 16, nullptr, [&](int p, int n, float a) { r1[p * 16 + n] = a + bb[n]; });
  }
  // blocks.1.1: conv_pw + ReLU (zero outside the map), depthwise 3x3/s1 + ReLU, conv_pwl + residual
  {
    const float* bb = WP<float>(wb, b2.pw.b);
    pw_lds<TW>(r1, 16, R10 * R10, 16, WP<TW>(wb, b2.pw.w), 56, nullptr,
               [&](int p, int n, float a) { r2[p * 56 + n] = in8(p) ? max_nan(a + bb[n], 0.f) : 0.f; });
  }
  dw_lds(r2, 56, R10, R10, 56, WP<float>(wb, b2.dw.w), WP<float>(wb, b2.dw.b), 3, 1, 0, ACT_RELU, r0, 56, MNV_T2, MNV_T2);
  {
    const float* bb = WP<float>(wb, b2.pwl.b);
    pw_lds<TW>(r0, 56, MNV_T2 * MNV_T2, 56, WP<TW>(wb, b2.pwl.w), 16, nullptr, [&](int p, int n, float a) {
      const int r = p / MNV_T2, q = p - r * MNV_T2, y = Y0 + r, x = X0 + q;
      if (y < S8 && x < S8) t1[((b * S8 + y) * S8 + x) * 16 + n] = a + bb[n] + r1[((r + 1) * R10 + q + 1) * 16 + n];
    });
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// blocks.2.0 .. blocks.5.0 + pool, one crop per workgroup.  Arena per block: X (block input, also the residual) at 0, the depthwise
// output D after it, and one channel group of cg expansion channels E (full map) after D; the block output overwrites X.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename TW>
__global__ __launch_bounds__(256) void mnv3_tail_kernel(const float* __restrict__ t1, const char* __restrict__ wb, MnvNet net,
                                                         float* __restrict__ pooled) {
  __shared__ float ar[MNV_TAIL_LDS_FLOATS];
  __shared__ float sm[288], sh[72], sg[288];
  const int64_t b = blockIdx.x;
  int H = net.S / 8;
  const float* src = t1 + b * (int64_t)H * H * 16;
  for (int i = threadIdx.x; i < H * H * 16; i += blockDim.x) ar[i] = src[i];
  __syncthreads();
  for (int bi = 3; bi < MNV_NBLK; ++bi) {
    const MnvBlock& bk = net.blk[bi];
    const int Ho = (H - 1) / bk.stride + 1, HWi = H * H, HWo = Ho * Ho;
    const int act = bk.hs ? ACT_HS : ACT_RELU;
    float* X = ar;
    float* D = ar + HWi * bk.cin;
    float* E = D + HWo * bk.mid;
    const float* pwb = WP<float>(wb, bk.pw.b);
    const float* dww = WP<float>(wb, bk.dw.w);
    const float* dwb = WP<float>(wb, bk.dw.b);
    for (int g0 = 0; g0 < bk.mid; g0 += bk.cg) {
      const int cg = bk.cg;
      pw_lds<TW>(X, bk.cin, HWi, bk.cin, WP<TW>(wb, bk.pw.w) + (size_t)g0 * bk.cin, cg, nullptr,
                 [&](int p, int n, float a) { E[p * cg + n] = act_f(a + pwb[g0 + n], act); });
      // depthwise over the group: weights [k*k][mid] read at column g0 (dw_lds indexes w[tap * C + c] with C = cg, so step by hand)
      for (int idx = threadIdx.x; idx < HWo * cg; idx += blockDim.x) {
        const int px = idx / cg, c = idx - px * cg;
        const int oy = px / Ho, ox = px - oy * Ho, k = bk.k, pad = k / 2;
        float acc = dwb[g0 + c];
        for (int ky = 0; ky < k; ++ky) {
          const int iy = oy * bk.stride + ky - pad;
          if (iy < 0 || iy >= H) continue;
          for (int kx = 0; kx < k; ++kx) {
            const int ix = ox * bk.stride + kx - pad;
            if (ix < 0 || ix >= H) continue;
            acc = fmaf(E[(iy * H + ix) * cg + c], dww[(ky * k + kx) * bk.mid + g0 + c], acc);
          }
        }
        D[px * bk.mid + g0 + c] = act_f(acc, act);
      }
      __syncthreads();
    }
    // squeeze (pixel order) + excite
    for (int c = threadIdx.x; c < bk.mid; c += blockDim.x) {
      float a = 0.f;
      for (int p = 0; p < HWo; ++p) a += D[p * bk.mid + c];
      sm[c] = a / (float)HWo;
    }
    __syncthreads();
    se_gate(sm, bk.mid, bk.se, wb, bk, sh, sg);
    const float* lb = WP<float>(wb, bk.pwl.b);
    const int res = bk.res, co = bk.cout;
    pw_lds<TW>(D, bk.mid, HWo, bk.mid, WP<TW>(wb, bk.pwl.w), co, sg, [&](int p, int n, float a) {
      const float v = a + lb[n];
      X[p * co + n] = res ? v + X[p * co + n] : v;
    });
    H = Ho;
  }
  // blocks.5.0: 1x1 conv + BN + hard-swish, then the global average pool in pixel order
  const int HW = H * H, cin = net.blk[MNV_NBLK - 1].cout, cc = net.cn_c;
  float* Y = ar + HW * cin;
  const float* cb = WP<float>(wb, net.cn.b);
  pw_lds<TW>(ar, cin, HW, cin, WP<TW>(wb, net.cn.w), cc, nullptr, [&](int p, int n, float a) { Y[p * cc + n] = act_f(a + cb[n], ACT_HS); });
  for (int c = threadIdx.x; c < cc; c += blockDim.x) {
    float a = 0.f;
    for (int p = 0; p < HW; ++p) a += Y[p * cc + c];
    pooled[b * cc + c] = a / (float)HW;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// conv_head: emb[m][n] = hswish(bias[n] + sum_k pooled[m][k] W[n][k]), 16 crops per workgroup of 4 waves, a wave owns nf / 4 columns
// (16x16 tiles).  F.normalize: squares summed per lane over its tiles, across the 16 lanes of a row (xor butterfly), then over the
// waves in wave order.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename TW>
__global__ __launch_bounds__(256) void mnv3_head_kernel(const float* __restrict__ pooled, int B, const char* __restrict__ wb, MnvNet net,
                                                         int l2norm, float* __restrict__ emb, int* __restrict__ status) {
  constexpr int NT = 16;                                 // tiles per wave (nf = 1024)
  __shared__ float ss[4][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, kq = 4 * (lane >> 4);
  const int K = net.cn_c, N = net.nf;
  const int64_t m0 = (int64_t)blockIdx.x * 16;
  const TW* W = WP<TW>(wb, net.head.w);
  const float* bias = WP<float>(wb, net.head.b);
  f32x4e acc[NT];
  const int64_t arow = m0 + r16;
  for (int t = 0; t < NT; ++t) {
    const int col = (wave * NT + t) * 16 + r16;
    acc[t] = f32x4e{0.f, 0.f, 0.f, 0.f};
    if constexpr (sizeof(TW) == 4) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = m0 + kq + i;
        float a = 0.f;
        if (row < B) for (int k = 0; k < K; ++k) a = fmaf(pooled[row * K + k], W[(size_t)col * K + k], a);
        acc[t][i] = a;
      }
    } else {
      typedef Mfma16<TW> M;
      for (int k0 = 0; k0 < K; k0 += 16) {
        typename M::V a, al, bv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = k0 + kq + j;
          M::split(a, al, j, (arow < B && k < K) ? pooled[arow * K + k] : 0.f);
          M::setw(bv, j, k < K ? W[(size_t)col * K + k] : (TW)0.f);
        }
        acc[t] = M::mma(al, bv, M::mma(a, bv, acc[t]));
      }
    }
  }
  float sq[4] = {0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < NT; ++t) {
    const int col = (wave * NT + t) * 16 + r16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = act_f(acc[t][i] + bias[col], ACT_HS);
      acc[t][i] = v;
      sq[i] = fmaf(v, v, sq[i]);
    }
  }
  if (l2norm) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      for (int o = 1; o < 16; o <<= 1) sq[i] += __shfl_xor(sq[i], o, 64);
    if (r16 == 0)
      for (int i = 0; i < 4; ++i) ss[wave][kq + i] = sq[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float n2 = (ss[0][kq + i] + ss[1][kq + i]) + (ss[2][kq + i] + ss[3][kq + i]);
      const float nr = sqrtf(n2);
      sq[i] = nr < 1e-12f ? 1e-12f : nr;                 // F.normalize: x / max(||x||, eps); a NaN norm stays NaN, as torch's clamp_min
    }
  }
  bool bad = false;
  for (int t = 0; t < NT; ++t) {
    const int col = (wave * NT + t) * 16 + r16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = m0 + kq + i;
      if (row >= B) continue;
      const float v = l2norm ? acc[t][i] / sq[i] : acc[t][i];
      bad |= !(fabsf(v) <= 3.0e38f);
      emb[row * N + col] = v;
    }
  }
  if (status && bad) atomicOr(status, 1);
}

#define MNV_LAUNCH_PREC(K, prec, grid, s, name, ...)                                                                  \
  do {                                                                                                                 \
    switch (prec) {                                                                                                    \
      case PREC_BF16: hipLaunchKernelGGL(K<__bf16>, grid, dim3(256), 0, s, __VA_ARGS__); break;                        \
      case PREC_FP16: hipLaunchKernelGGL(K<_Float16>, grid, dim3(256), 0, s, __VA_ARGS__); break;                      \
      case PREC_FP32: hipLaunchKernelGGL(K<float>, grid, dim3(256), 0, s, __VA_ARGS__); break;                         \
      default: return fail(EFFOCR_EINVAL, std::string(name) + ": unknown precision");                                 \
    }                                                                                                                  \
    return check_launch(name);                                                                                         \
  } while (0)

bool shape_ok(const MnvNet& net) { return net.S >= 32 && net.S <= 224 && net.S % 32 == 0 && net.stem_c == 16 && net.nf == 16 * 4 * 16; }

}  // namespace

int mnv3_stem_ds(int prec, const float* img, int B, const char* wb, const MnvNet& net, float* t0, float* part, hipStream_t s) {
  (void)prec;
  if (B <= 0) return EFFOCR_OK;
  if (!shape_ok(net)) return fail(EFFOCR_EUNSUPPORTED, "mnv3_stem_ds: unsupported shape");
  hipLaunchKernelGGL(mnv3_stem_ds_kernel, dim3((unsigned)(B * mnv3_tiles1(net.S))), dim3(256), 0, s, img, wb, net, t0, part);
  return check_launch("mnv3_stem_ds");
}

int mnv3_stage1(int prec, const float* t0, const float* part, int B, const char* wb, const MnvNet& net, float* t1, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (!shape_ok(net)) return fail(EFFOCR_EUNSUPPORTED, "mnv3_stage1: unsupported shape");
  MNV_LAUNCH_PREC(mnv3_stage1_kernel, prec, dim3((unsigned)(B * mnv3_tiles2(net.S))), s, "mnv3_stage1", t0, part, wb, net, t1);
}

int mnv3_tail(int prec, const float* t1, int B, const char* wb, const MnvNet& net, float* pooled, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (!shape_ok(net) || net.cn_c > 288) return fail(EFFOCR_EUNSUPPORTED, "mnv3_tail: unsupported shape");
  MNV_LAUNCH_PREC(mnv3_tail_kernel, prec, dim3((unsigned)B), s, "mnv3_tail", t1, wb, net, pooled);
}

int mnv3_head(int prec, const float* pooled, int B, const char* wb, const MnvNet& net, int l2norm, float* emb, int* status, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (!shape_ok(net)) return fail(EFFOCR_EUNSUPPORTED, "mnv3_head: unsupported shape");
  MNV_LAUNCH_PREC(mnv3_head_kernel, prec, dim3((unsigned)((B + 15) / 16)), s, "mnv3_head", pooled, B, wb, net, l2norm, emb, status);
}

}  // namespace effocr
