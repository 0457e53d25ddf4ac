// MobileNetV3 (Small 0.5 / 0.75 / 1.0, Large 1.0) forward kernels on gfx950 with the activations in HBM between blocks
// (libeffocr_mnv3.so; mnv3g_api.hip: mnv3_forward; DESIGN.md "MobileNetV3 family").
//
//   mg_stem     3x3/2 stem conv + folded BN + hard-swish, NCHW crops -> channels-last fp32, one output pixel (16 channels) per thread.
//   mg_pw       every 1x1 conv (expand, project, blocks.N.0 ConvBnAct, conv_head) as one GEMM form over pixel rows: 16-bit modes on
//               v_mfma_f32_16x16x16 with the weights as the A operand, so that a lane ends up with FOUR CONSECUTIVE output channels of one
//               pixel (16-byte bias / residual loads and stores); the fp32 activation enters as a 16-bit high part plus the 16-bit rounding
//               of its remainder (two MFMAs per K step), so only the weights carry the mode's rounding.  fp32 mode: one FMA chain per
//               output, k ascending.  Prologue: the squeeze-excite gate of the row's crop; epilogue: bias, activation, residual.
//   mg_dw       depthwise 3x3 / 5x5, stride 1 / 2, + folded BN + activation; four channels per thread, taps in (ky, kx) order.
//   mg_se_gate  one crop per workgroup: channel means in a fixed order, reduce FC + ReLU, expand FC + hard-sigmoid.
//   mg_pool     global average pool, pixels in order.
//   mg_finish   F.normalize in place and the non-finite check (an integer OR into the status word).
// A GEMM row's result depends on that row's K values alone and every reduction runs in an order fixed by the shapes: a crop's embedding is
// bitwise the same for every call size.
#include "mnv3g.hpp"

namespace effocr {
namespace {

// NaN-propagating maximum / minimum (IEEE 754-2019; v_maximum3_f32 / v_minimum3_f32), as torch's relu, hardswish and hardsigmoid: fmaxf and
// fminf return the operand that is not NaN, which turned a NaN crop into a finite embedding (DESIGN.md "NaN semantics")
__device__ __forceinline__ float mg_max(float a, float b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ float mg_min(float a, float b) { return __builtin_elementwise_minimum(a, b); }
__device__ __forceinline__ float mg_hsig(float x) { return mg_min(mg_max(x + 3.0f, 0.0f), 6.0f) / 6.0f; }
__device__ __forceinline__ float mg_act(float x, int a) {
  return a == MG_ACT_RELU ? mg_max(x, 0.0f) : a == MG_ACT_HS ? x * mg_hsig(x) : a == MG_ACT_SILU ? silu_fast(x) : x;
}

typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

template <typename TW> struct MgMma;
template <> struct MgMma<_Float16> {
  typedef h16x4 V;
  static __device__ __forceinline__ void split(V& hi, V& lo, int j, float x) { const _Float16 h = (_Float16)x; hi[j] = h; lo[j] = (_Float16)(x - (float)h); }
  static __device__ __forceinline__ f32x4v mma(V a, V b, f32x4v c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
};
template <> struct MgMma<__bf16> {
  typedef i16x4 V;
  static __device__ __forceinline__ void split(V& hi, V& lo, int j, float x) {
    const __bf16 h = (__bf16)x;
    hi[j] = __builtin_bit_cast(short, h); lo[j] = __builtin_bit_cast(short, (__bf16)(x - (float)h));
  }
  static __device__ __forceinline__ f32x4v mma(V a, V b, f32x4v c) { return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0); }
};

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mg_stem_kernel(const float* __restrict__ x, int64_t npix, int S, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= npix) return;
  const int S2 = S / 2;
  const int ox = (int)(idx % S2), oy = (int)((idx / S2) % S2);
  const int64_t b = idx / ((int64_t)S2 * S2);
  float acc[MG_STEM_C];
#pragma unroll
  for (int c = 0; c < MG_STEM_C; ++c) acc[c] = bias[c];
  for (int ci = 0; ci < 3; ++ci) {
    const float* xp = x + (b * 3 + ci) * (int64_t)S * S;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = 2 * oy + ky - 1;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = 2 * ox + kx - 1;
        if (iy < 0 || iy >= S || ix < 0 || ix >= S) continue;
        const float v = xp[(int64_t)iy * S + ix];
        const float* wt = w + ((ci * 3 + ky) * 3 + kx) * MG_STEM_C;
#pragma unroll
        for (int c = 0; c < MG_STEM_C; ++c) acc[c] = fmaf(v, wt[c], acc[c]);
      }
    }
  }
  float4* o = reinterpret_cast<float4*>(out + idx * MG_STEM_C);
#pragma unroll
  for (int c = 0; c < MG_STEM_C; c += 4)
    o[c / 4] = make_float4(mg_act(acc[c], MG_ACT_HS), mg_act(acc[c + 1], MG_ACT_HS), mg_act(acc[c + 2], MG_ACT_HS), mg_act(acc[c + 3], MG_ACT_HS));
}

// ---------------------------------------------------------------------------------------------------------------------------
template <int KS>
__global__ __launch_bounds__(256) void mg_dw_kernel(const float* __restrict__ in, int64_t total, int H, int C, int stride,
                                                     const float* __restrict__ w, const float* __restrict__ bias, int act,
                                                     float* __restrict__ out, int Ho) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (crop, oy, ox, channel quad), the quad fastest
  if (idx >= total) return;
  const int C4 = C / 4;
  const int c = (int)(idx % C4) * 4;
  const int64_t px = idx / C4;
  const int ox = (int)(px % Ho), oy = (int)((px / Ho) % Ho);
  const int64_t b = px / ((int64_t)Ho * Ho);
  constexpr int pad = KS / 2;
  const float* ip = in + b * (int64_t)H * H * C + c;
  float4 acc = *reinterpret_cast<const float4*>(bias + c);
#pragma unroll
  for (int ky = 0; ky < KS; ++ky) {
    const int iy = oy * stride + ky - pad;
    if (iy < 0 || iy >= H) continue;
#pragma unroll
    for (int kx = 0; kx < KS; ++kx) {
      const int ix = ox * stride + kx - pad;
      if (ix < 0 || ix >= H) continue;
      const float4 v = *reinterpret_cast<const float4*>(ip + ((int64_t)iy * H + ix) * C);
      const float4 wt = *reinterpret_cast<const float4*>(w + (ky * KS + kx) * C + c);
      acc.x = fmaf(v.x, wt.x, acc.x); acc.y = fmaf(v.y, wt.y, acc.y); acc.z = fmaf(v.z, wt.z, acc.z); acc.w = fmaf(v.w, wt.w, acc.w);
    }
  }
  *reinterpret_cast<float4*>(out + px * C + c) = make_float4(mg_act(acc.x, act), mg_act(acc.y, act), mg_act(acc.z, act), mg_act(acc.w, act));
}

// ---------------------------------------------------------------------------------------------------------------------------
constexpr int MG_SE_MAXC = 1024, MG_SE_MAXR = 256;

__device__ __forceinline__ float mg_wave_sum(float v) {           // xor butterfly: every lane ends with the same sum, same order every time
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void mg_se_gate_kernel(const float* __restrict__ t, int HW, int C, int R, const float* __restrict__ wr,
                                                          const float* __restrict__ br, const float* __restrict__ we,
                                                          const float* __restrict__ be, float* __restrict__ gate) {
  __shared__ float part[4 * MG_SE_MAXC];
  __shared__ float mean[MG_SE_MAXC];
  __shared__ float hid[MG_SE_MAXR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const float* tp = t + b * (int64_t)HW * C;
  // channel sums: G pixel groups (pixel p belongs to group p % G) of cw channel lanes; groups combined in order
  const int cw = C > 32 ? 64 : C > 16 ? 32 : 16, G = 256 / cw;
  const int g = tid / cw, l = tid % cw;
  for (int c = l; c < C; c += cw) {
    float s = 0.f;
    for (int p = g; p < HW; p += G) s += tp[(int64_t)p * C + c];
    part[g * C + c] = s;
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float s = 0.f;
    for (int i = 0; i < G; ++i) s += part[i * C + c];
    mean[c] = s / (float)HW;
  }
  __syncthreads();
  for (int j = wave; j < R; j += 4) {                    // one wave per hidden unit
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = fmaf(wr[(int64_t)j * C + c], mean[c], s);
    s = mg_wave_sum(s);
    if (lane == 0) hid[j] = mg_max(s + br[j], 0.f);
  }
  __syncthreads();
  for (int c = wave; c < C; c += 4) {                    // one wave per gate
    float s = 0.f;
    for (int j = lane; j < R; j += 64) s = fmaf(we[(int64_t)c * R + j], hid[j], s);
    s = mg_wave_sum(s);
    if (lane == 0) gate[b * C + c] = mg_hsig(s + be[c]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Pointwise GEMM.  Workgroup = 4 waves = 64 pixel rows x (16 NT) output channels; wave w owns rows m0 + 16 w .. + 15.
constexpr int MG_NT = 4;

template <typename TW>
__global__ __launch_bounds__(256) void mg_pw_kernel(const float* __restrict__ a, int64_t M, int K, const TW* __restrict__ w, int N,
                                                     const float* __restrict__ bias, const float* __restrict__ gate, int HW, int act,
                                                     const float* __restrict__ resid, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = 4 * (lane >> 4);
  const int64_t row = (int64_t)blockIdx.x * 64 + wave * 16 + r16;
  const bool rok = row < M;
  const int tn0 = blockIdx.y * MG_NT;
  const int ntiles = (N + 15) >> 4;
  const float* ar = a + (rok ? row : 0) * K;
  const float* gr = gate ? gate + ((rok ? row : 0) / HW) * K : nullptr;
  f32x4v acc[MG_NT];
#pragma unroll
  for (int t = 0; t < MG_NT; ++t) acc[t] = f32x4v{0.f, 0.f, 0.f, 0.f};
  if constexpr (sizeof(TW) == 4) {
    // exact fp32: this thread's pixel `row`, channels 16 (tn0 + t) + kq .. + 3; one chain per output, k ascending
    if (rok) {
      for (int k = 0; k < K; k += 4) {
        float4 av = *reinterpret_cast<const float4*>(ar + k);
        if (gr) { const float4 gv = *reinterpret_cast<const float4*>(gr + k); av.x *= gv.x; av.y *= gv.y; av.z *= gv.z; av.w *= gv.w; }
#pragma unroll
        for (int t = 0; t < MG_NT; ++t) {
          const int n = (tn0 + t) * 16 + kq;
          if (n >= N) continue;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float4 wv = *reinterpret_cast<const float4*>(w + (int64_t)(n + i) * K + k);
            acc[t][i] = fmaf(av.w, wv.w, fmaf(av.z, wv.z, fmaf(av.y, wv.y, fmaf(av.x, wv.x, acc[t][i]))));
          }
        }
      }
    }
  } else {
    typedef MgMma<TW> MM;
    const int Kp = (K + 15) & ~15;
    for (int k0 = 0; k0 < K; k0 += 16) {
      const int k = k0 + kq;
      float4 av = make_float4(0.f, 0.f, 0.f, 0.f);
      if (rok && k < K) {                                // K % 4 == 0: a quad is inside K or outside it as a whole
        av = *reinterpret_cast<const float4*>(ar + k);
        if (gr) { const float4 gv = *reinterpret_cast<const float4*>(gr + k); av.x *= gv.x; av.y *= gv.y; av.z *= gv.z; av.w *= gv.w; }
      }
      typename MM::V hi, lo;
      MM::split(hi, lo, 0, av.x); MM::split(hi, lo, 1, av.y); MM::split(hi, lo, 2, av.z); MM::split(hi, lo, 3, av.w);
#pragma unroll
      for (int t = 0; t < MG_NT; ++t) {
        if (tn0 + t >= ntiles) continue;                 // (uniform over the workgroup)
        // weight rows are padded to 16 n-tiles x Kp columns with zeros: no bounds test
        const typename MM::V wv = *reinterpret_cast<const typename MM::V*>(w + ((int64_t)(tn0 + t) * 16 + r16) * Kp + k);
        acc[t] = MM::mma(wv, lo, MM::mma(wv, hi, acc[t]));
      }
    }
  }
  if (!rok) return;
  // both forms: this lane holds pixel `row`, channels 16 (tn0 + t) + kq .. + 3
#pragma unroll
  for (int t = 0; t < MG_NT; ++t) {
    const int n = (tn0 + t) * 16 + kq;
    if (n >= N) continue;                                // N % 4 == 0
    const float4 bv = *reinterpret_cast<const float4*>(bias + n);
    float4 v = make_float4(mg_act(acc[t][0] + bv.x, act), mg_act(acc[t][1] + bv.y, act), mg_act(acc[t][2] + bv.z, act), mg_act(acc[t][3] + bv.w, act));
    if (resid) {
      const float4 rv = *reinterpret_cast<const float4*>(resid + row * N + n);
      v.x += rv.x; v.y += rv.y; v.z += rv.z; v.w += rv.w;
    }
    *reinterpret_cast<float4*>(out + row * N + n) = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mg_pool_kernel(const float* __restrict__ t, int64_t total, int HW, int C, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t b = idx / C;
  const int c = (int)(idx % C);
  const float* tp = t + b * (int64_t)HW * C + c;
  float s = 0.f;
  for (int p = 0; p < HW; ++p) s += tp[(int64_t)p * C];
  out[idx] = s / (float)HW;
}

__global__ __launch_bounds__(256) void mg_finish_kernel(float* __restrict__ emb, int D, int l2, int* __restrict__ status) {
  __shared__ float ss[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* e = emb + (int64_t)blockIdx.x * D;
  float sq = 0.f;
  bool bad = false;
  for (int d = tid; d < D; d += 256) {
    const float v = e[d];
    bad |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
    sq = fmaf(v, v, sq);
  }
  if (l2) {
    sq = mg_wave_sum(sq);
    if (lane == 0) ss[wave] = sq;
    __syncthreads();
    const float nr = sqrtf((ss[0] + ss[1]) + (ss[2] + ss[3]));
    const float den = nr < 1e-12f ? 1e-12f : nr;         // F.normalize: x / max(||x||, eps); a NaN norm stays NaN, as torch's clamp_min
    for (int d = tid; d < D; d += 256) e[d] = e[d] / den;
  }
  if (bad) atomicOr(status, 1);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
static inline unsigned mg_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

int mg_stem(const float* x, int B, int S, const float* w, const float* b, float* out, hipStream_t s) {
  const int64_t npix = (int64_t)B * (S / 2) * (S / 2);
  hipLaunchKernelGGL(mg_stem_kernel, dim3(mg_blocks(npix)), dim3(256), 0, s, x, npix, S, w, b, out);
  return check_launch("mg_stem");
}

int mg_dw(const float* in, int B, int H, int C, int k, int stride, const float* w, const float* b, int act, float* out, int Ho, hipStream_t s) {
  if (C % 4 || (k != 3 && k != 5) || (stride != 1 && stride != 2)) return fail(EFFOCR_EUNSUPPORTED, "mg_dw: unsupported geometry");
  const int64_t total = (int64_t)B * Ho * Ho * (C / 4);
  if (k == 3) hipLaunchKernelGGL(mg_dw_kernel<3>, dim3(mg_blocks(total)), dim3(256), 0, s, in, total, H, C, stride, w, b, act, out, Ho);
  else hipLaunchKernelGGL(mg_dw_kernel<5>, dim3(mg_blocks(total)), dim3(256), 0, s, in, total, H, C, stride, w, b, act, out, Ho);
  return check_launch("mg_dw");
}

int mg_se_gate(const float* t, int B, int HW, int C, int R, const float* wr, const float* br, const float* we, const float* be, float* gate,
               hipStream_t s) {
  if (C > MG_SE_MAXC || R > MG_SE_MAXR) return fail(EFFOCR_EUNSUPPORTED, "mg_se_gate: squeeze-excite wider than the kernel's LDS tables");
  hipLaunchKernelGGL(mg_se_gate_kernel, dim3((unsigned)B), dim3(256), 0, s, t, HW, C, R, wr, br, we, be, gate);
  return check_launch("mg_se_gate");
}

int mg_pw(int prec, const float* a, int64_t M, int K, const void* w, int N, const float* bias, const float* gate, int HW, int act,
          const float* resid, float* out, hipStream_t s) {
  if (K % 4 || N % 4) return fail(EFFOCR_EUNSUPPORTED, "mg_pw: K and N must be multiples of 4");
  const int ntiles = (N + 15) / 16;
  const dim3 grid((unsigned)((M + 63) / 64), (unsigned)((ntiles + MG_NT - 1) / MG_NT));
  if (prec == PREC_FP32)
    hipLaunchKernelGGL(mg_pw_kernel<float>, grid, dim3(256), 0, s, a, M, K, static_cast<const float*>(w), N, bias, gate, HW, act, resid, out);
  else if (prec == PREC_FP16)
    hipLaunchKernelGGL(mg_pw_kernel<_Float16>, grid, dim3(256), 0, s, a, M, K, static_cast<const _Float16*>(w), N, bias, gate, HW, act, resid, out);
  else
    hipLaunchKernelGGL(mg_pw_kernel<__bf16>, grid, dim3(256), 0, s, a, M, K, static_cast<const __bf16*>(w), N, bias, gate, HW, act, resid, out);
  return check_launch("mg_pw");
}

int mg_pool(const float* t, int B, int HW, int C, float* out, hipStream_t s) {
  const int64_t total = (int64_t)B * C;
  hipLaunchKernelGGL(mg_pool_kernel, dim3(mg_blocks(total)), dim3(256), 0, s, t, total, HW, C, out);
  return check_launch("mg_pool");
}

int mg_finish(float* emb, int B, int D, int l2, int* status, hipStream_t s) {
  hipLaunchKernelGGL(mg_finish_kernel, dim3((unsigned)B), dim3(256), 0, s, emb, D, l2, status);
  return check_launch("mg_finish");
}

}  // namespace effocr
