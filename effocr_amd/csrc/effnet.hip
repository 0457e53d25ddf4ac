// EfficientNet-B0 (efficientnet_b0 / tf_efficientnet_b0) kernels on gfx950 that the MobileNetV3 family's file does not have
// (libeffocr_effnet.so; effnet_api.hip: effnet_forward; DESIGN.md "EfficientNet-B0").  The 1x1 convolutions, the pool and the
// normalisation are mnv3g.hip's mg_pw / mg_pool / mg_finish.
//
//   ef_stem     3x3/2 stem conv to 32 channels + folded BN + SiLU, NCHW crops -> channels-last fp32, one output pixel per thread; the
//               "pad before" argument selects symmetric or TensorFlow SAME padding.
//   ef_dw       depthwise 3x3 / 5x5, stride 1 / 2, "pad before" argument, + folded BN + SiLU.  A workgroup owns one 16 x 16 output tile
//               of one crop and a run of channel quads; a thread keeps ONE channel quad (its taps in registers) and walks the tile's
//               pixels, so it can also sum what it writes: the workgroup emits the tile's per-channel sums, the squeeze-excite input.
//   ef_se_gate  one crop per workgroup, from the tile sums alone: means (tiles in order), reduce FC + SiLU (a wave per hidden unit),
//               expand FC + sigmoid (a thread per channel, coalesced over the transposed weight).
// Every reduction runs in an order fixed by the shapes and a crop's values depend on that crop's data alone.
#include "effnet.hpp"

namespace effocr {
namespace {

__device__ __forceinline__ float ef_wave_sum(float v) {           // xor butterfly: every lane ends with the same sum, same order every time
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// the gate's two activations in the IEEE form (a few hundred values per crop: their cost does not matter, their error feeds every pixel)
__device__ __forceinline__ float ef_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ef_stem_kernel(const float* __restrict__ x, int64_t npix, int S, int padb, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= npix) return;
  const int S2 = S / 2;
  const int ox = (int)(idx % S2), oy = (int)((idx / S2) % S2);
  const int64_t b = idx / ((int64_t)S2 * S2);
  float acc[EF_STEM_C];
#pragma unroll
  for (int c = 0; c < EF_STEM_C; ++c) acc[c] = bias[c];
  for (int ci = 0; ci < 3; ++ci) {
    const float* xp = x + (b * 3 + ci) * (int64_t)S * S;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = 2 * oy + ky - padb;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = 2 * ox + kx - padb;
        if (iy < 0 || iy >= S || ix < 0 || ix >= S) continue;
        const float v = xp[(int64_t)iy * S + ix];
        const float* wt = w + ((ci * 3 + ky) * 3 + kx) * EF_STEM_C;   // (uniform over the wave: scalar loads)
#pragma unroll
        for (int c = 0; c < EF_STEM_C; ++c) acc[c] = fmaf(v, wt[c], acc[c]);
      }
    }
  }
  float4* o = reinterpret_cast<float4*>(out + idx * EF_STEM_C);
#pragma unroll
  for (int c = 0; c < EF_STEM_C; c += 4) o[c / 4] = make_float4(silu_fast(acc[c]), silu_fast(acc[c + 1]), silu_fast(acc[c + 2]), silu_fast(acc[c + 3]));
}

// ---------------------------------------------------------------------------------------------------------------------------
// grid (tiles of the map, channel-quad runs, crops); block = QW x PS threads: thread (ql, ps) owns channel quad blockIdx.y * QW + ql and
// the tile pixels ps, ps + PS, ... (row-major inside the tile).  Sums: a thread's pixels ascending, then the PS threads of a quad ascending.
template <int KS>
__global__ __launch_bounds__(256) void ef_dw_kernel(const float* __restrict__ in, int H, int C, int stride, int padb, const float* __restrict__ w,
                                                     const float* __restrict__ bias, float* __restrict__ out, int Ho, int QW, int PS,
                                                     float* __restrict__ part) {
  __shared__ float4 red[256];
  const int tid = threadIdx.x;
  const int ps = tid / QW, ql = tid - ps * QW;
  const int c = (blockIdx.y * QW + ql) * 4;
  const int ntx = (Ho + EF_TILE - 1) / EF_TILE;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
  const int64_t b = blockIdx.z;
  const float* ip = in + b * (int64_t)H * H * C + c;
  float* op = out + b * (int64_t)Ho * Ho * C + c;
  float4 wt[KS * KS];
#pragma unroll
  for (int t = 0; t < KS * KS; ++t) wt[t] = *reinterpret_cast<const float4*>(w + t * C + c);
  const float4 bv = *reinterpret_cast<const float4*>(bias + c);
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int lp = ps; lp < EF_TILE * EF_TILE; lp += PS) {
    const int oy = ty * EF_TILE + lp / EF_TILE, ox = tx * EF_TILE + lp % EF_TILE;
    if (oy >= Ho || ox >= Ho) continue;
    float4 acc = bv;
#pragma unroll
    for (int ky = 0; ky < KS; ++ky) {
      const int iy = oy * stride + ky - padb;
      if (iy < 0 || iy >= H) continue;
#pragma unroll
      for (int kx = 0; kx < KS; ++kx) {
        const int ix = ox * stride + kx - padb;
        if (ix < 0 || ix >= H) continue;
        const float4 v = *reinterpret_cast<const float4*>(ip + ((int64_t)iy * H + ix) * C);
        const float4 k4 = wt[ky * KS + kx];
        acc.x = fmaf(v.x, k4.x, acc.x); acc.y = fmaf(v.y, k4.y, acc.y); acc.z = fmaf(v.z, k4.z, acc.z); acc.w = fmaf(v.w, k4.w, acc.w);
      }
    }
    const float4 r = make_float4(silu_fast(acc.x), silu_fast(acc.y), silu_fast(acc.z), silu_fast(acc.w));
    *reinterpret_cast<float4*>(op + ((int64_t)oy * Ho + ox) * C) = r;
    sum.x += r.x; sum.y += r.y; sum.z += r.z; sum.w += r.w;
  }
  red[tid] = sum;
  __syncthreads();
  if (ps == 0) {
    float4 s4 = red[ql];
    for (int i = 1; i < PS; ++i) { const float4 o = red[i * QW + ql]; s4.x += o.x; s4.y += o.y; s4.z += o.z; s4.w += o.w; }
    *reinterpret_cast<float4*>(part + (b * gridDim.x + blockIdx.x) * (int64_t)C + c) = s4;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ef_se_gate_kernel(const float* __restrict__ part, int NT, int HW, int C, int R, const float* __restrict__ wr,
                                                          const float* __restrict__ br, const float* __restrict__ wet,
                                                          const float* __restrict__ be, float* __restrict__ gate) {
  __shared__ float mean[EF_SE_MAXC];
  __shared__ float hid[EF_SE_MAXR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const float* pp = part + b * (int64_t)NT * C;
  for (int c = tid; c < C; c += 256) {
    float s = 0.f;
    for (int t = 0; t < NT; ++t) s += pp[(int64_t)t * C + c];
    mean[c] = s / (float)HW;
  }
  __syncthreads();
  for (int j = wave; j < R; j += 4) {                    // one wave per hidden unit
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = fmaf(wr[(int64_t)j * C + c], mean[c], s);
    s = ef_wave_sum(s);
    if (lane == 0) { const float h = s + br[j]; hid[j] = h * ef_sigmoid(h); }
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {                   // one thread per gate, hidden units ascending
    float s = 0.f;
    for (int j = 0; j < R; ++j) s = fmaf(wet[(int64_t)j * C + c], hid[j], s);
    gate[b * C + c] = ef_sigmoid(s + be[c]);
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
int ef_stem(const float* x, int B, int S, int padb, const float* w, const float* b, float* out, hipStream_t s) {
  if (S % 2 || (padb != 0 && padb != 1)) return fail(EFFOCR_EUNSUPPORTED, "ef_stem: unsupported geometry");
  const int64_t npix = (int64_t)B * (S / 2) * (S / 2);
  hipLaunchKernelGGL(ef_stem_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, x, npix, S, padb, w, b, out);
  return check_launch("ef_stem");
}

int ef_dw(const float* in, int B, int H, int C, int k, int stride, int padb, const float* w, const float* b, float* out, int Ho, float* part,
          hipStream_t s) {
  if (C <= 0 || C % 4 || (k != 3 && k != 5) || (stride != 1 && stride != 2) || padb < 0 || padb > k / 2 || Ho != (H - 1) / stride + 1 ||
      B <= 0 || B > 65535)
    return fail(EFFOCR_EUNSUPPORTED, "ef_dw: unsupported geometry");
  const int C4 = C / 4;
  int QW = 1;
  for (int d = 1; d <= 64 && d <= C4; ++d)
    if (C4 % d == 0) QW = d;                              // the widest run of channel quads (<= 64) that divides the channels
  const int PS = 256 / QW;
  const dim3 grid((unsigned)ef_tiles(Ho), (unsigned)(C4 / QW), (unsigned)B), block((unsigned)(QW * PS));
  if (k == 3) hipLaunchKernelGGL(ef_dw_kernel<3>, grid, block, 0, s, in, H, C, stride, padb, w, b, out, Ho, QW, PS, part);
  else hipLaunchKernelGGL(ef_dw_kernel<5>, grid, block, 0, s, in, H, C, stride, padb, w, b, out, Ho, QW, PS, part);
  return check_launch("ef_dw");
}

int ef_se_gate(const float* part, int B, int NT, int HW, int C, int R, const float* wr, const float* br, const float* wet, const float* be,
               float* gate, hipStream_t s) {
  if (C <= 0 || R <= 0 || C > EF_SE_MAXC || R > EF_SE_MAXR || NT <= 0 || HW <= 0 || B <= 0)
    return fail(EFFOCR_EUNSUPPORTED, "ef_se_gate: squeeze-excite wider than the kernel's LDS tables");
  hipLaunchKernelGGL(ef_se_gate_kernel, dim3((unsigned)B), dim3(256), 0, s, part, NT, HW, C, R, wr, br, wet, be, gate);
  return check_launch("ef_se_gate");
}

}  // namespace effocr
