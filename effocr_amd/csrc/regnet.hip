// RegNetX / RegNetY (regnetx_002 ... regnety_016) kernels on gfx950 that the MobileNetV3 family's file does not have
// (libeffocr_regnet.so; regnet_api.hip: regnet_forward; DESIGN.md "RegNet").  The 1x1 convolutions, the pool and the normalisation are
// mnv3g.hip's mg_pw / mg_pool / mg_finish.
//
//   rg_stem     3x3/2 stem conv to 32 channels + folded BN + ReLU, NCHW crops -> channels-last fp32, one output pixel per thread.
//   rg_gconv    grouped 3x3 (group width 8 / 16 / 24), stride 1 / 2, + folded BN + ReLU.  A workgroup owns a run of 64 output pixels of
//               one crop and one tile of 16 output channels; wave w owns pixels 16 w .. 16 w + 15 of the run.  16-bit modes: an implicit
//               GEMM on v_mfma_f32_16x16x16 over 9 taps x the input tiles of the tile's window (regnet.hpp), the activation as hi + lo
//               parts; fp32 mode: one FMA chain per output.  The workgroup also emits the per-channel sums of what it stored (RegNetY).
//   rg_se_gate  one crop per workgroup, from the tile sums alone: means (tiles in order), fc1 + ReLU (a wave per hidden unit), fc2 +
//               sigmoid (a thread per channel, coalesced over the transposed weight).
//   rg_gather2  the even rows and columns of a map: the rows the strided 1x1 shortcut reads.
//   rg_relu     ReLU in place: the block's activation AFTER the residual add.
// Every reduction runs in an order fixed by the shapes and a crop's values depend on that crop's data alone.
#include "regnet.hpp"

namespace effocr {
namespace {

// NaN-propagating maximum (as torch's relu; fmaxf would turn a NaN crop into a finite embedding)
__device__ __forceinline__ float rg_relu1(float x) { return __builtin_elementwise_maximum(x, 0.0f); }
__device__ __forceinline__ float rg_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float rg_wave_sum(float v) {           // xor butterfly: every lane ends with the same sum, same order every time
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

template <typename TW> struct RgMma;
template <> struct RgMma<_Float16> {
  typedef h16x4 V;
  static __device__ __forceinline__ void split(V& hi, V& lo, int j, float x) { const _Float16 h = (_Float16)x; hi[j] = h; lo[j] = (_Float16)(x - (float)h); }
  static __device__ __forceinline__ f32x4v mma(V a, V b, f32x4v c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
};
template <> struct RgMma<__bf16> {
  typedef i16x4 V;
  static __device__ __forceinline__ void split(V& hi, V& lo, int j, float x) {
    const __bf16 h = (__bf16)x;
    hi[j] = __builtin_bit_cast(short, h); lo[j] = __builtin_bit_cast(short, (__bf16)(x - (float)h));
  }
  static __device__ __forceinline__ f32x4v mma(V a, V b, f32x4v c) { return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0); }
};

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rg_stem_kernel(const float* __restrict__ x, int64_t npix, int S, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= npix) return;
  const int S2 = S / 2;
  const int ox = (int)(idx % S2), oy = (int)((idx / S2) % S2);
  const int64_t b = idx / ((int64_t)S2 * S2);
  float acc[RG_STEM_C];
#pragma unroll
  for (int c = 0; c < RG_STEM_C; ++c) acc[c] = bias[c];
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
        const float* wt = w + ((ci * 3 + ky) * 3 + kx) * RG_STEM_C;   // (uniform over the wave: scalar loads)
#pragma unroll
        for (int c = 0; c < RG_STEM_C; ++c) acc[c] = fmaf(v, wt[c], acc[c]);
      }
    }
  }
  float4* o = reinterpret_cast<float4*>(out + idx * RG_STEM_C);
#pragma unroll
  for (int c = 0; c < RG_STEM_C; c += 4) o[c / 4] = make_float4(rg_relu1(acc[c]), rg_relu1(acc[c + 1]), rg_relu1(acc[c + 2]), rg_relu1(acc[c + 3]));
}

// ---------------------------------------------------------------------------------------------------------------------------
// grid (rg_tiles(Ho), channel tiles, crops), 256 threads.  As in mg_pw a lane holds output pixel r16 = lane & 15 of its wave's 16 and
// the FOUR CONSECUTIVE output channels 16 ct + kq .. + 3, kq = 4 (lane >> 4); as the MFMA's B operand it supplies input channels
// kq .. kq + 3 of the current input tile at its pixel's tap.
template <typename TW>
__global__ __launch_bounds__(256) void rg_gconv_kernel(const float* __restrict__ in, int H, int C, int stride, int gw, const TW* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ out, int Ho, float* __restrict__ part) {
  __shared__ float red[RG_PIX_TILE * RG_CH_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, kq = 4 * (lane >> 4);
  const int ct = blockIdx.y;
  const int64_t b = blockIdx.z;
  const int lp = wave * 16 + r16;                          // pixel of the run
  const int p = blockIdx.x * RG_PIX_TILE + lp;             // output pixel of the crop
  const bool pok = p < Ho * Ho;
  const int oy = pok ? p / Ho : 0, ox = pok ? p - oy * Ho : 0;
  const float* ip = in + b * (int64_t)H * H * C;
  const int o = ct * RG_CH_TILE + kq;                      // this lane's first output channel; C % 4 == 0: the quad is inside C or outside
  const bool ook = o < C;
  f32x4v acc = f32x4v{0.f, 0.f, 0.f, 0.f};
  if constexpr (sizeof(TW) == 4) {
    if (pok && ook) {
      const int g0 = o / gw * gw;                          // gw % 4 == 0: the four channels are in one group
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * stride + ky - 1;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = ox * stride + kx - 1;
          if (ix < 0 || ix >= H) continue;
          const float* xr = ip + ((int64_t)iy * H + ix) * C + g0;
          const float* wr = w + ((int64_t)(ky * 3 + kx) * C + o) * gw;
          for (int ci = 0; ci < gw; ci += 4) {
            const float4 xv = *reinterpret_cast<const float4*>(xr + ci);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float4 wv = *reinterpret_cast<const float4*>(wr + (int64_t)i * gw + ci);
              acc[i] = fmaf(xv.w, wv.w, fmaf(xv.z, wv.z, fmaf(xv.y, wv.y, fmaf(xv.x, wv.x, acc[i]))));
            }
          }
        }
      }
    }
  } else {
    typedef RgMma<TW> MM;
    int kt0, nkt;
    rg_window(gw, C, ct, &kt0, &nkt);                      // (uniform over the workgroup)
    const int NKT = rg_nkt(gw);
    const TW* wt = w + (int64_t)ct * 9 * NKT * 256 + r16 * 16 + kq;
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * stride + ky - 1;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * stride + kx - 1;
        const bool tok = pok && iy >= 0 && iy < H && ix >= 0 && ix < H;
        const float* xr = ip + (tok ? ((int64_t)iy * H + ix) * C : 0);
        for (int j = 0; j < nkt; ++j) {
          const int c = (kt0 + j) * 16 + kq;
          float4 av = make_float4(0.f, 0.f, 0.f, 0.f);     // a tap outside the map, a pixel outside the crop, a channel outside C: zeros
          if (tok && c < C) av = *reinterpret_cast<const float4*>(xr + c);
          typename MM::V hi, lo;
          MM::split(hi, lo, 0, av.x); MM::split(hi, lo, 1, av.y); MM::split(hi, lo, 2, av.z); MM::split(hi, lo, 3, av.w);
          const typename MM::V wv = *reinterpret_cast<const typename MM::V*>(wt + ((ky * 3 + kx) * NKT + j) * 256);
          acc = MM::mma(wv, lo, MM::mma(wv, hi, acc));
        }
      }
    }
  }
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (pok && ook) {
    const float4 bv = *reinterpret_cast<const float4*>(bias + o);
    v = make_float4(rg_relu1(acc[0] + bv.x), rg_relu1(acc[1] + bv.y), rg_relu1(acc[2] + bv.z), rg_relu1(acc[3] + bv.w));
    *reinterpret_cast<float4*>(out + (b * Ho * Ho + p) * (int64_t)C + o) = v;
  }
  if (part) {                                              // (uniform over the grid)
    *reinterpret_cast<float4*>(red + lp * RG_CH_TILE + kq) = v;
    __syncthreads();
    const int oc = ct * RG_CH_TILE + tid;
    if (tid < RG_CH_TILE && oc < C) {
      float s = 0.f;
      for (int q = 0; q < RG_PIX_TILE; ++q) s += red[q * RG_CH_TILE + tid];
      part[(b * gridDim.x + blockIdx.x) * (int64_t)C + oc] = s;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rg_se_gate_kernel(const float* __restrict__ part, int NT, int HW, int C, int R, const float* __restrict__ w1,
                                                          const float* __restrict__ b1, const float* __restrict__ w2t,
                                                          const float* __restrict__ b2, float* __restrict__ gate) {
  __shared__ float mean[RG_SE_MAXC];
  __shared__ float hid[RG_SE_MAXR];
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
    for (int c = lane; c < C; c += 64) s = fmaf(w1[(int64_t)j * C + c], mean[c], s);
    s = rg_wave_sum(s);
    if (lane == 0) hid[j] = rg_relu1(s + b1[j]);
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {                   // one thread per gate, hidden units ascending
    float s = 0.f;
    for (int j = 0; j < R; ++j) s = fmaf(w2t[(int64_t)j * C + c], hid[j], s);
    gate[b * C + c] = rg_sigmoid(s + b2[c]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rg_gather2_kernel(const float* __restrict__ in, int64_t total, int H, int C4, int Ho, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (crop, oy, ox, channel quad), the quad fastest
  if (idx >= total) return;
  const int q = (int)(idx % C4);
  const int64_t px = idx / C4;
  const int ox = (int)(px % Ho), oy = (int)((px / Ho) % Ho);
  const int64_t b = px / ((int64_t)Ho * Ho);
  reinterpret_cast<float4*>(out)[idx] = reinterpret_cast<const float4*>(in)[((b * H + 2 * oy) * H + 2 * ox) * C4 + q];
}

__global__ __launch_bounds__(256) void rg_relu_kernel(float* __restrict__ x, int64_t n4) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n4) return;
  float4 v = reinterpret_cast<float4*>(x)[idx];
  v.x = rg_relu1(v.x); v.y = rg_relu1(v.y); v.z = rg_relu1(v.z); v.w = rg_relu1(v.w);
  reinterpret_cast<float4*>(x)[idx] = v;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
static inline unsigned rg_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

int rg_stem(const float* x, int B, int S, const float* w, const float* b, float* out, hipStream_t s) {
  if (S <= 0 || S % 2 || B <= 0) return fail(EFFOCR_EUNSUPPORTED, "rg_stem: unsupported geometry");
  const int64_t npix = (int64_t)B * (S / 2) * (S / 2);
  hipLaunchKernelGGL(rg_stem_kernel, dim3(rg_blocks(npix)), dim3(256), 0, s, x, npix, S, w, b, out);
  return check_launch("rg_stem");
}

int rg_gconv(int prec, const float* in, int B, int H, int C, int stride, int gw, const void* w, const float* bias, float* out, int Ho,
             float* part, hipStream_t s) {
  if ((gw != 8 && gw != 16 && gw != 24) || C <= 0 || C % gw || (stride != 1 && stride != 2) || H <= 0 || Ho != (H - 1) / stride + 1 ||
      B <= 0 || B > 65535 || (C + 15) / 16 > 65535 || prec < 0 || prec > 2)
    return fail(EFFOCR_EUNSUPPORTED, "rg_gconv: unsupported geometry");
  const dim3 grid((unsigned)rg_tiles(Ho), (unsigned)((C + RG_CH_TILE - 1) / RG_CH_TILE), (unsigned)B);
  if (prec == PREC_FP32)
    hipLaunchKernelGGL(rg_gconv_kernel<float>, grid, dim3(256), 0, s, in, H, C, stride, gw, static_cast<const float*>(w), bias, out, Ho, part);
  else if (prec == PREC_FP16)
    hipLaunchKernelGGL(rg_gconv_kernel<_Float16>, grid, dim3(256), 0, s, in, H, C, stride, gw, static_cast<const _Float16*>(w), bias, out, Ho, part);
  else
    hipLaunchKernelGGL(rg_gconv_kernel<__bf16>, grid, dim3(256), 0, s, in, H, C, stride, gw, static_cast<const __bf16*>(w), bias, out, Ho, part);
  return check_launch("rg_gconv");
}

int rg_se_gate(const float* part, int B, int NT, int HW, int C, int R, const float* w1, const float* b1, const float* w2t, const float* b2,
               float* gate, hipStream_t s) {
  if (C <= 0 || R <= 0 || C > RG_SE_MAXC || R > RG_SE_MAXR || NT <= 0 || HW <= 0 || B <= 0)
    return fail(EFFOCR_EUNSUPPORTED, "rg_se_gate: squeeze-excite wider than the kernel's LDS tables");
  hipLaunchKernelGGL(rg_se_gate_kernel, dim3((unsigned)B), dim3(256), 0, s, part, NT, HW, C, R, w1, b1, w2t, b2, gate);
  return check_launch("rg_se_gate");
}

int rg_gather2(const float* in, int B, int H, int C, float* out, hipStream_t s) {
  if (B <= 0 || H <= 0 || C <= 0 || C % 4) return fail(EFFOCR_EUNSUPPORTED, "rg_gather2: unsupported geometry");
  const int Ho = (H - 1) / 2 + 1;
  const int64_t total = (int64_t)B * Ho * Ho * (C / 4);
  hipLaunchKernelGGL(rg_gather2_kernel, dim3(rg_blocks(total)), dim3(256), 0, s, in, total, H, C / 4, Ho, out);
  return check_launch("rg_gather2");
}

int rg_relu(float* x, int64_t n, hipStream_t s) {
  if (n <= 0 || n % 4) return fail(EFFOCR_EUNSUPPORTED, "rg_relu: the element count must be a positive multiple of 4");
  hipLaunchKernelGGL(rg_relu_kernel, dim3(rg_blocks(n / 4)), dim3(256), 0, s, x, n / 4);
  return check_launch("rg_relu");
}

}  // namespace effocr
