// ConvNeXt encoder kernels on gfx950 (timm convnext_tiny semantics; api.hip: convnext_forward).
//
// Layout: the residual stream is fp32, channels-last, [tokens][Cp] with Cp = the stage width rounded up to 128 (96 -> 128,
// 192 -> 256): the pointwise linears then run on gemm_nt / gemm2_nt unchanged, and the pad channels hold zeros throughout (zero
// weights, biases and layer scale; every LayerNorm here masks them out).  The linear operands are in the handle's precision.
//
// Thread map shared by the per-token kernels: a SEGMENT of Cq = Cp / 4 threads owns whole tokens, thread t of a segment holds
// channels 4t .. 4t+3 (one float4) of each of them.  Cq is a multiple of 32, so a segment is a whole number of 32-lane halves of
// waves: a LayerNorm statistic is reduced with xor-shuffles inside each half, then the halves of a segment are summed through LDS
// in a fixed order.  No result depends on the batch size, the chunking or the launch geometry (batch invariance).
#include "common.hpp"
#include "kernels.hpp"

namespace effocr {
namespace {

constexpr float CNX_EPS = 1e-6f;

__device__ __forceinline__ float half_sum(float v) {      // sum over the 32-lane half of the wave (every lane gets it)
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// v[n] summed over the segment of this thread, for N values at once.  hs: LDS [halves per block][N].  Two barriers.
template <int N>
__device__ __forceinline__ void seg_sum(float (&v)[N], float* hs, int seg, int halves_per_seg) {
  const int hid = threadIdx.x >> 5;
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = half_sum(v[n]);
  if ((threadIdx.x & 31) == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) hs[hid * N + n] = v[n];
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) {
    float t = 0.f;
    for (int h = 0; h < halves_per_seg; ++h) t += hs[(seg * halves_per_seg + h) * N + n];
    v[n] = t;
  }
  __syncthreads();
}

template <typename TO> __device__ __forceinline__ void store4v(TO* p, f32x4 v) {
  if constexpr (sizeof(TO) == 4) *reinterpret_cast<f32x4*>(p) = v;
  else *reinterpret_cast<u32x2*>(p) = pack4<TO>(v[0], v[1], v[2], v[3]);
}

// LayerNorm of N tokens whose channels are spread over a segment (two-pass: mean, then the mean of squared deviations).
// real = this thread's channels are real (not padding); C = real channel count.
template <int N>
__device__ __forceinline__ void seg_layernorm(f32x4 (&v)[N], bool real, int C, int c4, const float* lnw, const float* lnb,
                                              float* hs, int seg, int hps) {
  float s[N];
#pragma unroll
  for (int n = 0; n < N; ++n) s[n] = real ? (v[n][0] + v[n][1]) + (v[n][2] + v[n][3]) : 0.f;
  seg_sum<N>(s, hs, seg, hps);
  const float invC = 1.0f / (float)C;
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const float mean = s[n] * invC;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[n][e] -= mean;
    s[n] = real ? (v[n][0] * v[n][0] + v[n][1] * v[n][1]) + (v[n][2] * v[n][2] + v[n][3] * v[n][3]) : 0.f;
  }
  seg_sum<N>(s, hs, seg, hps);
  f32x4 g = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
  if (real) { g = *reinterpret_cast<const f32x4*>(lnw + c4); b = *reinterpret_cast<const f32x4*>(lnb + c4); }
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const float rstd = 1.0f / sqrtf(s[n] * invC + CNX_EPS);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[n][e] = real ? v[n][e] * rstd * g[e] + b[e] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// stem: Conv2d(3, C0, 4, stride 4) + bias + LayerNorm over C0, straight from the NCHW crops.  Block = 8 segments of 32 threads
// (Cp = 128), one token per segment; the 48 input pixels of the block's 8 tokens are staged in LDS.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cnx_stem_kernel(const float* __restrict__ img, int B, int S, const float* __restrict__ wt,
                                                        const float* __restrict__ bias, const float* __restrict__ lnw,
                                                        const float* __restrict__ lnb, int C0, float* __restrict__ x) {
  __shared__ float px[8][48];
  __shared__ float hs[8 * 1];
  const int So = S / 4;
  const int64_t M = (int64_t)B * So * So;
  const int seg = threadIdx.x >> 5, t = threadIdx.x & 31, c4 = 4 * t;
  const int64_t m = (int64_t)blockIdx.x * 8 + seg;
  const int64_t mc = m < M ? m : M - 1;
  const int64_t b = mc / ((int64_t)So * So);
  const int p = (int)(mc - b * So * So), py = p / So, pxx = p - py * So;
  for (int k = t; k < 48; k += 32) {
    const int ci = k >> 4, ky = (k >> 2) & 3, kx = k & 3;
    px[seg][k] = img[((b * 3 + ci) * S + 4 * py + ky) * (int64_t)S + 4 * pxx + kx];
  }
  __syncthreads();
  const bool real = c4 < C0;
  f32x4 v[1];
  v[0] = *reinterpret_cast<const f32x4*>(bias + c4);
#pragma unroll 8
  for (int k = 0; k < 48; ++k) {
    const float a = px[seg][k];
    const f32x4 w = *reinterpret_cast<const f32x4*>(wt + k * 128 + c4);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[0][e] = fmaf(a, w[e], v[0][e]);
  }
  seg_layernorm<1>(v, real, C0, c4, lnw, lnb, hs, seg, 1);
  if (m < M) *reinterpret_cast<f32x4*>(x + m * 128 + c4) = v[0];
}

// ---------------------------------------------------------------------------------------------------------------------------
// depthwise 7x7 (pad 3) + bias + LayerNorm -> fc1 operand.  A segment owns a strip of TH x TW output tokens of one image (TH rows,
// TW consecutive columns) and all Cp channels; a thread slides over the TH + 6 input rows of its 4 channels, each row held in
// registers as TW + 6 float4 (the 3-pixel halo included, zeros outside the image), and accumulates the 49 taps per output in
// (ky, kx) order on top of the bias.  Input re-reads: (TH + 6)(TW + 6) / (TH TW) = 7 float4 per output float4 (from L2 / MALL).
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int DW_TH = 2, DW_TW = 8, DW_NT = DW_TH * DW_TW;

template <typename TO>
__global__ __launch_bounds__(256) void cnx_dwconv_ln_kernel(const float* __restrict__ x, int B, int H, int W, int C, int Cp,
                                                             const float* __restrict__ wdw, const float* __restrict__ bdw,
                                                             const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                             TO* __restrict__ out) {
  __shared__ float hs[8 * DW_NT];
  const int Cq = Cp >> 2, segs = blockDim.x / Cq, hps = Cq >> 5;
  const int seg = threadIdx.x / Cq, t = threadIdx.x - seg * Cq, c4 = 4 * t;
  const int sx = (W + DW_TW - 1) / DW_TW, sy = (H + DW_TH - 1) / DW_TH;
  const int64_t strips = (int64_t)B * sy * sx;
  int64_t sid = (int64_t)blockIdx.x * segs + seg;
  const bool live = sid < strips;
  sid = live ? sid : strips - 1;
  const int64_t b = sid / ((int64_t)sy * sx);
  const int r = (int)(sid - b * sy * sx), y0 = (r / sx) * DW_TH, x0 = (r % sx) * DW_TW;
  const bool real = c4 < C;
  const float* xb = x + (b * H) * (int64_t)W * Cp + c4;

  f32x4 acc[DW_NT];
  {
    const f32x4 bv = real ? *reinterpret_cast<const f32x4*>(bdw + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < DW_NT; ++n) acc[n] = bv;
  }
  if (real) {
#pragma unroll
    for (int ir = 0; ir < DW_TH + 6; ++ir) {
      const int yy = y0 - 3 + ir;
      if (yy < 0 || yy >= H) continue;                   // (uniform over the segment)
      f32x4 row[DW_TW + 6];
#pragma unroll
      for (int i = 0; i < DW_TW + 6; ++i) {
        const int xx = x0 - 3 + i;
        row[i] = (xx >= 0 && xx < W) ? *reinterpret_cast<const f32x4*>(xb + ((int64_t)yy * W + xx) * Cp) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int o = 0; o < DW_TH; ++o) {
        const int ky = ir - o;
        if (ky < 0 || ky > 6) continue;                  // (compile-time)
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(wdw + (ky * 7 + kx) * Cp + c4);
#pragma unroll
          for (int n = 0; n < DW_TW; ++n)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[o * DW_TW + n][e] = fmaf(row[n + kx][e], w[e], acc[o * DW_TW + n][e]);
        }
      }
    }
  }
  seg_layernorm<DW_NT>(acc, real, C, c4, lnw, lnb, hs, seg, hps);
  if (!live) return;
#pragma unroll
  for (int o = 0; o < DW_TH; ++o) {
    const int yy = y0 + o;
    if (yy >= H) continue;
#pragma unroll
    for (int n = 0; n < DW_TW; ++n) {
      const int xx = x0 + n;
      if (xx >= W) continue;
      store4v<TO>(out + ((b * H + yy) * (int64_t)W + xx) * Cp + c4, acc[o * DW_TW + n]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// downsample LayerNorm -> space-to-depth rows (the 2x2/s2 conv is then an NT GEMM with K = 4C).  One token per segment.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename TO>
__global__ __launch_bounds__(256) void cnx_ln_s2d_kernel(const float* __restrict__ x, int B, int H, int W, int C, int Cp,
                                                          const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                          TO* __restrict__ out) {
  __shared__ float hs[8];
  const int Cq = Cp >> 2, segs = blockDim.x / Cq, hps = Cq >> 5;
  const int seg = threadIdx.x / Cq, t = threadIdx.x - seg * Cq, c4 = 4 * t;
  const int64_t M = (int64_t)B * H * W;
  const int64_t m = (int64_t)blockIdx.x * segs + seg;
  const int64_t mc = m < M ? m : M - 1;
  const bool real = c4 < C;
  f32x4 v[1];
  v[0] = real ? *reinterpret_cast<const f32x4*>(x + mc * Cp + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
  seg_layernorm<1>(v, real, C, c4, lnw, lnb, hs, seg, hps);
  if (m >= M || !real) return;
  const int64_t b = mc / ((int64_t)H * W);
  const int p = (int)(mc - b * H * W), y = p / W, xx = p - y * W;
  const int64_t orow = (b * (H / 2) + (y >> 1)) * (int64_t)(W / 2) + (xx >> 1);
  store4v<TO>(out + orow * 4 * C + ((y & 1) * 2 + (xx & 1)) * C + c4, v[0]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// head: global average pool + LayerNorm (+ F.normalize) -> emb.  One image per workgroup of Cq threads; the pooled sum runs over
// the tokens in order.  A non-finite embedding ORs 1 into the workspace status word (effocr_encoder_check_status).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cnx_head_kernel(const float* __restrict__ x, int HW, int C, int Cp, const float* __restrict__ lnw,
                                                        const float* __restrict__ lnb, int l2norm, float* __restrict__ emb,
                                                        int* __restrict__ status) {
  __shared__ float hs[8];
  const int t = threadIdx.x, c4 = 4 * t, hps = (Cp >> 2) >> 5;
  const int64_t b = blockIdx.x;
  const bool real = c4 < C;
  f32x4 v[1] = {{0.f, 0.f, 0.f, 0.f}};
  if (real) {
    const float* p = x + b * HW * (int64_t)Cp + c4;
    for (int i = 0; i < HW; ++i) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(p + (int64_t)i * Cp);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[0][e] += a[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[0][e] /= (float)HW;
  }
  seg_layernorm<1>(v, real, C, c4, lnw, lnb, hs, 0, hps);
  if (l2norm) {
    float ss[1] = {real ? (v[0][0] * v[0][0] + v[0][1] * v[0][1]) + (v[0][2] * v[0][2] + v[0][3] * v[0][3]) : 0.f};
    seg_sum<1>(ss, hs, 0, hps);
    const float nrm = fmaxf(sqrtf(ss[0]), 1e-12f);        // F.normalize: x / max(||x||, eps)
#pragma unroll
    for (int e = 0; e < 4; ++e) v[0][e] = v[0][e] / nrm;
  }
  if (!real) return;
  bool bad = false;
#pragma unroll
  for (int e = 0; e < 4; ++e) bad |= !(fabsf(v[0][e]) <= 3.0e38f);
  *reinterpret_cast<f32x4*>(emb + b * C + c4) = v[0];
  if (status && bad) atomicOr(status, 1);
}

int segs_for(int Cp) { return 256 / (Cp / 4); }          // segments per 256-thread (or smaller) workgroup

}  // namespace

int cnx_stem(const float* img, int B, int S, const float* wt, const float* bias, const float* lnw, const float* lnb, int C0, float* x,
             hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (S < 32 || S % 32 || C0 > 128 || C0 % 4) return fail(EFFOCR_EUNSUPPORTED, "cnx_stem: S % 32 == 0 and C0 <= 128 required");
  const int64_t M = (int64_t)B * (S / 4) * (S / 4);
  hipLaunchKernelGGL(cnx_stem_kernel, dim3((unsigned)((M + 7) / 8)), dim3(256), 0, s, img, B, S, wt, bias, lnw, lnb, C0, x);
  return check_launch("cnx_stem");
}

int cnx_dwconv_ln(int prec, const float* x, int B, int H, int W, int C, int Cp, const float* w, const float* bias, const float* lnw,
                  const float* lnb, void* out, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (Cp % 128 || Cp > 1024 || C > Cp || C % 4) return fail(EFFOCR_EUNSUPPORTED, "cnx_dwconv_ln: Cp must be a multiple of 128 (<= 1024)");
  const int segs = segs_for(Cp);
  const int64_t strips = (int64_t)B * ((H + DW_TH - 1) / DW_TH) * ((W + DW_TW - 1) / DW_TW);
  const dim3 grid((unsigned)((strips + segs - 1) / segs)), block(segs * (Cp / 4));
  switch (prec) {
    case PREC_BF16: hipLaunchKernelGGL(cnx_dwconv_ln_kernel<__bf16>, grid, block, 0, s, x, B, H, W, C, Cp, w, bias, lnw, lnb, static_cast<__bf16*>(out)); break;
    case PREC_FP16: hipLaunchKernelGGL(cnx_dwconv_ln_kernel<_Float16>, grid, block, 0, s, x, B, H, W, C, Cp, w, bias, lnw, lnb, static_cast<_Float16*>(out)); break;
    case PREC_FP32: hipLaunchKernelGGL(cnx_dwconv_ln_kernel<float>, grid, block, 0, s, x, B, H, W, C, Cp, w, bias, lnw, lnb, static_cast<float*>(out)); break;
    default: return fail(EFFOCR_EINVAL, "cnx_dwconv_ln: unknown precision");
  }
  return check_launch("cnx_dwconv_ln");
}

int cnx_ln_s2d(int prec, const float* x, int B, int H, int W, int C, int Cp, const float* lnw, const float* lnb, void* out, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (Cp % 128 || Cp > 1024 || C > Cp || C % 4 || H % 2 || W % 2) return fail(EFFOCR_EUNSUPPORTED, "cnx_ln_s2d: bad shape");
  const int segs = segs_for(Cp);
  const int64_t M = (int64_t)B * H * W;
  const dim3 grid((unsigned)((M + segs - 1) / segs)), block(segs * (Cp / 4));
  switch (prec) {
    case PREC_BF16: hipLaunchKernelGGL(cnx_ln_s2d_kernel<__bf16>, grid, block, 0, s, x, B, H, W, C, Cp, lnw, lnb, static_cast<__bf16*>(out)); break;
    case PREC_FP16: hipLaunchKernelGGL(cnx_ln_s2d_kernel<_Float16>, grid, block, 0, s, x, B, H, W, C, Cp, lnw, lnb, static_cast<_Float16*>(out)); break;
    case PREC_FP32: hipLaunchKernelGGL(cnx_ln_s2d_kernel<float>, grid, block, 0, s, x, B, H, W, C, Cp, lnw, lnb, static_cast<float*>(out)); break;
    default: return fail(EFFOCR_EINVAL, "cnx_ln_s2d: unknown precision");
  }
  return check_launch("cnx_ln_s2d");
}

int cnx_head(const float* x, int B, int HW, int C, int Cp, const float* lnw, const float* lnb, int l2norm, float* emb, int* status, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (Cp % 128 || Cp > 1024 || C > Cp || C % 4 || HW <= 0) return fail(EFFOCR_EUNSUPPORTED, "cnx_head: bad shape");
  hipLaunchKernelGGL(cnx_head_kernel, dim3((unsigned)B), dim3(Cp / 4), 0, s, x, HW, C, Cp, lnw, lnb, l2norm, emb, status);
  return check_launch("cnx_head");
}

}  // namespace effocr
