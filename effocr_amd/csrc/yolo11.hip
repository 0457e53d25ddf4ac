// The two kernels the YOLO11 localizer (yolo11_api.hip, libeffocr_yolo11.so) has of its own; everything else it runs is what the YOLOv8
// engine runs: resnet.hip's implicit-GEMM convolution, yolo.hip's upsample / max pool / im2col and yolov8.hip's stem and decode.
//   attention_nhwc   C2PSA's multi-head self-attention over the stride-32 map: softmax(32^-1/2 q k^T) v per (image, head), fp32 on the VALU
//   dwconv3x3_nhwc   depthwise 3x3 / stride 1 / pad 1 + folded-BN bias (+ SiLU) (+ a tensor added behind it) on channel-slice views
// Both are a small share of the network (about 1 % of yolo11n's FLOPs, 0.1 % of x's) and are written for exactness and a fixed summation
// order, not tuned: DESIGN.md section 3 "YOLO11".
#include "common.hpp"
#include "kernels.hpp"
#include <math.h>

namespace effocr {
namespace {

constexpr int AT_Q = 64;       // queries per workgroup: four lanes a query, each owns 16 of the 64 output dims and 16 of a tile's 64 keys
constexpr int AT_K = 64;       // keys per tile
constexpr int AT_KS = 36;      // floats per K row in LDS (32 + 4: the four keys a quad reads at once sit 36 floats apart, on different banks)
constexpr int AT_PS = 68;      // floats per row of the probability tile (64 + 4: 16 queries of a wave read 16 different bank groups)

// grid (query blocks of 64, heads, images), 256 threads.  Flash-attention form: K / V are walked in tiles of 64 keys through LDS (41 KB a
// workgroup whatever N is) with a running maximum m and sum l per query, so nothing grows with N^2 and an (image, head) pair is spread over
// ceil(N / 64) workgroups.  Lane (query ql = tid / 4, part = tid % 4):
//   scores   s_j = scale * sum_d q_d k_d for its keys j * 4 + part (j = 0..15), d ascending in one fmaf chain; keys past N get -inf
//   maximum  over its 16 scores, then over the quad (two xor shuffles): every lane of a quad holds the same tile maximum
//   p_j = expf(s_j - m_new) -> LDS; its 16 p summed j ascending, then over the quad; l = l * expf(m_old - m_new) + that
//   values   acc_d = acc_d * expf(m_old - m_new), then += p_key * v[key][d] for the tile's keys ascending, d = part * 16 .. + 15
// so the order of every sum of a query row is fixed by N and the tile size alone — not by the batch, the image's position or the query
// block.  The tail queries of the last block compute on a clamped row and store nothing; the tail keys are loaded clamped and weigh 0.
__global__ __launch_bounds__(256) void attention_kernel(const float* __restrict__ qkv, int qkv_ld, int qkv_off, float* __restrict__ out, int out_ld,
                                                        int out_off, int N) {
  __shared__ __attribute__((aligned(16))) float Ks[AT_K * AT_KS];
  __shared__ __attribute__((aligned(16))) float Vs[AT_K * 64];
  __shared__ __attribute__((aligned(16))) float Ps[AT_Q * AT_PS];
  const int tid = threadIdx.x, ql = tid >> 2, part = tid & 3;
  const int h = blockIdx.y;
  const int64_t row0 = (int64_t)blockIdx.z * N;
  const int n = blockIdx.x * AT_Q + ql, nq = min(n, N - 1);
  const float* base = qkv + row0 * qkv_ld + qkv_off + h * 128;
  const float scale = 0.17677669529663687f;                  // 32^-1/2 (key_dim 32)
  float q[32];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(base + (int64_t)nq * qkv_ld + 4 * c);
#pragma unroll
    for (int e = 0; e < 4; ++e) q[4 * c + e] = v[e];
  }
  float m = -INFINITY, l = 0.f, acc[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) acc[d] = 0.f;
  for (int k0 = 0; k0 < N; k0 += AT_K) {
    __syncthreads();                                         // the previous tile's reads are done
#pragma unroll
    for (int i = 0; i < 2; ++i) {                            // K tile: 64 keys x 8 float4
      const int idx = tid + 256 * i, key = idx >> 3, c = idx & 7;
      const int kk = min(k0 + key, N - 1);
      *reinterpret_cast<f32x4*>(Ks + key * AT_KS + 4 * c) = *reinterpret_cast<const f32x4*>(base + (int64_t)kk * qkv_ld + 32 + 4 * c);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {                            // V tile: 64 keys x 16 float4
      const int idx = tid + 256 * i, key = idx >> 4, c = idx & 15;
      const int kk = min(k0 + key, N - 1);
      *reinterpret_cast<f32x4*>(Vs + key * 64 + 4 * c) = *reinterpret_cast<const f32x4*>(base + (int64_t)kk * qkv_ld + 64 + 4 * c);
    }
    __syncthreads();
    float sc[16], tmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int key = 4 * j + part;
      const float* kr = Ks + key * AT_KS;
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const f32x4 kv = *reinterpret_cast<const f32x4*>(kr + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) dot = fmaf(q[4 * c + e], kv[e], dot);
      }
      sc[j] = (k0 + key < N) ? dot * scale : -INFINITY;
      tmax = fmaxf(tmax, sc[j]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 1, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 2, 64));
    const float mn = fmaxf(m, tmax);                         // finite: key k0 of every tile exists
    const float corr = expf(m - mn);                         // first tile: expf(-inf) = 0
    float psum = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float p = expf(sc[j] - mn);
      Ps[ql * AT_PS + 4 * j + part] = p;
      psum += p;
    }
    psum += __shfl_xor(psum, 1, 64);
    psum += __shfl_xor(psum, 2, 64);
    l = l * corr + psum;
    m = mn;
#pragma unroll
    for (int d = 0; d < 16; ++d) acc[d] *= corr;
    __syncthreads();                                         // the probability tile is complete
#pragma unroll 4
    for (int k4 = 0; k4 < AT_K; k4 += 4) {
      const f32x4 p4 = *reinterpret_cast<const f32x4*>(Ps + ql * AT_PS + k4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float* vr = Vs + (k4 + e) * 64 + part * 16;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const f32x4 vv = *reinterpret_cast<const f32x4*>(vr + 4 * c);
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[4 * c + u] = fmaf(p4[e], vv[u], acc[4 * c + u]);
        }
      }
    }
  }
  if (n < N) {
    float* o = out + (row0 + n) * out_ld + out_off + h * 64 + part * 16;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f32x4 r;
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = acc[4 * c + u] / l;
      *reinterpret_cast<f32x4*>(o + 4 * c) = r;
    }
  }
}

// One thread per (pixel, 4 channels): the 9 taps (ky, kx) ascending in one fmaf chain per channel (a tap outside the map is skipped, which
// is adding its exact zero), then + bias, x / (1 + expf(-x)) when silu, + add.  A pixel's value depends on its own window alone.
__global__ __launch_bounds__(256) void dwconv3x3_kernel(const float* __restrict__ in, int in_ld, int in_off, int icut, int istride, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int silu, const float* __restrict__ add, int add_ld, int add_off,
                                                        float* __restrict__ out, int out_ld, int out_off, int64_t npix, int H, int W, int C4) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= npix * C4) return;
  const int c = (int)(id % C4) * 4;
  const int64_t pix = id / C4;
  const int x = (int)(pix % W), y = (int)((pix / W) % H);
  const int cin = in_off + (icut ? c / icut * istride + c % icut : c);
  float wt[36];                                              // wt[i * 9 + tap]: channel c + i
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(w + (int64_t)c * 9 + 4 * t);
#pragma unroll
    for (int e = 0; e < 4; ++e) wt[4 * t + e] = v[e];
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int iy = y + ky - 1, ix = x + kx - 1;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      const f32x4 v = *reinterpret_cast<const f32x4*>(in + (pix + (int64_t)(ky - 1) * W + (kx - 1)) * in_ld + cin);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = fmaf(v[i], wt[i * 9 + ky * 3 + kx], acc[i]);
    }
  const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + c);
  f32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float t = acc[i] + bv[i];
    r[i] = silu ? t / (1.0f + expf(-t)) : t;
  }
  if (add) {
    const f32x4 av = *reinterpret_cast<const f32x4*>(add + pix * add_ld + add_off + c);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] += av[i];
  }
  *reinterpret_cast<f32x4*>(out + pix * out_ld + out_off + c) = r;
}

}  // namespace

int attention_nhwc(const float* qkv, int qkv_ld, int qkv_off, float* out, int out_ld, int out_off, int B, int N, int heads, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (!qkv || !out) return fail(EFFOCR_EINVAL, "attention_nhwc: NULL pointer");
  if (N < 1 || heads < 1 || qkv_off < 0 || out_off < 0 || qkv_ld % 4 || qkv_off % 4 || out_ld % 4 || out_off % 4 || qkv_off + heads * 128 > qkv_ld ||
      out_off + heads * 64 > out_ld)
    return fail(EFFOCR_EINVAL, "attention_nhwc: heads x 128 qkv channels and heads x 64 output channels must fit their rows, offsets multiples of 4");
  if (N > Y11_MAX_TOKENS) return fail(EFFOCR_EUNSUPPORTED, "attention_nhwc: more than " + std::to_string(Y11_MAX_TOKENS) + " tokens per image");
  if (B > 65535 || heads > 65535) return fail(EFFOCR_EUNSUPPORTED, "attention_nhwc: batch or heads above 65535");
  hipLaunchKernelGGL(attention_kernel, dim3((unsigned)((N + AT_Q - 1) / AT_Q), (unsigned)heads, (unsigned)B), dim3(256), 0, s, qkv, qkv_ld, qkv_off, out, out_ld,
                     out_off, N);
  return check_launch("attention_nhwc");
}

int dwconv3x3_nhwc(const float* in, int in_ld, int in_off, int icut, int istride, const float* w, const float* bias, int silu, const float* add, int add_ld,
                   int add_off, float* out, int out_ld, int out_off, int B, int H, int W, int C, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (!in || !w || !bias || !out) return fail(EFFOCR_EINVAL, "dwconv3x3_nhwc: NULL pointer");
  if (H < 1 || W < 1 || C < 4 || C % 4 || in_ld % 4 || in_off % 4 || out_ld % 4 || out_off % 4 || in_off < 0 || out_off < 0 || out_off + C > out_ld)
    return fail(EFFOCR_EINVAL, "dwconv3x3_nhwc: channel counts, row widths and offsets must be multiples of 4, the output slice inside its rows");
  if (icut ? (icut < 4 || icut % 4 || istride % 4 || istride < icut || C % icut || in_off + (C / icut - 1) * istride + icut > in_ld) : in_off + C > in_ld)
    return fail(EFFOCR_EINVAL, "dwconv3x3_nhwc: the input channels do not fit their rows");
  if (add && (add_ld % 4 || add_off % 4 || add_off < 0 || add_off + C > add_ld)) return fail(EFFOCR_EINVAL, "dwconv3x3_nhwc: the added tensor's slice does not fit its rows");
  const int64_t npix = (int64_t)B * H * W, threads = npix * (C / 4);
  if ((threads + 255) / 256 >= ((int64_t)1 << 31)) return fail(EFFOCR_EUNSUPPORTED, "dwconv3x3_nhwc: too many pixels");
  hipLaunchKernelGGL(dwconv3x3_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, in, in_ld, in_off, icut, istride, w, bias, silu, add, add_ld, add_off,
                     out, out_ld, out_off, npix, H, W, C / 4);
  return check_launch("dwconv3x3_nhwc");
}

}  // namespace effocr
