// BiT ResNetV2 (libeffocr_bit.so; DESIGN.md "BiT"): the three operators its forward needs beyond the convolutions of resnet16.hip /
// resnet.hip — GroupNorm + ReLU, the stem's zero pad + max pool, and the head (final GroupNorm + ReLU + global average pool).
//
// GroupNorm statistics cannot be folded into weights: they belong to one (crop, group).  They are computed in fp32 from deviations about a
// mean, never from E[x^2] - E[x]^2: a workgroup reduces one tile of pixels in two passes (tile mean, then squared deviations about it; the
// tile stays in registers) and writes (mean, M2, shift) per group; a small kernel merges a crop's tiles with Chan's formula in tile order; the
// apply kernel streams.
// Every value is taken relative to a shift, the group's first channel at the crop's first pixel (x - shift is exact or nearly so where the
// mean is many standard deviations from zero), so the rounding errors scale with the deviations and not with the mean.
// Tile size and reduction order follow from (HW, C) alone, so a crop's result is bitwise the same in every call size.
#include "common.hpp"
#include "kernels.hpp"
#include "bit.hpp"

namespace effocr {
namespace {

static_assert(BIT_GN_TILE == 8 * 256 * 8, "a GroupNorm tile is 8 pixels per thread: 256 threads x 8 channels x 8 steps");

template <typename T> struct V8of { typedef __attribute__((__vector_size__(8 * sizeof(T)))) T type; };

// Sum over one GroupNorm group of the per-thread, per-channel partials part[thread][8]: thread = pixel lane * CV + channel vector.  Group
// g = channels [g cpg, (g + 1) cpg): cpg x PS = 64 values, added in a fixed order by one thread.
__device__ __forceinline__ float gn_group_sum(const float* part, int g, int cpg, int CV, int PS) {
  float a = 0.f;
  for (int c = g * cpg; c < (g + 1) * cpg; ++c)
    for (int q = 0; q < PS; ++q) a += part[(q * CV + (c >> 3)) * 8 + (c & 7)];
  return a;
}

// One tile of TP pixels x C channels of crop blockIdx.y: per group (mean - shift, M2 = sum of squared deviations about that mean, shift)
// -> partial [b][tile][group][BIT_GN_REC].  256 threads: thread = (pixel lane, 8-channel vector), CV = C / 8 vectors per pixel, PS = 256 / CV pixel lanes.
template <typename T>
__global__ __launch_bounds__(256) void bit_gn_stats_kernel(const T* __restrict__ in, float* __restrict__ partial, int HW, int C, int TP, int ntiles) {
  typedef typename V8of<T>::type V8;
  __shared__ float part[256 * 8];
  __shared__ float mean_s[BIT_GROUPS];
  const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
  const int CV = C >> 3, PS = 256 / CV, cpg = C / BIT_GROUPS;
  const int cv = tid & (CV - 1), pl = tid / CV;
  const int p0 = tile * TP, p1 = min(p0 + TP, HW);
  const T* base = in + (int64_t)b * HW * C + cv * 8;
  float s[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    s[e] = 0.f;
    sh[e] = (float)in[(int64_t)b * HW * C + (cv * 8 + e) / cpg * cpg];
  }
  V8 v[8];                                                   // this thread's part of the tile: TP / PS = 8 pixels, kept for the second pass
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int p = p0 + pl + i * PS;
    if (p < p1) v[i] = *reinterpret_cast<const V8*>(base + (int64_t)p * C);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (p0 + pl + i * PS < p1) {
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += (float)v[i][e] - sh[e];
    }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[tid * 8 + e] = s[e];
  __syncthreads();
  const float n = (float)((p1 - p0) * cpg);
  if (tid < BIT_GROUPS) mean_s[tid] = gn_group_sum(part, tid, cpg, CV, PS) / n;
  __syncthreads();
  float m[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { m[e] = mean_s[(cv * 8 + e) / cpg]; s[e] = 0.f; }
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (p0 + pl + i * PS < p1) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = ((float)v[i][e] - sh[e]) - m[e]; s[e] += d * d; }
    }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[tid * 8 + e] = s[e];
  __syncthreads();
  if (tid < BIT_GROUPS) {
    float* o = partial + (((int64_t)b * ntiles + tile) * BIT_GROUPS + tid) * BIT_GN_REC;
    o[0] = mean_s[tid];
    o[1] = gn_group_sum(part, tid, cpg, CV, PS);
    o[2] = (float)in[(int64_t)b * HW * C + tid * cpg];         // the shift: the apply kernel may run in place and must not re-read it
  }
}

// A crop's group statistics from its tiles' (n, mean - shift, M2), merged by Chan's formula in tile order -> (mean - shift,
// 1 / sqrt(biased var + eps))
__device__ __forceinline__ void gn_merge(const float* __restrict__ partial, int g, int HW, int cpg, int TP, int ntiles, float& mean, float& rstd) {
  float n = 0.f, mu = 0.f, M2 = 0.f;
  for (int t = 0; t < ntiles; ++t) {
    const float nb = (float)((min((t + 1) * TP, HW) - t * TP) * cpg);
    const float mb = partial[(t * BIT_GROUPS + g) * BIT_GN_REC], M2b = partial[(t * BIT_GROUPS + g) * BIT_GN_REC + 1];
    const float nt = n + nb, d = mb - mu;
    mu += d * (nb / nt);
    M2 += M2b + d * d * (n * nb / nt);
    n = nt;
  }
  mean = mu;
  rstd = 1.0f / sqrtf(M2 / n + BIT_GN_EPS);
}

// One workgroup per crop, one thread per group: the merged (mean - shift, 1 / sigma) replace the first two values of the crop's FIRST tile
// record (thread g is the only reader of the records of group g), so that the apply kernel's workgroups start streaming at once instead
// of each repeating the merge.
__global__ __launch_bounds__(64) void bit_gn_merge_kernel(float* __restrict__ partial, int HW, int C, int TP, int ntiles) {
  const int g = threadIdx.x;
  if (g >= BIT_GROUPS) return;
  float* pb = partial + (int64_t)blockIdx.x * ntiles * BIT_GROUPS * BIT_GN_REC;
  float mean, rstd;
  gn_merge(pb, g, HW, C / BIT_GROUPS, TP, ntiles, mean, rstd);
  pb[g * BIT_GN_REC] = mean;
  pb[g * BIT_GN_REC + 1] = rstd;
}

// The same tile: out = relu(((x - shift) - (mean - shift)) * rstd * gamma + beta), rounded once to T (NaN-propagating, as torch's relu).  out may alias in.
template <typename T>
__global__ __launch_bounds__(256) void bit_gn_apply_kernel(const T* in, T* out, const float* __restrict__ partial, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int HW, int C, int TP, int ntiles) {
  typedef typename V8of<T>::type V8;
  __shared__ float mean_s[BIT_GROUPS], rstd_s[BIT_GROUPS], shift_s[BIT_GROUPS];
  const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
  const int CV = C >> 3, PS = 256 / CV, cpg = C / BIT_GROUPS;
  const int cv = tid & (CV - 1), pl = tid / CV;
  if (tid < BIT_GROUPS) {                                    // the crop's merged statistics (bit_gn_merge_kernel)
    const float* pb = partial + ((int64_t)b * ntiles * BIT_GROUPS + tid) * BIT_GN_REC;
    mean_s[tid] = pb[0]; rstd_s[tid] = pb[1]; shift_s[tid] = pb[2];
  }
  __syncthreads();
  float m[8], a[8], bt[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = cv * 8 + e, g = c / cpg;
    m[e] = mean_s[g];
    a[e] = rstd_s[g] * gamma[c];
    bt[e] = beta[c];
    sh[e] = shift_s[g];
  }
  const int p0 = tile * TP, p1 = min(p0 + TP, HW);
  const int64_t base = (int64_t)b * HW * C + cv * 8;
  for (int p = p0 + pl; p < p1; p += PS) {
    const V8 v = *reinterpret_cast<const V8*>(in + base + (int64_t)p * C);
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float y = fmaf(((float)v[e] - sh[e]) - m[e], a[e], bt[e]);
      o[e] = (T)(y < 0.f ? 0.f : y);
    }
    *reinterpret_cast<V8*>(out + base + (int64_t)p * C) = o;
  }
}

// max_pool2d(pad(in, 1, value 0), 3, 2) on NHWC, 8 channels per thread: a tap outside the image is a 0 that takes part in the maximum (the
// stem's output has negative values); the maximum is exact in any type and a NaN wins, as in torch's max_pool2d
template <typename T>
__global__ __launch_bounds__(256) void bit_stem_pool_kernel(const T* __restrict__ in, T* __restrict__ out, int B, int H, int W, int C, int OH, int OW) {
  typedef typename V8of<T>::type V8;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int C8 = C / 8;
  const int64_t total = (int64_t)B * OH * OW * C8;
  if (id >= total) return;
  const int c8 = (int)(id % C8);
  const int64_t p = id / C8;
  const int ox = (int)(p % OW), oy = (int)((p / OW) % OH);
  const int64_t b = p / ((int64_t)OW * OH);
  float m[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int iy = oy * 2 - 1 + ky, ix = ox * 2 - 1 + kx;
      const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
      V8 v = {};
      if (ok) v =*reinterpret_cast<const V8*>(in + ((b * H + iy) * W + ix) * C + c8 * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = ok ? (float)v[e] : 0.f;
        m[e] = (f > m[e] || f != f) ? f : m[e];
      }
    }
  V8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (T)m[e];
  *reinterpret_cast<V8*>(out + p * C + c8 * 8) = o;
}

// Head: one workgroup of 256 threads per crop, thread = C / 256 <= 8 consecutive channels, so a group is 8 consecutive threads.  Three
// passes over the crop's [HW][C] block, all fp32 and in pixel order: group means, squared deviations, then the per-channel mean of
// relu((x - mean) * rstd * gamma + beta); + F.normalize when l2norm.  A non-finite embedding ORs 1 into *status.
template <typename T>
__global__ __launch_bounds__(256) void bit_head_kernel(const T* __restrict__ in, float* __restrict__ emb, int HW, int C, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, int l2norm, int* __restrict__ status) {
  __shared__ float chs[256];
  __shared__ float mean_s[BIT_GROUPS], rstd_s[BIT_GROUPS];
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int per = C / 256;
  const T* xb = in + (int64_t)b * HW * C + tid * per;
  const float n = (float)HW * (float)(per * 8);
  const float shift = (float)in[(int64_t)b * HW * C + (tid >> 3) * 8 * per];   // the group's first channel at pixel 0 (see the top of the file)
  float s = 0.f;
  for (int p = 0; p < HW; ++p)
    for (int t = 0; t < per; ++t) s += (float)xb[(int64_t)p * C + t] - shift;
  chs[tid] = s;
  __syncthreads();
  if (tid < BIT_GROUPS) {
    float a = 0.f;
    for (int i = 0; i < 8; ++i) a += chs[tid * 8 + i];
    mean_s[tid] = a / n;
  }
  __syncthreads();
  const float mu = mean_s[tid >> 3];
  s = 0.f;
  for (int p = 0; p < HW; ++p)
    for (int t = 0; t < per; ++t) { const float d = ((float)xb[(int64_t)p * C + t] - shift) - mu; s += d * d; }
  chs[tid] = s;
  __syncthreads();
  if (tid < BIT_GROUPS) {
    float a = 0.f;
    for (int i = 0; i < 8; ++i) a += chs[tid * 8 + i];
    rstd_s[tid] = 1.0f / sqrtf(a / n + BIT_GN_EPS);
  }
  __syncthreads();
  const float rstd = rstd_s[tid >> 3];
  float v[8];
  float ss = 0.f;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    v[t] = 0.f;
    if (t < per) {
      const int c = tid * per + t;
      const float a = rstd * gamma[c], sh = beta[c];
      float acc = 0.f;
      for (int p = 0; p < HW; ++p) {
        const float y = fmaf(((float)xb[(int64_t)p * C + t] - shift) - mu, a, sh);
        acc += y < 0.f ? 0.f : y;                             // NaN-propagating
      }
      v[t] = acc / (float)HW;
      ss += v[t] * v[t];
    }
  }
  if (l2norm) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    const float nr = sqrtf(red[0] + red[1] + red[2] + red[3]);
    const float nrm = nr < 1e-12f ? 1e-12f : nr;             // F.normalize's clamp; a NaN norm stays NaN
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = v[t] / nrm;
  }
  bool bad = false;
#pragma unroll
  for (int t = 0; t < 8; ++t)
    if (t < per) {
      emb[(int64_t)b * C + tid * per + t] = v[t];
      bad |= !__builtin_isfinite(v[t]);
    }
  if (status && bad) atomicOr(status, 1);
}

template <typename T>
int launch_gn(const void* in, void* out, int B, int HW, int C, const float* gamma, const float* beta, float* partial, hipStream_t s) {
  const int TP = bit_gn_tile_pixels(C), nt = bit_gn_tiles(HW, C);
  const dim3 g((unsigned)nt, (unsigned)B);
  hipLaunchKernelGGL((bit_gn_stats_kernel<T>), g, dim3(256), 0, s, static_cast<const T*>(in), partial, HW, C, TP, nt);
  hipLaunchKernelGGL(bit_gn_merge_kernel, dim3((unsigned)B), dim3(64), 0, s, partial, HW, C, TP, nt);
  hipLaunchKernelGGL((bit_gn_apply_kernel<T>), g, dim3(256), 0, s, static_cast<const T*>(in), static_cast<T*>(out), partial, gamma, beta, HW, C, TP, nt);
  return check_launch("bit_groupnorm_relu");
}

template <typename T> int launch_pool(const void* in, void* out, int B, int H, int W, int C, int OH, int OW, int64_t total, hipStream_t s) {
  hipLaunchKernelGGL((bit_stem_pool_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, static_cast<const T*>(in), static_cast<T*>(out),
                     B, H, W, C, OH, OW);
  return check_launch("bit_stem_pool");
}

template <typename T>
int launch_head(const void* in, float* emb, int B, int HW, int C, const float* gamma, const float* beta, int l2norm, int* status, hipStream_t s) {
  hipLaunchKernelGGL((bit_head_kernel<T>), dim3((unsigned)B), dim3(256), 0, s, static_cast<const T*>(in), emb, HW, C, gamma, beta, l2norm, status);
  return check_launch("bit_head");
}

}  // namespace

int bit_groupnorm_relu(int prec, const void* in, void* out, int B, int HW, int C, const float* gamma, const float* beta, float* partial,
                       hipStream_t s) {
  if (B <= 0 || HW <= 0) return EFFOCR_OK;
  if (C < 64 || C > 2048 || (C & (C - 1))) return fail(EFFOCR_EUNSUPPORTED, "bit_groupnorm_relu: C must be a power of two from 64 to 2048");
  if (B > 65535) return fail(EFFOCR_EUNSUPPORTED, "bit_groupnorm_relu: more than 65535 crops in one launch (use a smaller chunk)");
  if ((int64_t)HW * C >= ((int64_t)1 << 31)) return fail(EFFOCR_EUNSUPPORTED, "bit_groupnorm_relu: a crop of 2^31 or more elements");
  if (prec == PREC_FP16) return launch_gn<_Float16>(in, out, B, HW, C, gamma, beta, partial, s);
  if (prec == PREC_BF16) return launch_gn<__bf16>(in, out, B, HW, C, gamma, beta, partial, s);
  return launch_gn<float>(in, out, B, HW, C, gamma, beta, partial, s);
}

int bit_stem_pool(int prec, const void* in, void* out, int B, int H, int W, int C, int OH, int OW, hipStream_t s) {
  if (C % 8) return fail(EFFOCR_EUNSUPPORTED, "bit_stem_pool: C must be a multiple of 8");
  const int64_t total = (int64_t)B * OH * OW * (C / 8);
  if (total <= 0) return EFFOCR_OK;
  if (total >= ((int64_t)1 << 39)) return fail(EFFOCR_EUNSUPPORTED, "bit_stem_pool: too many outputs for one launch (use a smaller chunk)");
  if (prec == PREC_FP16) return launch_pool<_Float16>(in, out, B, H, W, C, OH, OW, total, s);
  if (prec == PREC_BF16) return launch_pool<__bf16>(in, out, B, H, W, C, OH, OW, total, s);
  return launch_pool<float>(in, out, B, H, W, C, OH, OW, total, s);
}

int bit_head(int prec, const void* in, float* emb, int B, int HW, int C, const float* gamma, const float* beta, int l2norm, int* status,
             hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (HW <= 0) return fail(EFFOCR_EINVAL, "bit_head: no pixels");
  if (C % 256 || C > 2048) return fail(EFFOCR_EUNSUPPORTED, "bit_head: C must be a multiple of 256, at most 2048");
  if (prec == PREC_FP16) return launch_head<_Float16>(in, emb, B, HW, C, gamma, beta, l2norm, status, s);
  if (prec == PREC_BF16) return launch_head<__bf16>(in, emb, B, HW, C, gamma, beta, l2norm, status, s);
  return launch_head<float>(in, emb, B, HW, C, gamma, beta, l2norm, status, s);
}

}  // namespace effocr
