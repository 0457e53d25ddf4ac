// Swin-T encoder kernels on gfx950 (timm swin_tiny_patch4_window7_224 semantics; swin_api.hip: swin_forward).  Part of
// libeffocr_swin.so only.
//
// Layout: the residual stream is fp32, channels-last, [tokens][Cp] with Cp = the stage width rounded up to 128 (96 -> 128,
// 192 -> 256); tokens of a crop are row-major over its H x H map.  The pad channels hold zeros throughout: zero weights and biases
// fill them, and every LayerNorm here masks them out and writes zeros there.  The linears (qkv, proj, fc1, fc2, reduction) run on
// gemm_nt / gemm2_nt in the handle's precision.  LayerNorm eps is 1e-5 everywhere (nn.LayerNorm's default, what timm's Swin uses).
//
// Thread map of the per-token kernels (as convnext.hip): a SEGMENT of Cq = width / 4 threads owns whole tokens, thread t of a
// segment holds channels 4t .. 4t+3 (one float4).  Cq is a multiple of 32, so a LayerNorm statistic is reduced with xor-shuffles
// inside each 32-lane half, then the halves of a segment are summed through LDS in a fixed order.  No result depends on the batch
// size, the chunking or the launch geometry.
#include "common.hpp"
#include "kernels.hpp"
#include "swin.hpp"

namespace effocr {
namespace {

__device__ __forceinline__ float half_sum(float v) {      // sum over the 32-lane half of the wave (every lane gets it)
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// v summed over the segment of this thread.  hs: LDS [halves per block].  Two barriers: every thread of the block must call it.
__device__ __forceinline__ float seg_sum(float v, float* hs, int seg, int halves_per_seg) {
  v = half_sum(v);
  if ((threadIdx.x & 31) == 0) hs[threadIdx.x >> 5] = v;
  __syncthreads();
  float t = 0.f;
  for (int h = 0; h < halves_per_seg; ++h) t += hs[seg * halves_per_seg + h];
  __syncthreads();
  return t;
}

// two-pass LayerNorm of one token spread over a segment; real = this thread's channels are real, C = real channel count
__device__ __forceinline__ f32x4 seg_layernorm(f32x4 v, bool real, int C, int c4, const float* lnw, const float* lnb, float eps,
                                               float* hs, int seg, int hps) {
  const float invC = 1.0f / (float)C;
  const float mean = seg_sum(real ? (v[0] + v[1]) + (v[2] + v[3]) : 0.f, hs, seg, hps) * invC;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] -= mean;
  const float var = seg_sum(real ? (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]) : 0.f, hs, seg, hps) * invC;
  const float rstd = 1.0f / sqrtf(var + eps);
  f32x4 g = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
  if (real) { g = *reinterpret_cast<const f32x4*>(lnw + c4); b = *reinterpret_cast<const f32x4*>(lnb + c4); }
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = real ? v[e] * rstd * g[e] + b[e] : 0.f;
  return v;
}

template <typename TO> __device__ __forceinline__ void store4v(TO* p, f32x4 v) {
  if constexpr (sizeof(TO) == 4) *reinterpret_cast<f32x4*>(p) = v;
  else *reinterpret_cast<u32x2*>(p) = pack4<TO>(v[0], v[1], v[2], v[3]);
}

// 8 consecutive elements <-> fp32 (16-byte aligned for 16-bit types, 32-byte for fp32)
template <typename T> __device__ __forceinline__ void load8(const T* p, float (&f)[8]) {
  if constexpr (sizeof(T) == 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { f[e] = a[e]; f[4 + e] = b[e]; }
  } else {
    typedef __attribute__((__vector_size__(8 * sizeof(T)))) T V8;
    const V8 v = *reinterpret_cast<const V8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (float)v[e];
  }
}
template <typename T> __device__ __forceinline__ void store8(T* p, const float* f) {
  if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<f32x4*>(p) = f32x4{f[0], f[1], f[2], f[3]};
    *reinterpret_cast<f32x4*>(p + 4) = f32x4{f[4], f[5], f[6], f[7]};
  } else {
    typedef __attribute__((__vector_size__(8 * sizeof(T)))) T V8;
    V8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (T)f[e];
    *reinterpret_cast<V8*>(p) = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// patch_embed: Conv2d(3, C0, 4, stride 4) + bias + LayerNorm over C0, straight from the NCHW crops.  Block = 8 segments of 32
// threads (Cp = 128), one token per segment; the 48 input pixels of the block's 8 tokens are staged in LDS.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void swin_stem_kernel(const float* __restrict__ img, int B, int S, const float* __restrict__ wt,
                                                         const float* __restrict__ bias, const float* __restrict__ lnw,
                                                         const float* __restrict__ lnb, int C0, float eps, float* __restrict__ x) {
  __shared__ float px[8][48];
  __shared__ float hs[8];
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
  f32x4 v = *reinterpret_cast<const f32x4*>(bias + c4);
#pragma unroll 8
  for (int k = 0; k < 48; ++k) {
    const float a = px[seg][k];
    const f32x4 w = *reinterpret_cast<const f32x4*>(wt + k * 128 + c4);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaf(a, w[e], v[e]);
  }
  v = seg_layernorm(v, c4 < C0, C0, c4, lnw, lnb, eps, hs, seg, 1);
  if (m < M) *reinterpret_cast<f32x4*>(x + m * 128 + c4) = v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// LayerNorm of the residual rows -> the next linear's operand [M][Cp] in prec's type (pad channels written as 0).  One token per
// segment.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename TO>
__global__ __launch_bounds__(256) void swin_ln_kernel(const float* __restrict__ x, int64_t M, int C, int Cp, const float* __restrict__ lnw,
                                                       const float* __restrict__ lnb, float eps, TO* __restrict__ out) {
  __shared__ float hs[8];
  const int Cq = Cp >> 2, segs = blockDim.x / Cq, hps = Cq >> 5;
  const int seg = threadIdx.x / Cq, t = threadIdx.x - seg * Cq, c4 = 4 * t;
  const int64_t m = (int64_t)blockIdx.x * segs + seg;
  const int64_t mc = m < M ? m : M - 1;
  const bool real = c4 < C;
  f32x4 v = real ? *reinterpret_cast<const f32x4*>(x + mc * Cp + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
  v = seg_layernorm(v, real, C, c4, lnw, lnb, eps, hs, seg, hps);
  if (m < M) store4v<TO>(out + m * Cp + c4, v);
}

// ---------------------------------------------------------------------------------------------------------------------------
// patch merging: gather 2x2 in timm's channel order [x(2i,2j), x(2i+1,2j), x(2i,2j+1), x(2i+1,2j+1)] (row, column), THEN
// LayerNorm over the 4C channels -> the reduction GEMM's operand [B*(H/2)^2][4C].  One output token per segment of C threads
// (thread t holds concatenated channels 4t .. 4t+3: quadrant 4t / C, channel 4t % C of it).
// ---------------------------------------------------------------------------------------------------------------------------
template <typename TO>
__global__ __launch_bounds__(384) void swin_merge_kernel(const float* __restrict__ x, int B, int H, int C, int Cp, const float* __restrict__ lnw,
                                                          const float* __restrict__ lnb, float eps, TO* __restrict__ out) {
  __shared__ float hs[12];
  const int segs = blockDim.x / C, hps = C >> 5;
  const int seg = threadIdx.x / C, t = threadIdx.x - seg * C, c4 = 4 * t;
  const int Ho = H / 2;
  const int64_t M = (int64_t)B * Ho * Ho;
  const int64_t m = (int64_t)blockIdx.x * segs + seg;
  const int64_t mc = m < M ? m : M - 1;
  const int64_t b = mc / ((int64_t)Ho * Ho);
  const int p = (int)(mc - b * Ho * Ho), i = p / Ho, j = p - i * Ho;
  const int q = c4 / C, c = c4 - q * C, dy = q & 1, dx = q >> 1;
  f32x4 v = *reinterpret_cast<const f32x4*>(x + ((b * H + 2 * i + dy) * (int64_t)H + 2 * j + dx) * Cp + c);
  v = seg_layernorm(v, true, 4 * C, c4, lnw, lnb, eps, hs, seg, hps);
  if (m < M) store4v<TO>(out + m * 4 * C + c4, v);
}

// ---------------------------------------------------------------------------------------------------------------------------
// (shifted-)window attention of one (crop, window, head) per 64-lane workgroup; lane i < 49 owns query token i of the 7x7 window,
// lanes 49..63 only help stage K and V (the 49 -> 64 pad: their rows take part in no softmax and no store).
//   qkv  [tokens][3][Cp] in the operand type (q, k, v at column offsets 0, Cp, 2 Cp; head h = channels 32h .. 32h+31)
//   out  [tokens][Cp]    attention output in the operand type; the workgroups of head 0 also write the pad channels C .. Cp-1 as 0
// The cyclic roll (torch.roll by -shift before, +shift after) and the window partition / reverse are index arithmetic: window-local
// token p = (py, px) of window (wy, wx) sits at rolled (Y, X) = (7 wy + py, 7 wx + px), i.e. at the original token
// ((Y + shift) % H, (X + shift) % H) — both for the loads and for the store.  Scores in fp32:
//   s_ij = (q_i * 32^-0.5) . k_j + table[(py_i - py_j + 6) * 13 + (px_i - px_j + 6)][h]  (+ -100 if i, j lie in different regions)
// with the regions of timm's / HF's mask (per axis: [0, H-7), [H-7, H-shift), [H-shift, H) of the rolled coordinate), then a
// softmax over the 49 keys and P . V, every sum in ascending j / d order.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int WS = 7, WT = WS * WS, HD = 32, RPB = (2 * WS - 1) * (2 * WS - 1);

template <typename T>
__global__ __launch_bounds__(64) void swin_wattn_kernel(const T* __restrict__ qkv, int H, int C, int Cp, int heads, int shift,
                                                         const float* __restrict__ table, T* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float ks[WT][HD];
  __shared__ __attribute__((aligned(16))) float vs[WT][HD];
  __shared__ float tb[RPB];
  __shared__ int reg[WT];
  const int lane = threadIdx.x;
  const int nw = H / WS, nwin = nw * nw;
  const int64_t gid = blockIdx.x;
  const int h = (int)(gid % heads);
  const int64_t bw = gid / heads;
  const int w = (int)(bw % nwin);
  const int64_t b = bw / nwin;
  const int wy = w / nw, wx = w - wy * nw;
  auto token = [&](int p) -> int64_t {
    const int py = p / WS, px = p - py * WS;
    int y = WS * wy + py + shift, x = WS * wx + px + shift;
    y -= y >= H ? H : 0;
    x -= x >= H ? H : 0;
    return (b * H + y) * (int64_t)H + x;
  };
  const int64_t ld = 3 * (int64_t)Cp;
  // K and V rows of the window: 49 tokens x 4 chunks of 8 elements, each
  for (int idx = lane; idx < 2 * WT * 4; idx += 64) {
    const int which = idx >= WT * 4, r = idx - which * WT * 4, p = r >> 2, ch = r & 3;
    float f[8];
    load8<T>(qkv + token(p) * ld + (1 + which) * Cp + h * HD + ch * 8, f);
    float* dst = which ? &vs[p][ch * 8] : &ks[p][ch * 8];
#pragma unroll
    for (int e = 0; e < 8; ++e) dst[e] = f[e];
  }
  for (int r = lane; r < RPB; r += 64) tb[r] = table[r * heads + h];
  if (lane < WT) {
    const int py = lane / WS, px = lane - py * WS;
    const int Y = WS * wy + py, X = WS * wx + px;
    reg[lane] = shift ? ((Y >= H - WS) + (Y >= H - shift)) * 3 + (X >= H - WS) + (X >= H - shift) : 0;
  }
  const bool live = lane < WT;
  const int i = live ? lane : 0;
  const int64_t ti = token(i);
  float q[HD];
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    float f[8];
    load8<T>(qkv + ti * ld + h * HD + ch * 8, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) q[ch * 8 + e] = f[e] * 0.17677669529663687f;   // 32^-0.5
  }
  __syncthreads();
  const int pyi = i / WS, pxi = i - pyi * WS, ri = reg[i];
  float s[WT];
  float mx = -3.0e38f;
#pragma unroll
  for (int j = 0; j < WT; ++j) {
    float a = 0.f;
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
      const f32x4 k4 = *reinterpret_cast<const f32x4*>(&ks[j][d]);
      a = fmaf(q[d], k4[0], a); a = fmaf(q[d + 1], k4[1], a); a = fmaf(q[d + 2], k4[2], a); a = fmaf(q[d + 3], k4[3], a);
    }
    const int pyj = j / WS, pxj = j - pyj * WS;
    a += tb[(pyi - pyj + WS - 1) * (2 * WS - 1) + (pxi - pxj + WS - 1)];
    if (reg[j] != ri) a += -100.0f;
    s[j] = a;
    mx = fmaxf(mx, a);
  }
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < WT; ++j) { s[j] = __expf(s[j] - mx); sum += s[j]; }
  const float inv = 1.0f / sum;
  float o[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) o[d] = 0.f;
#pragma unroll
  for (int j = 0; j < WT; ++j) {
    const float pj = s[j] * inv;
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
      const f32x4 v4 = *reinterpret_cast<const f32x4*>(&vs[j][d]);
      o[d] = fmaf(pj, v4[0], o[d]); o[d + 1] = fmaf(pj, v4[1], o[d + 1]); o[d + 2] = fmaf(pj, v4[2], o[d + 2]); o[d + 3] = fmaf(pj, v4[3], o[d + 3]);
    }
  }
  if (!live) return;
  T* orow = out + ti * Cp;
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) store8<T>(orow + h * HD + ch * 8, &o[ch * 8]);
  if (h == 0) {
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = C; c < Cp; c += 8) store8<T>(orow + c, z);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// head: final LayerNorm of every token, then the mean over the HW tokens (LN before pool), (+ F.normalize) -> emb.  One crop per
// workgroup of C / 4 threads; the tokens are summed in order.  A non-finite embedding ORs 1 into the workspace status word.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void swin_head_kernel(const float* __restrict__ x, int HW, int C, int Cp, const float* __restrict__ lnw,
                                                         const float* __restrict__ lnb, float eps, int l2norm, float* __restrict__ emb,
                                                         int* __restrict__ status) {
  __shared__ float hs[8];
  const int t = threadIdx.x, c4 = 4 * t, hps = blockDim.x >> 5;
  const int64_t b = blockIdx.x;
  const bool real = c4 < C;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < HW; ++i) {
    f32x4 v = real ? *reinterpret_cast<const f32x4*>(x + (b * HW + i) * (int64_t)Cp + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
    v = seg_layernorm(v, real, C, c4, lnw, lnb, eps, hs, 0, hps);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += v[e];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] /= (float)HW;
  if (l2norm) {
    const float ss = seg_sum(real ? (acc[0] * acc[0] + acc[1] * acc[1]) + (acc[2] * acc[2] + acc[3] * acc[3]) : 0.f, hs, 0, hps);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);           // F.normalize: x / max(||x||, eps)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = acc[e] / nrm;
  }
  if (!real) return;
  bool bad = false;
#pragma unroll
  for (int e = 0; e < 4; ++e) bad |= !(fabsf(acc[e]) <= 3.0e38f);
  *reinterpret_cast<f32x4*>(emb + b * C + c4) = acc;
  if (status && bad) atomicOr(status, 1);
}

}  // namespace

int swin_stem(const float* img, int B, int S, const float* wt, const float* bias, const float* lnw, const float* lnb, int C0, float eps,
              float* x, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (S % 4 || C0 > 128 || C0 % 4) return fail(EFFOCR_EUNSUPPORTED, "swin_stem: S % 4 == 0 and C0 <= 128 required");
  const int64_t M = (int64_t)B * (S / 4) * (S / 4);
  hipLaunchKernelGGL(swin_stem_kernel, dim3((unsigned)((M + 7) / 8)), dim3(256), 0, s, img, B, S, wt, bias, lnw, lnb, C0, eps, x);
  return check_launch("swin_stem");
}

int swin_layernorm(int prec, const float* x, int64_t M, int C, int Cp, const float* lnw, const float* lnb, float eps, void* out, hipStream_t s) {
  if (M <= 0) return EFFOCR_OK;
  if (Cp % 128 || Cp > 1024 || C > Cp || C % 4) return fail(EFFOCR_EUNSUPPORTED, "swin_layernorm: Cp must be a multiple of 128 (<= 1024)");
  const int segs = Cp >= 1024 ? 1 : 256 / (Cp / 4);
  const dim3 grid((unsigned)((M + segs - 1) / segs)), block(segs * (Cp / 4));
  switch (prec) {
    case PREC_BF16: hipLaunchKernelGGL(swin_ln_kernel<__bf16>, grid, block, 0, s, x, M, C, Cp, lnw, lnb, eps, static_cast<__bf16*>(out)); break;
    case PREC_FP16: hipLaunchKernelGGL(swin_ln_kernel<_Float16>, grid, block, 0, s, x, M, C, Cp, lnw, lnb, eps, static_cast<_Float16*>(out)); break;
    case PREC_FP32: hipLaunchKernelGGL(swin_ln_kernel<float>, grid, block, 0, s, x, M, C, Cp, lnw, lnb, eps, static_cast<float*>(out)); break;
    default: return fail(EFFOCR_EINVAL, "swin_layernorm: unknown precision");
  }
  return check_launch("swin_layernorm");
}

int swin_merge(int prec, const float* x, int B, int H, int C, int Cp, const float* lnw, const float* lnb, float eps, void* out, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (C % 32 || C > 384 || C > Cp || Cp % 4 || H % 2) return fail(EFFOCR_EUNSUPPORTED, "swin_merge: C must be a multiple of 32 (<= 384), H even");
  const int segs = C >= 256 ? 1 : 256 / C;
  const int64_t M = (int64_t)B * (H / 2) * (H / 2);
  const dim3 grid((unsigned)((M + segs - 1) / segs)), block(segs * C);
  switch (prec) {
    case PREC_BF16: hipLaunchKernelGGL(swin_merge_kernel<__bf16>, grid, block, 0, s, x, B, H, C, Cp, lnw, lnb, eps, static_cast<__bf16*>(out)); break;
    case PREC_FP16: hipLaunchKernelGGL(swin_merge_kernel<_Float16>, grid, block, 0, s, x, B, H, C, Cp, lnw, lnb, eps, static_cast<_Float16*>(out)); break;
    case PREC_FP32: hipLaunchKernelGGL(swin_merge_kernel<float>, grid, block, 0, s, x, B, H, C, Cp, lnw, lnb, eps, static_cast<float*>(out)); break;
    default: return fail(EFFOCR_EINVAL, "swin_merge: unknown precision");
  }
  return check_launch("swin_merge");
}

int swin_window_attention(int prec, const void* qkv, int B, int H, int C, int Cp, int shift, const float* table, void* out, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (H % WS || C % HD || C > Cp || Cp % 8 || shift < 0 || shift >= WS || (shift && H <= WS))
    return fail(EFFOCR_EUNSUPPORTED, "swin_window_attention: H % 7 == 0, C % 32 == 0, 0 <= shift < 7 (0 for one window) required");
  const int heads = C / HD;
  const int64_t nblk = (int64_t)B * (H / WS) * (H / WS) * heads;
  const dim3 grid((unsigned)nblk), block(64);
  switch (prec) {
    case PREC_BF16: hipLaunchKernelGGL(swin_wattn_kernel<__bf16>, grid, block, 0, s, static_cast<const __bf16*>(qkv), H, C, Cp, heads, shift, table, static_cast<__bf16*>(out)); break;
    case PREC_FP16: hipLaunchKernelGGL(swin_wattn_kernel<_Float16>, grid, block, 0, s, static_cast<const _Float16*>(qkv), H, C, Cp, heads, shift, table, static_cast<_Float16*>(out)); break;
    case PREC_FP32: hipLaunchKernelGGL(swin_wattn_kernel<float>, grid, block, 0, s, static_cast<const float*>(qkv), H, C, Cp, heads, shift, table, static_cast<float*>(out)); break;
    default: return fail(EFFOCR_EINVAL, "swin_window_attention: unknown precision");
  }
  return check_launch("swin_window_attention");
}

int swin_head(const float* x, int B, int HW, int C, int Cp, const float* lnw, const float* lnb, float eps, int l2norm, float* emb, int* status,
              hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (C % 128 || C > 1024 || C > Cp || Cp % 4 || HW <= 0) return fail(EFFOCR_EUNSUPPORTED, "swin_head: bad shape");
  hipLaunchKernelGGL(swin_head_kernel, dim3((unsigned)B), dim3(C / 4), 0, s, x, HW, C, Cp, lnw, lnb, eps, l2norm, emb, status);
  return check_launch("swin_head");
}

}  // namespace effocr
