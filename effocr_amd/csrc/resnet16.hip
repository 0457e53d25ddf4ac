// ResNet-34 / ResNet-50 16-bit path (libeffocr_resnet.so; DESIGN.md "ResNet-34 / ResNet-50").
//
// Activations are NHWC in the operand type (f16 or bf16) between layers.  A convolution is an implicit GEMM on
// v_mfma_f32_32x32x16_{f16,bf16}: rows = output pixels (b, oy, ox), columns = output channels, K = (ky, kx, ci) with ci fastest.
// Every layer this path runs has Cin % 64 == 0 (the stem goes through a 192-column im2col first), so one 128-byte K-stage of a row is 64
// contiguous input channels of ONE tap and the im2col gather is the stage loader itself (zero-filled taps outside the image).  BN is
// folded into the weights on the host; the epilogue adds the bias, the optional residual, applies ReLU and rounds once to the operand
// type.  K is reduced by one workgroup in stage order (no split-K): an output pixel's value does not depend on the number of crops.
#include "common.hpp"
#include "kernels.hpp"
#include "resnet16.hpp"
#include "tile128.hpp"

namespace effocr {
namespace {

using namespace tile128;

// 4 values of T as one vector (the 8-byte loads and stores of the epilogue)
template <typename T> struct V4of { typedef __attribute__((__vector_size__(4 * sizeof(T)))) T type; };

// one K-stage of MFMAs for a wave's NI x 2 sub-tiles (32 channels x 32 pixels each), weights and pixels in LDS rows of 64 values
template <typename T, int NI>
__device__ __forceinline__ void rn_stage_mma(f32x16 (&acc)[NI][2], const char* sW, const char* sX, int wrow0, int xrow0, int lane) {
  typedef typename Op16<T>::V8 V8;
  const int r31 = lane & 31, half = lane >> 5;
  const char* pw = sW + (wrow0 + r31) * ROWS;
  const char* px = sX + (xrow0 + r31) * ROWS;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    V8 a[NI], b[2];
#pragma unroll
    for (int i = 0; i < NI; ++i) a[i] = *reinterpret_cast<const V8*>(pw + i * 32 * ROWS + (2 * ks + half) * 16);
#pragma unroll
    for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const V8*>(px + j * 32 * ROWS + (2 * ks + half) * 16);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = Op16<T>::mfma(a[i], b[j], acc[i][j]);
  }
}

// NW = channel tile: 128 (2 x 2 waves of 64 channels x 64 pixels) or 64 (2 x 2 waves of 32 x 64), chosen by Cout alone.
// Tile = 128 pixels x NW channels; a stage = [NW weight rows | 128 pixel rows] of 144 bytes, double buffered (73.7 / 55.3 KB).
template <typename T, int NW>
__global__ __launch_bounds__(256, 2) void rn_conv16_kernel(Conv16Args a) {
  constexpr int NI = NW / 64;
  constexpr int WTB = NW * ROWS, STB = WTB + TILEB;
  __shared__ __attribute__((aligned(16))) char smem[2 * STB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id(), wn = w >> 1, wm = w & 1;
  const int M = a.B * a.OH * a.OW;
  const int K = a.KH * a.KW * a.Cin;
  const int nks = K / 64;
  const int ntn = a.Cout / NW;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (bid / ntn) * BM, n0 = (bid % ntn) * NW;
  const int wrow0 = wn * (NW / 2), xrow0 = wm * 64;
  const T* in = reinterpret_cast<const T*>(a.in);

  // this thread's 4 pixel rows: top-left input coordinate of the window and the element index of (b, iy0, ix0, 8 c)
  int iy0[4], ix0[4], base[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int m = m0 + (tid >> 3) + 32 * i;
    m = m < M ? m : M - 1;                                   // clamp: rows past M are never stored
    const int ox = m % a.OW, t = m / a.OW;
    const int oy = t % a.OH, b = t / a.OH;
    iy0[i] = oy * a.stride - a.pad;
    ix0[i] = ox * a.stride - a.pad;
    base[i] = ((b * a.H + iy0[i]) * a.W + ix0[i]) * a.Cin + (tid & 7) * 8;   // < 2^31 elements: rn_conv16 checks
  }
  unsigned woff[NI * 2];                                     // byte offsets of this thread's weight rows (< 4 GB: checked)
#pragma unroll
  for (int i = 0; i < NI * 2; ++i) woff[i] = (unsigned)(n0 + (tid >> 3) + 32 * i) * (unsigned)(K * 2) + (tid & 7) * 16;

  f32x16 acc[NI][2];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  u32x4 rw[NI * 2], rx[4];
  int ky = 0, kx = 0, ci0 = 0;                               // tap and first channel of the stage being loaded
  auto load_stage = [&](int ks) __attribute__((always_inline)) {
    const char* wb = reinterpret_cast<const char*>(a.w) + (int64_t)ks * ROWB;
#pragma unroll
    for (int i = 0; i < NI * 2; ++i) rw[i] = *reinterpret_cast<const u32x4*>(wb + woff[i]);
    const int off = (ky * a.W + kx) * a.Cin + ci0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = (unsigned)(iy0[i] + ky) < (unsigned)a.H && (unsigned)(ix0[i] + kx) < (unsigned)a.W;
      const u32x4 v = *reinterpret_cast<const u32x4*>(in + (ok ? base[i] + off : 0));
      rx[i] = ok ? v : u32x4{0u, 0u, 0u, 0u};
    }
    ci0 += 64;                                               // advance to the next stage's tap
    const bool wc = ci0 >= a.Cin;
    ci0 = wc ? 0 : ci0;
    kx += wc ? 1 : 0;
    const bool wx = kx >= a.KW;
    kx = wx ? 0 : kx;
    ky += wx ? 1 : 0;
  };
  auto store_stage = [&](char* st) __attribute__((always_inline)) {
    const int c = tid & 7;
#pragma unroll
    for (int i = 0; i < NI * 2; ++i) *reinterpret_cast<u32x4*>(st + ((tid >> 3) + 32 * i) * ROWS + c * 16) = rw[i];
    stage_store<T>(rx, st + WTB, tid);
  };

  load_stage(0);
  store_stage(smem);
  __syncthreads();
  for (int ks = 0; ks < nks; ++ks) {
    char* cur = smem + (ks & 1) * STB;
    char* nxt = smem + ((ks & 1) ^ 1) * STB;
    const bool more = ks + 1 < nks;
    if (more) load_stage(ks + 1);
    rn_stage_mma<T, NI>(acc, cur, cur + WTB, wrow0, xrow0, lane);
    if (more) store_stage(nxt);
    __syncthreads();
  }

  // epilogue: bias in the MFMA result layout, tile to LDS as fp32 [pixel][NW + 4], then whole pixel rows: residual, ReLU, one rounding
  constexpr int TS = NW + 4;
  static_assert(128 * TS * 4 <= 2 * STB, "rn_conv16: the output tile must fit the stage buffers");
  float* tile = reinterpret_cast<float*>(smem);
  const int half = lane >> 5;
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int nl = wrow0 + i * 32 + 8 * q + 4 * half;
      const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + n0 + nl);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        f32x4 v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
        v += bv;
        *reinterpret_cast<f32x4*>(tile + (xrow0 + j * 32 + (lane & 31)) * TS + nl) = v;
      }
    }
  __syncthreads();
  typedef typename V4of<T>::type T4;
  const T* resid = reinterpret_cast<const T*>(a.resid);
  T* out = reinterpret_cast<T*>(a.out);
  constexpr int C4 = NW / 4;                                 // 4-channel pieces per pixel row
#pragma unroll
  for (int it = 0; it < 128 * C4 / 256; ++it) {
    const int idx = it * 256 + tid, p = idx / C4, c4 = idx - p * C4;
    const int m = m0 + p;
    if (m >= M) continue;
    const int64_t o = (int64_t)m * a.Cout + n0 + c4 * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(tile + p * TS + c4 * 4);
    if (resid) {
      const T4 r = *reinterpret_cast<const T4*>(resid + o);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += (float)r[e];
    }
    if (a.relu) {                                            // NaN-propagating, as torch's relu: a non-finite value reaches the status word
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.f ? 0.f : v[e];
    }
    T4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = (T)v[e];
    *reinterpret_cast<T4*>(out + o) = h;
  }
}

// stem im2col: col[(b,oy,ox)][(ky*7+kx)*3 + c] = x[b][c][2oy-3+ky][2ox-3+kx] in T (0 outside the image and for k >= 147); one thread per
// 8 consecutive columns of a row (one 16-byte store), 32-bit indices (rn_im2col16 checks), divisions by constants only
template <typename T>
__global__ __launch_bounds__(256) void rn_im2col16_kernel(const float* __restrict__ x, T* __restrict__ col, int M, int H, int W, int OH, int OW) {
  typedef typename Op16<T>::V8 V8;
  constexpr int CH = RN_STEM_K16 / 8;
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= M * CH) return;
  const int m = id / CH, k0 = (id - m * CH) * 8;
  const int ox = m % OW, t = m / OW;
  const int oy = t % OH, b = t / OH;
  const float* xb = x + (int64_t)b * 3 * H * W;
  V8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = k0 + e;
    const int c = k % 3, tap = k / 3, kx = tap % 7, ky = tap / 7;
    const int iy = oy * 2 - 3 + ky, ix = ox * 2 - 3 + kx;
    const bool ok = k < 147 && iy >= 0 && iy < H && ix >= 0 && ix < W;
    o[e] = (T)(ok ? xb[(c * H + iy) * W + ix] : 0.f);
  }
  *reinterpret_cast<V8*>(col + (int64_t)id * 8) = o;
}

// max_pool2d(3, 2, 1) on 16-bit NHWC, 8 channels per thread (max is exact in any type; padding never wins; a NaN wins)
template <typename T>
__global__ __launch_bounds__(256) void rn_maxpool16_kernel(const T* __restrict__ in, T* __restrict__ out, int B, int H, int W, int C, int OH, int OW) {
  typedef typename Op16<T>::V8 V8;
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
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
        const V8 v = *reinterpret_cast<const V8*>(in + ((b * H + iy) * W + ix) * C + c8 * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {                      // NaN-propagating, as torch's max_pool2d
          const float f = (float)v[e];
          m[e] = (f > m[e] || f != f) ? f : m[e];
        }
      }
    }
  V8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (T)m[e];
  *reinterpret_cast<V8*>(out + p * C + c8 * 8) = o;
}

// global average pool over HW in fp32 (pixels summed in order) -> emb [B][C] fp32, + F.normalize when l2norm; one workgroup of 256
// threads per crop, C / 256 <= 8 channels per thread.  A non-finite embedding ORs 1 into *status.
template <typename T>
__global__ __launch_bounds__(256) void rn_avgpool_kernel(const T* __restrict__ in, float* __restrict__ emb, int HW, int C, int l2norm,
                                                         int* __restrict__ status) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int per = C / 256;                                   // 2 (C = 512) or 8 (C = 2048)
  float v[8];
  float ss = 0.f;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    v[t] = 0.f;
    if (t < per) {
      const int c = tid * per + t;
      float s = 0.f;
      for (int p = 0; p < HW; ++p) s += (float)in[((int64_t)b * HW + p) * C + c];
      v[t] = s / (float)HW;
      ss += v[t] * v[t];
    }
  }
  if (l2norm) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    const float nr = sqrtf(red[0] + red[1] + red[2] + red[3]);
    const float nrm = nr < 1e-12f ? 1e-12f : nr;             // F.normalize's clamp; a NaN norm stays NaN, as torch's clamp_min
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

template <typename T> int launch_conv16(const Conv16Args& a, hipStream_t s) {
  const int64_t M = (int64_t)a.B * a.OH * a.OW;
  const int nw = a.Cout % 128 == 0 ? 128 : 64;
  const int64_t grid = ((M + BM - 1) / BM) * (a.Cout / nw);
  if (nw == 128) hipLaunchKernelGGL((rn_conv16_kernel<T, 128>), dim3((unsigned)grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((rn_conv16_kernel<T, 64>), dim3((unsigned)grid), dim3(256), 0, s, a);
  return check_launch("rn_conv16");
}

}  // namespace

int rn_conv16(int prec, const Conv16Args& a, hipStream_t s) {
  const int64_t M = (int64_t)a.B * a.OH * a.OW;
  if (M <= 0) return EFFOCR_OK;
  if (a.Cin % 64 != 0 || a.Cout % 64 != 0) return fail(EFFOCR_EUNSUPPORTED, "rn_conv16: Cin and Cout must be multiples of 64");
  if ((int64_t)a.B * a.H * a.W * a.Cin >= ((int64_t)1 << 31) || M * a.Cout >= ((int64_t)1 << 31))
    return fail(EFFOCR_EUNSUPPORTED, "rn_conv16: activations of 2^31 or more elements (use a smaller chunk)");
  if ((int64_t)a.Cout * a.KH * a.KW * a.Cin * 2 >= ((int64_t)1 << 32)) return fail(EFFOCR_EUNSUPPORTED, "rn_conv16: weights of 4 GB or more");
  return prec == PREC_FP16 ? launch_conv16<_Float16>(a, s) : launch_conv16<__bf16>(a, s);
}

int rn_im2col16(int prec, const float* x, void* col, int B, int H, int W, int OH, int OW, hipStream_t s) {
  const int64_t M = (int64_t)B * OH * OW;
  if (M <= 0) return EFFOCR_OK;
  if (M * RN_STEM_K16 >= ((int64_t)1 << 31) || (int64_t)B * 3 * H * W >= ((int64_t)1 << 31))
    return fail(EFFOCR_EUNSUPPORTED, "rn_im2col16: 2^31 or more elements (use a smaller chunk)");
  const dim3 g((unsigned)((M * (RN_STEM_K16 / 8) + 255) / 256));
  if (prec == PREC_FP16) hipLaunchKernelGGL((rn_im2col16_kernel<_Float16>), g, dim3(256), 0, s, x, static_cast<_Float16*>(col), (int)M, H, W, OH, OW);
  else hipLaunchKernelGGL((rn_im2col16_kernel<__bf16>), g, dim3(256), 0, s, x, static_cast<__bf16*>(col), (int)M, H, W, OH, OW);
  return check_launch("rn_im2col16");
}

int rn_maxpool16(int prec, const void* in, void* out, int B, int H, int W, int C, int OH, int OW, hipStream_t s) {
  if (C % 8) return fail(EFFOCR_EUNSUPPORTED, "rn_maxpool16: C must be a multiple of 8");
  const int64_t total = (int64_t)B * OH * OW * (C / 8);
  if (total <= 0) return EFFOCR_OK;
  const dim3 g((unsigned)((total + 255) / 256));
  if (prec == PREC_FP16)
    hipLaunchKernelGGL((rn_maxpool16_kernel<_Float16>), g, dim3(256), 0, s, static_cast<const _Float16*>(in), static_cast<_Float16*>(out), B, H, W, C, OH, OW);
  else hipLaunchKernelGGL((rn_maxpool16_kernel<__bf16>), g, dim3(256), 0, s, static_cast<const __bf16*>(in), static_cast<__bf16*>(out), B, H, W, C, OH, OW);
  return check_launch("rn_maxpool16");
}

int rn_avgpool(int prec, const void* in, float* emb, int B, int HW, int C, int l2norm, int* status, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (C % 256 || C > 2048) return fail(EFFOCR_EUNSUPPORTED, "rn_avgpool: C must be a multiple of 256, at most 2048");
  const dim3 g((unsigned)B);
  if (prec == PREC_FP16) hipLaunchKernelGGL((rn_avgpool_kernel<_Float16>), g, dim3(256), 0, s, static_cast<const _Float16*>(in), emb, HW, C, l2norm, status);
  else if (prec == PREC_BF16) hipLaunchKernelGGL((rn_avgpool_kernel<__bf16>), g, dim3(256), 0, s, static_cast<const __bf16*>(in), emb, HW, C, l2norm, status);
  else hipLaunchKernelGGL((rn_avgpool_kernel<float>), g, dim3(256), 0, s, static_cast<const float*>(in), emb, HW, C, l2norm, status);
  return check_launch("rn_avgpool");
}

}  // namespace effocr
