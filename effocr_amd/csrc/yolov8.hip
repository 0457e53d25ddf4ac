// The two kernels the YOLOv8 localizer (yolov8_api.hip, libeffocr_yolov8.so) has of its own; everything else it runs is the YOLOv5
// engine's: resnet.hip's implicit-GEMM convolution and yolo.hip's upsample / max pool / im2col.
//   stem3x3s2_nchw   model.0 = Conv(3, c, 3, 2): 27 taps straight from the NCHW input -> NHWC channel slice, bias + SiLU
//   yolov8_decode    Detect of one level: the 4 x 16-bin box distributions (DFL) -> distances -> (cx, cy, w, h) * stride, the constant
//                    objectness 1.0 and sigmoid class scores, written as the rows [B, total, 5 + nc] the YOLOv5 NMS kernels read
#include "common.hpp"
#include "kernels.hpp"
#include <math.h>

namespace effocr {
namespace {

// The scheme of yolo.hip's stem6x6s2_g16_kernel at 3x3 / stride 2 / pad 1: channel GROUPS of 16 (blockIdx.y) cover the five widths
// (16 / 32 / 48 / 64 / 80, stored with a channel stride padded to 32); a thread owns four horizontally adjacent pixels (OW % 4 == 0)
// x 16 channels (64 accumulators) and walks the 9 (ky, c) input rows of 9 columns, 3 taps each.  The weights come from the
// [tap (ky, kx, c)][wt_ld] transpose at a uniform address, so through the scalar cache.  Inputs as single floats, clamped and selected
// (no alignment or parity demand on x or W).  A group at or above `cout` is the zero padding the next layer's implicit GEMM reads: it
// skips the taps, and its zero bias gives SiLU(0) = 0.  Taps ascending (ky, c, kx) per output in one fmaf chain: a pixel's value depends on
// its own window alone.  The layer moves 12 B in and 4 * cout_st B out per pixel for 54 * cout flops: bound by its stores at every width.
__global__ __launch_bounds__(256) void stem3x3s2_g16_kernel(const float* __restrict__ x, const float* __restrict__ wt, int wt_ld, const float* __restrict__ bias,
                                                            float* __restrict__ out, int B, int H, int W, int OH, int OW, int out_ld, int out_off, int cout) {
  const int OW4 = OW >> 2;
  const int id = (int)blockIdx.x * 256 + (int)threadIdx.x;           // B * OH * OW / 4 < 2^31 (checked by the launcher)
  if (id >= B * OH * OW4) return;
  const int g0 = blockIdx.y * 16;
  const int ox = id % OW4 * 4, oy = id / OW4 % OH, b = id / (OW4 * OH);
  float acc[4][16];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int co = 0; co < 16; ++co) acc[p][co] = 0.f;
  if (g0 < cout) {
    const int ix0 = ox * 2 - 1;
#pragma unroll 1
    for (int r = 0; r < 9; ++r) {                            // (ky, c): one input row of 9 columns, its 3 taps unrolled
      const int ky = r / 3, c = r - 3 * ky, iy = oy * 2 - 1 + ky;
      const bool rowok = iy >= 0 && iy < H;
      const float* xr = x + ((int64_t)(b * 3 + c) * H + min(max(iy, 0), H - 1)) * W;
      float v[9];
#pragma unroll
      for (int j = 0; j < 9; ++j) {                          // the zero padding as a bit mask on a clamped (always valid) load
        const int ix = ix0 + j;
        const unsigned keep = (rowok && ix >= 0 && ix < W) ? ~0u : 0u;
        v[j] = __uint_as_float(__float_as_uint(xr[min(max(ix, 0), W - 1)]) & keep);
      }
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const float* wr = wt + (size_t)((ky * 3 + kx) * 3 + c) * wt_ld + g0;     // uniform address: scalar loads
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + 4 * q);
#pragma unroll
          for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[p][4 * q + e] = fmaf(v[kx + 2 * p], wv[e], acc[p][4 * q + e]);
        }
      }
    }
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    float* o = out + ((int64_t)(b * OH + oy) * OW + ox + p) * out_ld + out_off + g0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + g0 + 4 * q);
      f32x4 r;
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = silu_fast(acc[p][4 * q + e] + bv[e]);
      *reinterpret_cast<f32x4*>(o + 4 * q) = r;
    }
  }
}

__device__ __forceinline__ float sigmoid_f(float v) { return 1.0f / (1.0f + expf(-v)); }

// Four lanes per anchor point, lane j = side j (left, top, right, bottom): it reads the side's 16 logits (64 contiguous bytes), takes
// d_j = sum_k k e_k / sum_k e_k with e_k = exp(v_k - max v), both sums k ascending in fp32, and the four distances meet through
// ds_bpermute (__shfl) inside the aligned quad.  Lane 0 then writes cx and the constant objectness, lane 1 cy, lane 2 w, lane 3 h, and
// class score c is written by lane c % 4.  Nothing is reduced across anchor points: a row depends on its own pixel alone.
// grid covers B * ny * nx * 4 threads; the tail quads past the end compute on a clamped pixel and store nothing.
__global__ __launch_bounds__(256) void yolov8_decode_kernel(const float* __restrict__ box, int box_ld, const float* __restrict__ cls, int cls_ld,
                                                            float* __restrict__ pred, int B, int ny, int nx, int nc, float stride, int64_t total,
                                                            int64_t row0) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t npix = (int64_t)B * ny * nx;
  const int j = (int)(id & 3);
  const bool live = (id >> 2) < npix;
  const int64_t pix = live ? id >> 2 : npix - 1;
  const int px = (int)(pix % nx), py = (int)((pix / nx) % ny);
  const int64_t b = pix / ((int64_t)nx * ny);
  const float* v = box + pix * box_ld + 16 * j;
  float t[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(v + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) t[4 * q + e] = r[e];
  }
  float m = t[0];
#pragma unroll
  for (int k = 1; k < 16; ++k) m = fmaxf(m, t[k]);
  float den = 0.f, num = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const float e = expf(t[k] - m);
    den += e;
    num += (float)k * e;
  }
  const float d = num / den;
  const int lane = threadIdx.x & 63, q0 = lane & ~3;
  const float d0 = __shfl(d, q0, 64), d1 = __shfl(d, q0 + 1, 64), d2 = __shfl(d, q0 + 2, 64), d3 = __shfl(d, q0 + 3, 64);
  if (!live) return;
  const float ax = (float)px + 0.5f, ay = (float)py + 0.5f;
  const float x1 = ax - d0, y1 = ay - d1, x2 = ax + d2, y2 = ay + d3;
  const int no = nc + 5;
  float* o = pred + (b * total + row0 + (int64_t)py * nx + px) * no;
  o[j] = (j == 0 ? (x1 + x2) * 0.5f : j == 1 ? (y1 + y2) * 0.5f : j == 2 ? x2 - x1 : y2 - y1) * stride;
  if (j == 0) o[4] = 1.0f;
  const float* cv = cls + pix * cls_ld;
  for (int c = j; c < nc; c += 4) o[5 + c] = sigmoid_f(cv[c]);
}

}  // namespace

int stem3x3s2_nchw(const float* x, const float* wt, int wt_ld, const float* bias, float* out, int B, int H, int W, int OH, int OW, int out_ld, int out_off,
                   int cout, int cout_st, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (OW % 4 || cout_st % 16 || cout % 16 || cout > cout_st || wt_ld < cout_st || out_off % 4 || out_ld % 4 || out_off + cout_st > out_ld)
    return fail(EFFOCR_EUNSUPPORTED, "stem3x3s2: output width must be a multiple of 4, channel counts of 16, the slice inside its buffer");
  if (OH != (H - 1) / 2 + 1 || OW != (W - 1) / 2 + 1) return fail(EFFOCR_EINVAL, "stem3x3s2: output size is not ceil(input / 2)");
  const int64_t threads = (int64_t)B * OH * (OW / 4);
  if (threads >= ((int64_t)1 << 31) - 256 || (int64_t)B * 3 * H * W >= ((int64_t)1 << 31)) return fail(EFFOCR_EUNSUPPORTED, "stem3x3s2: batch too large for 32-bit pixel indices");
  hipLaunchKernelGGL(stem3x3s2_g16_kernel, dim3((unsigned)((threads + 255) / 256), (unsigned)(cout_st / 16)), dim3(256), 0, s, x, wt, wt_ld, bias, out, B, H, W,
                     OH, OW, out_ld, out_off, cout);
  return check_launch("stem3x3s2_nchw");
}

int yolov8_decode(const float* box, int box_ld, const float* cls, int cls_ld, float* pred, int B, int ny, int nx, int nc, float stride, int64_t total,
                  int64_t row0, hipStream_t s) {
  const int64_t npix = (int64_t)B * ny * nx;
  if (npix <= 0) return EFFOCR_OK;
  if (box_ld < 64 || box_ld % 4 || cls_ld < nc || nc < 1) return fail(EFFOCR_EINVAL, "yolov8_decode: box rows need 64 channels (a multiple of 4), class rows nc");
  if (row0 < 0 || row0 + (int64_t)ny * nx > total) return fail(EFFOCR_EINVAL, "yolov8_decode: the level's rows do not fit the prediction tensor");
  const int64_t blocks = (npix * 4 + 255) / 256;
  if (blocks >= ((int64_t)1 << 31)) return fail(EFFOCR_EUNSUPPORTED, "yolov8_decode: too many anchor points");
  hipLaunchKernelGGL(yolov8_decode_kernel, dim3((unsigned)blocks), dim3(256), 0, s, box, box_ld, cls, cls_ld, pred, B, ny, nx, nc, stride, total, row0);
  return check_launch("yolov8_decode");
}

}  // namespace effocr
