// libeffocr_head.so: the FFNN classifier head (include/effocr_head.h) — logits = emb @ W^T + b in exact fp32 on
// v_mfma_f32_16x16x4_f32, with torch.argmax(-1) fused behind it.  Its own library: libeffocr_hip.so is at its size cap.
//
// Tiling.  A workgroup is 4 waves; a wave owns CT tiles of 16 classes and RT tiles of 16 rows (batch), so a workgroup covers
// 16*RT rows x 64*CT classes and every (row, class) is computed by exactly one wave over the whole of k (no split-K).  Each lane
// loads float4s of both operands straight from global memory: lane l holds row/class (l & 15) at k = kb + 4*(l >> 4) .. +3, and the
// four MFMAs of a 16-wide k-block take component t of those float4s — the fixed k order of effocr_head.h.  Out-of-range rows and
// classes are clamped on load and masked on store, so no access leaves [0, batch) x [0, n_classes).
//   batch <= 16 / 32 / 64: RT = 1 / 2 / 4, CT = 1 — one row block, W streams from HBM exactly once over 64-class workgroups that
//                          cover every CU (30 813 classes: 482 workgroups);
//   batch > 64:            RT = 4, CT = 2 — 64 x 128 tiles; the row block is the fastest grid index, so the workgroups that share a
//                          W tile run together and W comes from HBM once, the embeddings from L2.
// Argmax.  Every (row, class) gives a 64-bit key: high half the order-preserving bits of the logit (+0 for -0, NaN above +inf),
// low half ~class.  max() of keys = torch.argmax (first index of the maximum, first NaN).  A workgroup reduces its 64*CT classes
// (shuffles, then LDS across the 4 waves) and writes one key per row; with one class block that key is the answer, otherwise a
// second kernel takes the max over the class blocks.  max is order-independent: ids are deterministic.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/effocr_head.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxD = 4096;
constexpr int64_t kMaxBatch = int64_t(1) << 24;
constexpr int kClassesPerBlockMin = 64;      // the smallest class tile of a workgroup (CT = 1): sizes the workspace

__device__ __forceinline__ uint64_t argmax_key(float v, int cls) {
  uint32_t u = __float_as_uint(v);
  uint32_t o;
  if (v != v)
    o = 0xFFFFFFFFu;                         // NaN: above +inf (0xFF800000), every NaN equal -> the first one wins
  else if (v == 0.0f)
    o = 0x80000000u;                         // -0 == +0 for torch.argmax
  else
    o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return (uint64_t(o) << 32) | uint32_t(~uint32_t(cls));
}

__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

template <int RT, int CT, int U>
__global__ __launch_bounds__(256) void head_gemm(const float* __restrict__ emb, int64_t B, int d, const float* __restrict__ w,
                                                 const float* __restrict__ bias, int N, float* __restrict__ logits,
                                                 uint64_t* __restrict__ keys, int64_t* __restrict__ ids, int nrb) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int rb = blockIdx.x % nrb, cb = blockIdx.x / nrb;
  const int64_t r0 = int64_t(rb) * (16 * RT);
  const int n0 = cb * (64 * CT) + wave * (16 * CT);

  const float* pa[RT];
  const float* pb[CT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    int64_t r = r0 + 16 * t + i;
    pa[t] = emb + (r < B ? r : B - 1) * int64_t(d) + 4 * q;
  }
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    int n = n0 + 16 * c + i;
    pb[c] = w + int64_t(n < N ? n : N - 1) * d + 4 * q;
  }

  f32x4 acc[RT][CT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kb = 0; kb < d; kb += 16 * U) {
    float4 a[U][RT], b[U][CT];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = kb + 16 * u + 4 * q;     // d % 4 == 0: a float4 is either wholly inside the row or wholly past its end
      const bool in = k < d;
#pragma unroll
      for (int t = 0; t < RT; ++t) a[u][t] = in ? *reinterpret_cast<const float4*>(pa[t] + kb + 16 * u) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int c = 0; c < CT; ++c) b[u][c] = in ? *reinterpret_cast<const float4*>(pb[c] + kb + 16 * u) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (kb + 16 * u >= d) break;           // wave-uniform: a block wholly past d adds nothing
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][t].x, b[u][c].x, acc[t][c], 0, 0, 0);
          acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][t].y, b[u][c].y, acc[t][c], 0, 0, 0);
          acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][t].z, b[u][c].z, acc[t][c], 0, 0, 0);
          acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][t].w, b[u][c].w, acc[t][c], 0, 0, 0);
        }
    }
  }

  // C/D layout: lane l, register r -> row 4*(l >> 4) + r, column l & 15
  float bv[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    int n = n0 + 16 * c + i;
    bv[c] = bias[n < N ? n : N - 1];
  }
  __shared__ uint64_t red[4][16 * RT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = r0 + 16 * t + 4 * q + r;
      uint64_t key = 0;                      // below every real key (the smallest real high half is 0x007FFFFF, -inf)
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const int n = n0 + 16 * c + i;
        const float v = acc[t][c][r] + bv[c];
        if (n < N) {
          if (logits != nullptr && row < B) logits[row * N + n] = v;
          key = umax64(key, argmax_key(v, n));
        }
      }
      if (keys != nullptr || ids != nullptr) {
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) key = umax64(key, __shfl_xor(key, m, 16));
        if (i == 0) red[wave][16 * t + 4 * q + r] = key;
      }
    }
  if (keys == nullptr && ids == nullptr) return;
  __syncthreads();
  if (threadIdx.x < 16 * RT) {
    const int64_t row = r0 + threadIdx.x;
    if (row < B) {
      uint64_t key = umax64(umax64(red[0][threadIdx.x], red[1][threadIdx.x]), umax64(red[2][threadIdx.x], red[3][threadIdx.x]));
      if (ids != nullptr)
        ids[row] = int64_t(~uint32_t(key));
      else
        keys[row * (gridDim.x / nrb) + cb] = key;
    }
  }
}

// one wave per row: max over the row's class-block keys
__global__ __launch_bounds__(64) void head_argmax_final(const uint64_t* __restrict__ keys, int ncb, int64_t* __restrict__ ids) {
  const int64_t row = blockIdx.x;
  uint64_t key = 0;
  for (int j = threadIdx.x; j < ncb; j += 64) key = umax64(key, keys[row * ncb + j]);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) key = umax64(key, __shfl_xor(key, m, 64));
  if (threadIdx.x == 0) ids[row] = int64_t(~uint32_t(key));
}

template <int RT, int CT, int U>
void launch(const float* emb, int64_t B, int d, const float* w, const float* bias, int N, float* logits, uint64_t* keys,
            int64_t* ids, int nrb, int ncb, hipStream_t s) {
  hipLaunchKernelGGL((head_gemm<RT, CT, U>), dim3(unsigned(nrb) * unsigned(ncb)), dim3(256), 0, s, emb, B, d, w, bias, N, logits,
                     keys, ids, nrb);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int effocr_head_abi_version(void) { return EFFOCR_HEAD_ABI_VERSION; }

const char* effocr_head_last_error(void) { return g_err.c_str(); }

size_t effocr_classifier_head_workspace_bytes(int64_t batch, int n_classes) {
  if (batch <= 0 || n_classes < 1) return 0;
  const int64_t ncb = (int64_t(n_classes) + kClassesPerBlockMin - 1) / kClassesPerBlockMin;
  return size_t(batch) * size_t(ncb) * sizeof(uint64_t);
}

int effocr_classifier_head(const float* emb_dev, int64_t batch, int d, const float* w_dev, const float* b_dev, int n_classes,
                           float* logits_dev, int64_t* ids_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (batch < 0 || batch > kMaxBatch) return fail(EFFOCR_HEAD_EINVAL, "classifier_head: batch must be in [0, 2^24]");
  if (d < 4 || d > kMaxD || d % 4 != 0) return fail(EFFOCR_HEAD_EINVAL, "classifier_head: d must be a multiple of 4 in [4, 4096]");
  if (n_classes < 1) return fail(EFFOCR_HEAD_EINVAL, "classifier_head: n_classes must be >= 1");
  if (batch == 0) return EFFOCR_HEAD_OK;     // nothing to compute or write (an empty torch tensor's data pointer is NULL)
  if (logits_dev == nullptr && ids_dev == nullptr) return fail(EFFOCR_HEAD_EINVAL, "classifier_head: logits and ids both NULL");
  if (w_dev == nullptr || b_dev == nullptr || emb_dev == nullptr)
    return fail(EFFOCR_HEAD_EINVAL, "classifier_head: NULL input");
  if (!aligned16(emb_dev) || !aligned16(w_dev)) return fail(EFFOCR_HEAD_EINVAL, "classifier_head: emb and w must be 16-byte aligned");
  const int RT = batch <= 16 ? 1 : batch <= 32 ? 2 : 4;
  const int CT = batch <= 64 ? 1 : 2;
  const int64_t nrb = (batch + 16 * RT - 1) / (16 * RT);
  const int64_t ncb = (int64_t(n_classes) + 64 * CT - 1) / (64 * CT);
  if (nrb * ncb > INT32_MAX) return fail(EFFOCR_HEAD_EINVAL, "classifier_head: batch x n_classes too large for one grid");
  uint64_t* keys = nullptr;
  if (ids_dev != nullptr && ncb > 1) {
    const size_t need = effocr_classifier_head_workspace_bytes(batch, n_classes);
    if (workspace_bytes < need || workspace_dev == nullptr)
      return fail(EFFOCR_HEAD_EINVAL, "classifier_head: workspace of " + std::to_string(workspace_bytes) + " bytes, " +
                                          std::to_string(need) + " needed");
    keys = static_cast<uint64_t*>(workspace_dev);
  } else if (ids_dev != nullptr) {
    // one class block: the GEMM writes the ids itself; the workspace check stays so a caller's size never depends on the tiling
    if (workspace_bytes < effocr_classifier_head_workspace_bytes(batch, n_classes))
      return fail(EFFOCR_HEAD_EINVAL, "classifier_head: workspace too small");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  int64_t* gemm_ids = (ids_dev != nullptr && ncb == 1) ? ids_dev : nullptr;
  const int nr = int(nrb), nc = int(ncb);
  if (RT == 1)
    launch<1, 1, 4>(emb_dev, batch, d, w_dev, b_dev, n_classes, logits_dev, keys, gemm_ids, nr, nc, s);
  else if (RT == 2)
    launch<2, 1, 4>(emb_dev, batch, d, w_dev, b_dev, n_classes, logits_dev, keys, gemm_ids, nr, nc, s);
  else if (CT == 1)
    launch<4, 1, 2>(emb_dev, batch, d, w_dev, b_dev, n_classes, logits_dev, keys, gemm_ids, nr, nc, s);
  else
    launch<4, 2, 2>(emb_dev, batch, d, w_dev, b_dev, n_classes, logits_dev, keys, gemm_ids, nr, nc, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EFFOCR_HEAD_EHIP, std::string("classifier_head: ") + hipGetErrorString(e));
  if (keys != nullptr) {
    hipLaunchKernelGGL(head_argmax_final, dim3(unsigned(batch)), dim3(64), 0, s, keys, nc, ids_dev);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(EFFOCR_HEAD_EHIP, std::string("classifier_head argmax: ") + hipGetErrorString(e));
  }
  return EFFOCR_HEAD_OK;
}

}  // extern "C"
