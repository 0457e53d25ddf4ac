// PVTv2 encoder kernels on gfx950 (timm pvt_v2_b0 .. pvt_v2_b5 semantics; pvt_api.hip: pvt_forward).  Part of libeffocr_pvt.so only.  What
// PVTv2 adds to this tree: an attention whose N queries attend to at most 49 spatially reduced keys, a depthwise 3x3 + GELU inside the
// MLP on token rows, overlapping patch embeddings and the spatial reduction as implicit GEMMs, and a GEMM that takes the family's narrow
// widths (32, 64, 160, 320 and their kv widths) as they are.  Contracts and rounding points: pvt.hpp.
#include "common.hpp"
#include "kernels.hpp"
#include "pvt.hpp"
#include <math.h>

namespace effocr {
namespace {

constexpr int KSLOTS = (PVT_MAX_KEYS + 31) / 32 * 32;    // 64 key slots: two 32-key tiles

// ---------------------------------------------------------------------------------------------------------------------------
// MFMA fragments: a lane holds 8 consecutive k of row (lane & 31), k = 16 step + 8 (lane >> 5) + 0 .. 7.  mma(a, b, c): c[r] += sum_k
// a[row mfma32_row(r, lane)][k] b[row lane & 31][k].  16-bit: one v_mfma_f32_32x32x16; fp32: eight v_mfma_f32_32x32x2f32, the j-th taking
// element j of both halves (k = j and 8 + j) — the same 16 k per step, in a fixed order.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename E> struct Frag {
  typename Op16<E>::V8 v;
  __device__ __forceinline__ void zero() { v = __builtin_bit_cast(typename Op16<E>::V8, u32x4{0u, 0u, 0u, 0u}); }
  __device__ __forceinline__ void load(const E* p) { v = __builtin_bit_cast(typename Op16<E>::V8, *reinterpret_cast<const u32x4*>(p)); }
  __device__ __forceinline__ void set(int j, float f) { v[j] = (E)f; }
  static __device__ __forceinline__ f32x16 mma(const Frag& a, const Frag& b, f32x16 c) { return Op16<E>::mfma(a.v, b.v, c); }
};
template <> struct Frag<float> {
  float v[8];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
  }
  __device__ __forceinline__ void load(const float* p) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
  }
  __device__ __forceinline__ void set(int j, float f) { v[j] = f; }
  static __device__ __forceinline__ f32x16 mma(const Frag& a, const Frag& b, f32x16 c) {
#pragma unroll
    for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[j], b.v[j], c, 0, 0, 0);
    return c;
  }
};

template <typename E> __device__ __forceinline__ void store4(E* p, float a, float b, float c, float d) {
  if constexpr (sizeof(E) == 4) *reinterpret_cast<f32x4*>(p) = f32x4{a, b, c, d};
  else *reinterpret_cast<u32x2*>(p) = pack4<E>(a, b, c, d);
}
template <typename E> __device__ __forceinline__ void load4(const E* p, float (&v)[4]) {
  if constexpr (sizeof(E) == 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = a[j];
  } else {
    E x[4];
    *reinterpret_cast<u32x2*>(x) = *reinterpret_cast<const u32x2*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (float)x[j];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// GEMM.  A workgroup is four independent waves (no LDS, no barrier); wave w of block (x, y) owns rows 32 (4 x + w) .. + 32 and columns
// 32 NT y .. + 32 NT.  W is the MFMA's first operand, so that a lane ends up with one row and runs of 4 consecutive columns of it.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename E, int AMODE, int NT>
__global__ __launch_bounds__(256) void pvt_gemm_kernel(PvtGemm g, int epi, int OH) {
  const int lane = lane_id(), r31 = lane & 31, half = lane >> 5;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave_id()) * 32;
  if (row0 >= g.rows) return;
  const int n0 = blockIdx.y * (32 * NT);
  const int K = g.K, N = g.N;
  const int64_t row = row0 + r31;
  const int64_t rl = row < g.rows ? row : g.rows - 1;     // a slot past the last row repeats it and is not stored
  // this lane's row of the activation operand
  int b = 0, oy = 0, ox = 0;
  if constexpr (AMODE != PVT_A_DENSE) {
    const int64_t per = (int64_t)OH * OH;
    b = (int)(rl / per);
    const int i = (int)(rl - (int64_t)b * per);
    oy = i / OH; ox = i - oy * OH;
  }
  const E* wrow[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) wrow[t] = static_cast<const E*>(g.W) + (int64_t)(n0 + 32 * t + r31) * K + 8 * half;
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  for (int k0 = 0; k0 < K; k0 += 16) {
    const int k = k0 + 8 * half;
    Frag<E> xf;
    if constexpr (AMODE == PVT_A_DENSE) {
      xf.load(static_cast<const E*>(g.X) + rl * K + k);
    } else if constexpr (AMODE == PVT_A_CONV) {
      const int tap = k / g.Cin, c = k - tap * g.Cin;
      const int ky = tap / g.ksize, kx = tap - ky * g.ksize;
      const int iy = oy * g.stride - g.pad + ky, ix = ox * g.stride - g.pad + kx;
      if (iy >= 0 && iy < g.H && ix >= 0 && ix < g.H) xf.load(static_cast<const E*>(g.X) + (((int64_t)b * g.H + iy) * g.H + ix) * g.Cin + c);
      else xf.zero();
    } else {
      const float* img = static_cast<const float*>(g.X) + (int64_t)b * 3 * g.H * g.H;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int kk = k + j;
        const int c = kk / 49, rem = kk - c * 49;
        const int ky = rem / 7, kx = rem - ky * 7;
        const int iy = oy * 4 - 3 + ky, ix = ox * 4 - 3 + kx;
        float v = 0.f;
        if (kk < 147 && iy >= 0 && iy < g.H && ix >= 0 && ix < g.H) v = img[((int64_t)c * g.H + iy) * g.H + ix];
        xf.set(j, v);
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      Frag<E> wf;
      wf.load(wrow[t] + k0);
      acc[t] = Frag<E>::mma(wf, xf, acc[t]);
    }
  }
  if (row >= g.rows) return;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int n = n0 + 32 * t + 8 * q4 + 4 * half;
      const f32x4 bv = *reinterpret_cast<const f32x4*>(g.bias + n);
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = acc[t][4 * q4 + e] + bv[e];
      const int64_t o = row * N + n;
      if (epi == PVT_EPI_OP) {
        store4<E>(static_cast<E*>(g.out) + o, v[0], v[1], v[2], v[3]);
      } else {
        if (epi == PVT_EPI_RESID) {
          const f32x4 rv = *reinterpret_cast<const f32x4*>(g.resid + o);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = rv[e] + v[e];
        }
        *reinterpret_cast<f32x4*>(static_cast<float*>(g.out) + o) = f32x4{v[0], v[1], v[2], v[3]};
      }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Attention, 16-bit modes.  Scores are computed swapped (S^T = K Q^T) so that a lane holds one query and 16 keys of a tile — register r is
// key 32 kt + (r & 3) + 8 (r >> 2) + 4 half — and the P fragment feeds O^T = V^T P^T as it falls out.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename E, int HD>
__global__ __launch_bounds__(256) void pvt_attn_mfma_kernel(const E* __restrict__ q, const E* __restrict__ kv, E* __restrict__ out, int N, int M,
                                                            int heads, int nchunks, float scale) {
  typedef typename Op16<E>::V8 V8;
  constexpr int KROW = HD * 2 + 16;         // bytes per K row (padded by 16 B)
  constexpr int KC = HD / 8;                // 16-byte chunks per K (and V) row
  constexpr int VS = KSLOTS / 2 + 6;        // dwords per V^T row (even, VS / 2 odd -> conflict-free b64 reads)
  constexpr int NDB = HD / 32;
  __shared__ __attribute__((aligned(16))) char sK[KSLOTS * KROW];
  __shared__ __attribute__((aligned(16))) uint32_t sV[HD * VS];

  const int tid = threadIdx.x, lane = tid & 63, r31 = lane & 31, half = lane >> 5;
  const int w = wave_id();
  const int chunk = blockIdx.x % nchunks, bh = blockIdx.x / nchunks;
  const int b = bh / heads, h = bh - b * heads;
  const int ld = heads * HD, ldkv = 2 * ld;
  const int nkt = (M + 31) / 32, TP = nkt * 32;
  const E* qb_ = q + (int64_t)b * N * ld + h * HD;
  const E* kb_ = kv + (int64_t)b * M * ldkv + h * HD;
  const E* vb_ = kb_ + ld;

  // K rows (zero rows from M on: those slots are never read from memory)
  for (int id = tid; id < TP * KC; id += 256) {
    const int t = id / KC, c = id - t * KC;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (t < M) v = *reinterpret_cast<const u32x4*>(kb_ + (int64_t)t * ldkv + c * 8);
    *reinterpret_cast<u32x4*>(sK + t * KROW + c * 16) = v;
  }
  // V transposed: dword (d, tp) = {V[2 tp][d], V[2 tp + 1][d]} (zeros from M on)
  for (int id = tid; id < (TP / 2) * KC; id += 256) {
    const int tp = id / KC, c = id - tp * KC, t0 = 2 * tp;
    u32x4 v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
    if (t0 < M) v0 = *reinterpret_cast<const u32x4*>(vb_ + (int64_t)t0 * ldkv + c * 8);
    if (t0 + 1 < M) v1 = *reinterpret_cast<const u32x4*>(vb_ + (int64_t)(t0 + 1) * ldkv + c * 8);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const uint32_t lo = v0[jj], hi = v1[jj];
      sV[(c * 8 + 2 * jj) * VS + tp] = (lo & 0xffffu) | (hi << 16);
      sV[(c * 8 + 2 * jj + 1) * VS + tp] = (lo >> 16) | (hi & 0xffff0000u);
    }
  }
  __syncthreads();

  constexpr float LOG2E = 1.44269504088896340736f;
  const int q0 = chunk * PVT_QCHUNK;
  const int q1 = min(N, q0 + PVT_QCHUNK);
  for (int qs = q0 + w * PVT_QBLK; qs < q1; qs += 4 * PVT_QBLK) {
    int tq = qs + r31;
    const bool qvalid = tq < q1;
    tq = qvalid ? tq : q1 - 1;
    V8 qf[HD / 16];
#pragma unroll
    for (int ks = 0; ks < HD / 16; ++ks)
      qf[ks] = __builtin_bit_cast(V8, *reinterpret_cast<const u32x4*>(qb_ + (int64_t)tq * ld + (2 * ks + half) * 8));

    f32x16 sc[2];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[kt][r] = kt < nkt ? 0.f : -INFINITY;
      if (kt < nkt) {
#pragma unroll
        for (int ks = 0; ks < HD / 16; ++ks) {
          const V8 kf = *reinterpret_cast<const V8*>(sK + (kt * 32 + r31) * KROW + (2 * ks + half) * 16);
          sc[kt] = Op16<E>::mfma(kf, qf[ks], sc[kt]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          const float v = key < M ? sc[kt][r] * scale : -INFINITY;   // a padded key: weight exactly 0
          sc[kt][r] = v;
          mx = fmaxf(mx, v);
        }
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));               // key 0 is always live: mx is finite unless a score is not
    const float mc = mx * LOG2E;
    f32x16 o[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      if (kt < nkt) {
#pragma unroll
        for (int mm = 0; mm < 2; ++mm) {
          V8 pf;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float p = __builtin_amdgcn_exp2f(fmaf(sc[kt][8 * mm + j], LOG2E, -mc));
            l += p;
            pf[j] = (E)p;
          }
#pragma unroll
          for (int db = 0; db < NDB; ++db) {
            const uint32_t* vp = sV + (db * 32 + r31) * VS + (kt * 16 + 8 * mm + 2 * half);
            const u32x2 lo = *reinterpret_cast<const u32x2*>(vp);
            const u32x2 hi = *reinterpret_cast<const u32x2*>(vp + 4);
            const u32x4 vv = {lo[0], lo[1], hi[0], hi[1]};
            o[db] = Op16<E>::mfma(__builtin_bit_cast(V8, vv), pf, o[db]);
          }
        }
      }
    }
    l += __shfl_xor(l, 32, 64);
    if (qvalid) {
      const float inv = 1.0f / l;
      E* orow = out + ((int64_t)b * N + tq) * ld + h * HD;
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
          *reinterpret_cast<u32x2*>(orow + db * 32 + 8 * q4 + 4 * half) =
              pack4<E>(o[db][4 * q4] * inv, o[db][4 * q4 + 1] * inv, o[db][4 * q4 + 2] * inv, o[db][4 * q4 + 3] * inv);
    }
  }
}

// fp32 mode: K and V of the (crop, head) staged in LDS, one thread per (query, 32 values).  The parity path, not a throughput kernel.
template <int HD>
__global__ __launch_bounds__(256) void pvt_attn_f32_kernel(const float* __restrict__ q, const float* __restrict__ kv, float* __restrict__ out, int N,
                                                           int M, int heads, int nchunks, float scale) {
  __shared__ __attribute__((aligned(16))) float sK[PVT_MAX_KEYS * HD];
  __shared__ __attribute__((aligned(16))) float sV[PVT_MAX_KEYS * HD];
  constexpr int NCH = HD / 32;
  const int chunk = blockIdx.x % nchunks, bh = blockIdx.x / nchunks;
  const int b = bh / heads, h = bh - b * heads;
  const int ld = heads * HD, ldkv = 2 * ld;
  const float* qb_ = q + (int64_t)b * N * ld + h * HD;
  const float* kb_ = kv + (int64_t)b * M * ldkv + h * HD;
  for (int id = threadIdx.x; id < M * (HD / 4); id += 256) {
    const int t = id / (HD / 4), c = id - t * (HD / 4);
    *reinterpret_cast<f32x4*>(sK + t * HD + 4 * c) = *reinterpret_cast<const f32x4*>(kb_ + (int64_t)t * ldkv + 4 * c);
    *reinterpret_cast<f32x4*>(sV + t * HD + 4 * c) = *reinterpret_cast<const f32x4*>(kb_ + ld + (int64_t)t * ldkv + 4 * c);
  }
  __syncthreads();
  const int q0 = chunk * PVT_QCHUNK;
  const int nq = min(N, q0 + PVT_QCHUNK) - q0;
  for (int id = threadIdx.x; id < nq * NCH; id += 256) {
    const int tq = q0 + id / NCH, ch = id % NCH;
    float qv[HD], o[32];
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(qb_ + (int64_t)tq * ld + d);
#pragma unroll
      for (int e = 0; e < 4; ++e) qv[d + e] = v[e];
    }
    float mx = -INFINITY;
    for (int key = 0; key < M; ++key) {
      float sc = 0.f;
#pragma unroll
      for (int d = 0; d < HD; ++d) sc = fmaf(qv[d], sK[key * HD + d], sc);
      mx = fmaxf(mx, sc * scale);
    }
#pragma unroll
    for (int d = 0; d < 32; ++d) o[d] = 0.f;
    float l = 0.f;
    for (int key = 0; key < M; ++key) {
      float sc = 0.f;
#pragma unroll
      for (int d = 0; d < HD; ++d) sc = fmaf(qv[d], sK[key * HD + d], sc);
      const float p = expf(sc * scale - mx);
      l += p;
      const float* vr = sV + key * HD + ch * 32;
#pragma unroll
      for (int d = 0; d < 32; ++d) o[d] = fmaf(p, vr[d], o[d]);
    }
    const float inv = 1.0f / l;
    float* orow = out + ((int64_t)b * N + tq) * ld + h * HD + ch * 32;
#pragma unroll
    for (int d = 0; d < 32; d += 4) *reinterpret_cast<f32x4*>(orow + d) = f32x4{o[d] * inv, o[d + 1] * inv, o[d + 2] * inv, o[d + 3] * inv};
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// depthwise 3x3 + bias + GELU: one thread per (token, 4 channels)
// ---------------------------------------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(256) void pvt_dwconv_gelu_kernel(const E* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                              E* __restrict__ out, int B, int H, int W, int C) {
  const int c4n = C / 4;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (int64_t)B * H * W * c4n) return;
  const int c = 4 * (int)(id % c4n);
  const int64_t pix = id / c4n;
  const int x = (int)(pix % W), y = (int)((pix / W) % H);
  const int64_t b = pix / ((int64_t)H * W);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = y - 1 + ky;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = x - 1 + kx;
      if (ix < 0 || ix >= W) continue;
      float v[4];
      load4<E>(in + ((b * H + iy) * W + ix) * C + c, v);
      const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (ky * 3 + kx) * C + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(v[e], wv[e], acc[e]);
    }
  }
  const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + c);
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = gelu_erf(acc[e] + bv[e]);
  store4<E>(out + pix * C + c, acc[0], acc[1], acc[2], acc[3]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// LayerNorm: one wave per row, lane l holds columns 4 l + 256 j (j = 0, 1)
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename TO>
__global__ __launch_bounds__(256) void pvt_layernorm_kernel(const float* __restrict__ x, int64_t rows, int C, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, TO* __restrict__ out) {
  const int lane = lane_id();
  const int64_t row = (int64_t)blockIdx.x * 4 + wave_id();
  if (row >= rows) return;
  float v[2][4];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = 4 * lane + 256 * j;
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    if (c < C) t = *reinterpret_cast<const f32x4*>(x + row * C + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[j][e] = t[e]; sum += t[e]; }
  }
  const float mean = wave_sum(sum) / (float)C;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j)
    if (4 * lane + 256 * j < C) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[j][e] -= mean; sq += v[j][e] * v[j][e]; }
    }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)C + eps);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = 4 * lane + 256 * j;
    if (c < C) {
      const f32x4 gv = *reinterpret_cast<const f32x4*>(gamma + c), bv = *reinterpret_cast<const f32x4*>(beta + c);
      float y[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = fmaf(v[j][e] * rstd, gv[e], bv[e]);
      store4<TO>(out + row * C + c, y[0], y[1], y[2], y[3]);
    }
  }
}

// one crop per workgroup; a block sum is xor-shuffles inside each wave, then the four waves through LDS in a fixed order
__global__ __launch_bounds__(256) void pvt_pool_kernel(const float* __restrict__ x, int T, int D, int l2norm, float* __restrict__ emb,
                                                       int* __restrict__ status) {
  __shared__ float ws[4];
  const int64_t b = blockIdx.x;
  constexpr int PER = 4;                                   // D <= 1024
  float v[PER];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int c = threadIdx.x + 256 * k;
    float sum = 0.f;
    if (c < D)
      for (int t = 0; t < T; ++t) sum += x[(b * T + t) * (int64_t)D + c];
    v[k] = sum / (float)T;
    ss += v[k] * v[k];
  }
  if (l2norm) {
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float nrm = fmaxf(sqrtf((ws[0] + ws[1]) + (ws[2] + ws[3])), 1e-12f);   // F.normalize: x / max(||x||, eps)
#pragma unroll
    for (int k = 0; k < PER; ++k) v[k] = v[k] / nrm;
  }
  bool bad = false;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int c = threadIdx.x + 256 * k;
    if (c < D) {
      emb[b * D + c] = v[k];
      bad |= !(fabsf(v[k]) <= 3.0e38f);
    }
  }
  if (status && bad) atomicOr(status, 1);
}

template <typename E, int AMODE>
int launch_gemm(int epi, const PvtGemm& g, int OH, hipStream_t s) {
  const unsigned gx = (unsigned)((g.rows + 127) / 128);
  if (g.N % 64 == 0) hipLaunchKernelGGL((pvt_gemm_kernel<E, AMODE, 2>), dim3(gx, (unsigned)(g.N / 64)), dim3(256), 0, s, g, epi, OH);
  else hipLaunchKernelGGL((pvt_gemm_kernel<E, AMODE, 1>), dim3(gx, (unsigned)(g.N / 32)), dim3(256), 0, s, g, epi, OH);
  return check_launch("pvt_gemm");
}

template <typename E>
int launch_gemm_mode(int epi, const PvtGemm& g, int OH, hipStream_t s) {
  switch (g.amode) {
    case PVT_A_DENSE: return launch_gemm<E, PVT_A_DENSE>(epi, g, OH, s);
    case PVT_A_CONV: return launch_gemm<E, PVT_A_CONV>(epi, g, OH, s);
    default: return launch_gemm<E, PVT_A_STEM>(epi, g, OH, s);
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int pvt_gemm(int prec, int epi, const PvtGemm& g, hipStream_t s) {
  if (g.rows <= 0) return EFFOCR_OK;
  if (!g.X || !g.W || !g.bias || !g.out || (epi == PVT_EPI_RESID && !g.resid)) return fail(EFFOCR_EINVAL, "pvt_gemm: NULL argument");
  if (epi < PVT_EPI_OP || epi > PVT_EPI_RESID) return fail(EFFOCR_EINVAL, "pvt_gemm: unknown epilogue");
  if (g.N < 32 || g.N % 32 || g.K < 16 || g.K % 16) return fail(EFFOCR_EUNSUPPORTED, "pvt_gemm: N % 32 == 0 and K % 16 == 0 required");
  if (!aligned16(g.X) || !aligned16(g.W) || !aligned16(g.bias) || !aligned16(g.out) || (g.resid && !aligned16(g.resid)))
    return fail(EFFOCR_EINVAL, "pvt_gemm: pointers must be 16-byte aligned");
  if (g.rows > ((int64_t)1 << 31) - 256) return fail(EFFOCR_EUNSUPPORTED, "pvt_gemm: too many rows for one launch");
  int OH = 0;
  if (g.amode == PVT_A_CONV) {
    if (g.B < 1 || g.H < 1 || g.Cin < 8 || g.Cin % 8 || g.ksize < 1 || g.stride < 1 || g.pad < 0 || g.H + 2 * g.pad < g.ksize)
      return fail(EFFOCR_EUNSUPPORTED, "pvt_gemm: convolution operand needs Cin % 8 == 0 and a kernel that fits the padded grid");
    OH = (g.H + 2 * g.pad - g.ksize) / g.stride + 1;
    if (g.K != g.ksize * g.ksize * g.Cin || g.rows != (int64_t)g.B * OH * OH) return fail(EFFOCR_EINVAL, "pvt_gemm: K / rows do not match the convolution geometry");
  } else if (g.amode == PVT_A_STEM) {
    if (g.B < 1 || g.H < 4 || g.H % 4) return fail(EFFOCR_EUNSUPPORTED, "pvt_gemm: the stem needs a crop side that is a multiple of 4");
    OH = g.H / 4;
    if (g.K != PVT_STEM_K || g.rows != (int64_t)g.B * OH * OH) return fail(EFFOCR_EINVAL, "pvt_gemm: K / rows do not match the stem geometry");
  } else if (g.amode != PVT_A_DENSE) {
    return fail(EFFOCR_EINVAL, "pvt_gemm: unknown operand mode");
  }
  switch (prec) {
    case PREC_BF16: return launch_gemm_mode<__bf16>(epi, g, OH, s);
    case PREC_FP16: return launch_gemm_mode<_Float16>(epi, g, OH, s);
    case PREC_FP32: return launch_gemm_mode<float>(epi, g, OH, s);
  }
  return fail(EFFOCR_EINVAL, "pvt_gemm: unknown precision");
}

int pvt_attention(int prec, const void* q, const void* kv, int B, int N, int M, int heads, int hd, void* out, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (!q || !kv || !out) return fail(EFFOCR_EINVAL, "pvt_attention: NULL argument");
  if (N < 1 || M < 1 || M > PVT_MAX_KEYS || heads < 1 || (hd != 32 && hd != 64))
    return fail(EFFOCR_EUNSUPPORTED, "pvt_attention: N >= 1, 1 <= M <= 49, heads >= 1 and a head width of 32 or 64 required");
  if (!aligned16(q) || !aligned16(kv) || !aligned16(out)) return fail(EFFOCR_EINVAL, "pvt_attention: pointers must be 16-byte aligned");
  const int nchunks = (N + PVT_QCHUNK - 1) / PVT_QCHUNK;
  if ((int64_t)B * heads * nchunks >= (int64_t)1 << 31) return fail(EFFOCR_EUNSUPPORTED, "pvt_attention: too many workgroups for one launch");
  const dim3 grid((unsigned)(B * heads * nchunks)), blk(256);
  const float scale = 1.0f / sqrtf((float)hd);
  switch (prec) {
    case PREC_BF16:
      if (hd == 32) hipLaunchKernelGGL((pvt_attn_mfma_kernel<__bf16, 32>), grid, blk, 0, s, static_cast<const __bf16*>(q), static_cast<const __bf16*>(kv), static_cast<__bf16*>(out), N, M, heads, nchunks, scale);
      else hipLaunchKernelGGL((pvt_attn_mfma_kernel<__bf16, 64>), grid, blk, 0, s, static_cast<const __bf16*>(q), static_cast<const __bf16*>(kv), static_cast<__bf16*>(out), N, M, heads, nchunks, scale);
      break;
    case PREC_FP16:
      if (hd == 32) hipLaunchKernelGGL((pvt_attn_mfma_kernel<_Float16, 32>), grid, blk, 0, s, static_cast<const _Float16*>(q), static_cast<const _Float16*>(kv), static_cast<_Float16*>(out), N, M, heads, nchunks, scale);
      else hipLaunchKernelGGL((pvt_attn_mfma_kernel<_Float16, 64>), grid, blk, 0, s, static_cast<const _Float16*>(q), static_cast<const _Float16*>(kv), static_cast<_Float16*>(out), N, M, heads, nchunks, scale);
      break;
    case PREC_FP32:
      if (hd == 32) hipLaunchKernelGGL((pvt_attn_f32_kernel<32>), grid, blk, 0, s, static_cast<const float*>(q), static_cast<const float*>(kv), static_cast<float*>(out), N, M, heads, nchunks, scale);
      else hipLaunchKernelGGL((pvt_attn_f32_kernel<64>), grid, blk, 0, s, static_cast<const float*>(q), static_cast<const float*>(kv), static_cast<float*>(out), N, M, heads, nchunks, scale);
      break;
    default: return fail(EFFOCR_EINVAL, "pvt_attention: unknown precision");
  }
  return check_launch("pvt_attention");
}

int pvt_dwconv_gelu(int prec, const void* in, int B, int H, int W, int C, const float* w, const float* bias, void* out, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (!in || !w || !bias || !out) return fail(EFFOCR_EINVAL, "pvt_dwconv_gelu: NULL argument");
  if (H < 1 || W < 1 || C < 4 || C % 4) return fail(EFFOCR_EUNSUPPORTED, "pvt_dwconv_gelu: H, W >= 1 and C % 4 == 0 required");
  if (!aligned16(in) || !aligned16(w) || !aligned16(bias) || !aligned16(out)) return fail(EFFOCR_EINVAL, "pvt_dwconv_gelu: pointers must be 16-byte aligned");
  const int64_t n = (int64_t)B * H * W * (C / 4);
  if ((n + 255) / 256 >= (int64_t)1 << 31) return fail(EFFOCR_EUNSUPPORTED, "pvt_dwconv_gelu: too many outputs for one launch");
  const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
  switch (prec) {
    case PREC_BF16: hipLaunchKernelGGL(pvt_dwconv_gelu_kernel<__bf16>, grid, blk, 0, s, static_cast<const __bf16*>(in), w, bias, static_cast<__bf16*>(out), B, H, W, C); break;
    case PREC_FP16: hipLaunchKernelGGL(pvt_dwconv_gelu_kernel<_Float16>, grid, blk, 0, s, static_cast<const _Float16*>(in), w, bias, static_cast<_Float16*>(out), B, H, W, C); break;
    case PREC_FP32: hipLaunchKernelGGL(pvt_dwconv_gelu_kernel<float>, grid, blk, 0, s, static_cast<const float*>(in), w, bias, static_cast<float*>(out), B, H, W, C); break;
    default: return fail(EFFOCR_EINVAL, "pvt_dwconv_gelu: unknown precision");
  }
  return check_launch("pvt_dwconv_gelu");
}

int pvt_layernorm(int prec, const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps, void* out, int out_f32,
                  hipStream_t s) {
  if (rows <= 0) return EFFOCR_OK;
  if (!x || !gamma || !beta || !out) return fail(EFFOCR_EINVAL, "pvt_layernorm: NULL argument");
  if (C < 4 || C % 4 || C > PVT_MAX_WIDTH) return fail(EFFOCR_EUNSUPPORTED, "pvt_layernorm: C % 4 == 0 and 4 <= C <= 512 required");
  if (!aligned16(x) || !aligned16(gamma) || !aligned16(beta) || !aligned16(out)) return fail(EFFOCR_EINVAL, "pvt_layernorm: pointers must be 16-byte aligned");
  if ((rows + 3) / 4 >= (int64_t)1 << 31) return fail(EFFOCR_EUNSUPPORTED, "pvt_layernorm: too many rows for one launch");
  const dim3 grid((unsigned)((rows + 3) / 4)), blk(256);
  if (out_f32 || prec == PREC_FP32) hipLaunchKernelGGL(pvt_layernorm_kernel<float>, grid, blk, 0, s, x, rows, C, gamma, beta, eps, static_cast<float*>(out));
  else if (prec == PREC_BF16) hipLaunchKernelGGL(pvt_layernorm_kernel<__bf16>, grid, blk, 0, s, x, rows, C, gamma, beta, eps, static_cast<__bf16*>(out));
  else if (prec == PREC_FP16) hipLaunchKernelGGL(pvt_layernorm_kernel<_Float16>, grid, blk, 0, s, x, rows, C, gamma, beta, eps, static_cast<_Float16*>(out));
  else return fail(EFFOCR_EINVAL, "pvt_layernorm: unknown precision");
  return check_launch("pvt_layernorm");
}

int pvt_pool(const float* x, int B, int T, int D, int l2norm, float* emb, int* status, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (!x || !emb) return fail(EFFOCR_EINVAL, "pvt_pool: NULL argument");
  if (T < 1 || D < 1 || D > 1024) return fail(EFFOCR_EUNSUPPORTED, "pvt_pool: 1 <= D <= 1024 and T >= 1 required");
  hipLaunchKernelGGL(pvt_pool_kernel, dim3((unsigned)B), dim3(256), 0, s, x, T, D, l2norm, emb, status);
  return check_launch("pvt_pool");
}

}  // namespace effocr
