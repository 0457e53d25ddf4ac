// BEiT encoder kernels on gfx950 (timm beit_base_patch16_224 / beitv2_base_patch16_224 semantics; beit_api.hip: beit_forward).  Part
// of libeffocr_beit.so only.  The patch im2col, the LayerNorms and the cls row come from vit_ops.hip, the linears from gemm.hip /
// gemm2.hip; what BEiT adds is attention with an additive relative-position bias and a head that pools the patch tokens.
//
// Relative-position index (i = query token, j = key token; token 0 = cls, token 1 + y W + x = patch (y, x), E = (2W-1)^2):
//   patch -> patch   (y_i - y_j + W-1) (2W-1) + (x_i - x_j + W-1)  =  code(i) - code(j) + 2W(W-1)   with code(t) = y (2W-1) + x
//   cls -> any  E,   any -> cls  E + 1,   cls -> cls  E + 2
// The patch term is linear in one integer per token, so the kernels keep code(t) of every key in LDS beside the head's column of the
// bias table (at most 732 fp32) and never see a T x T index array.
#include "common.hpp"
#include "kernels.hpp"
#include "beit.hpp"
#include <math.h>

namespace effocr {
namespace {

constexpr int TB_MAX = (2 * BEIT_MAX_W - 1) * (2 * BEIT_MAX_W - 1) + 3;   // 732

// this head's column of the table and code(t) of every token slot (0 for cls and for the padded slots) -> LDS
__device__ __forceinline__ void stage_bias(const float* __restrict__ table, int heads, int h, int W, int T, int slots, float* tb, int* code) {
  const int entries = beit_table_entries(W);
  for (int r = threadIdx.x; r < entries; r += blockDim.x) tb[r] = table[r * heads + h];
  for (int t = threadIdx.x; t < slots; t += blockDim.x) {
    const int p = t - 1, y = p / W, x = p - y * W;
    code[t] = (t >= 1 && t < T) ? y * (2 * W - 1) + x : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// 16-bit modes.  One workgroup (4 waves) per (image, head), the row-major form of vit_ops.hip's attn_mfma_kernel: K (144-B padded
// rows) and V^T (packed key pairs) are staged once in LDS, each wave owns 32-query blocks, the scores are computed swapped
// (S^T = K Q^T, v_mfma_f32_32x32x16) so that a lane holds one query and all of its keys — register r of key tile kt is key
// kt*32 + (r&3) + 8*(r>>2) + 4*half — and the un-normalised P fragment feeds O^T = V^T P^T as it falls out.  New here: every score
// becomes fmaf(s, 1/8, table[index]) before the row maximum (so the scale can no longer ride in the exponent constant: exp2 takes
// log2(e) alone), and the padded keys are masked after the bias.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename E, int NKT>
__global__ __launch_bounds__(256, 2) void beit_attn_mfma_kernel(const E* __restrict__ qkv, const float* __restrict__ table,
                                                                E* __restrict__ out, int W, int T, int heads) {
  typedef typename Op16<E>::V8 V8;
  constexpr int TP = 32 * NKT;
  constexpr int KROW = 144;                 // bytes per K row: 64 elements + 16 B pad
  constexpr int VS = TP / 2 + 6;            // dwords per V^T row (even, VS/2 odd -> conflict-free b64 reads)
  __shared__ __attribute__((aligned(16))) char smem[TP * KROW + 64 * VS * 4];
  __shared__ __attribute__((aligned(16))) int sC[TP];
  __shared__ float tb[TB_MAX];
  char* sK = smem;
  uint32_t* sV = reinterpret_cast<uint32_t*>(smem + TP * KROW);

  const int tid = threadIdx.x, lane = tid & 63, r31 = lane & 31, half = lane >> 5;
  const int w = wave_id();
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int D = heads * 64;
  const int64_t ld = 3 * (int64_t)D;
  const int64_t tok0 = (int64_t)b * T;
  auto qkv_ptr = [&](int t, int sec, int c8) -> const u32x4* {
    return reinterpret_cast<const u32x4*>(qkv + (tok0 + t) * ld + sec * D + h * 64 + c8 * 8);
  };
  auto load_q = [&](V8 (&q)[4], int qb) {
    int tq = qb * 32 + r31;
    tq = tq < T ? tq : T - 1;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) q[ks] = __builtin_bit_cast(V8, *qkv_ptr(tq, 0, 2 * ks + half));
  };
  // K rows (zero rows beyond T) and V -> registers -> LDS; every global load is issued before the first LDS write
  constexpr int NKI = TP * 8 / 256;
  constexpr int NVI = ((TP / 2) * 8 + 255) / 256;
  u32x4 kreg[NKI], v0reg[NVI], v1reg[NVI];
  V8 qf[4];
  if (w * 32 < T) load_q(qf, w);
#pragma unroll
  for (int i = 0; i < NKI; ++i) {
    const int id = tid + 256 * i, t = id >> 3, c = id & 7;
    kreg[i] = u32x4{0u, 0u, 0u, 0u};
    if (t < T) kreg[i] = *qkv_ptr(t, 1, c);
  }
#pragma unroll
  for (int i = 0; i < NVI; ++i) {
    const int id = tid + 256 * i, tp = id >> 3, c = id & 7, t0 = 2 * tp;
    v0reg[i] = u32x4{0u, 0u, 0u, 0u}; v1reg[i] = u32x4{0u, 0u, 0u, 0u};
    if (t0 < T) v0reg[i] = *qkv_ptr(t0, 2, c);
    if (t0 + 1 < T) v1reg[i] = *qkv_ptr(t0 + 1, 2, c);
  }
  stage_bias(table, heads, h, W, T, TP, tb, sC);
#pragma unroll
  for (int i = 0; i < NKI; ++i) {
    const int id = tid + 256 * i, t = id >> 3, c = id & 7;
    *reinterpret_cast<u32x4*>(sK + t * KROW + c * 16) = kreg[i];
  }
#pragma unroll
  for (int i = 0; i < NVI; ++i) {
    const int id = tid + 256 * i, tp = id >> 3, c = id & 7;
    if (id < (TP / 2) * 8) {                // V transposed: dword (d, tp) = {V[2tp][d], V[2tp+1][d]}
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const uint32_t a = v0reg[i][jj], bq = v1reg[i][jj];
        sV[(c * 8 + 2 * jj) * VS + tp] = (a & 0xffffu) | (bq << 16);
        sV[(c * 8 + 2 * jj + 1) * VS + tp] = (a >> 16) | (bq & 0xffff0000u);
      }
    }
  }
  __syncthreads();

  const int EE = (2 * W - 1) * (2 * W - 1), off = 2 * W * (W - 1);
  constexpr float LOG2E = 1.44269504088896340736f;
  for (int qb = w; qb * 32 < T; qb += 4) {
    int tq = qb * 32 + r31;
    const bool qvalid = tq < T;
    tq = qvalid ? tq : T - 1;

    f32x16 s[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const V8 kf = *reinterpret_cast<const V8*>(sK + (kt * 32 + r31) * KROW + (2 * ks + half) * 16);
        s[kt] = Op16<E>::mfma(kf, qf[ks], s[kt]);
      }
    }
    // the query fragments are dead from here: the next block's arrive under this block's softmax and P V
    __builtin_amdgcn_sched_barrier(0);
    if ((qb + 4) * 32 < T) load_q(qf, qb + 4);
    // scale + bias, mask of the padded keys, row max
    const bool qcls = tq == 0;
    const int base = sC[tq] + off;
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int key0 = kt * 32 + 8 * r4 + 4 * half;
        const int ck[4] = {sC[key0], sC[key0 + 1], sC[key0 + 2], sC[key0 + 3]};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * r4 + e;
          int idx = qcls ? EE : base - ck[e];
          if (kt == 0 && r == 0) idx = half == 0 ? (qcls ? EE + 2 : EE + 1) : idx;     // key 0 = cls
          float v = fmaf(s[kt][r], 0.125f, tb[idx]);
          if (kt == NKT - 1 && key0 + e >= T) v = -INFINITY;
          s[kt][r] = v;
          mx = fmaxf(mx, v);
        }
      }
      __builtin_amdgcn_sched_barrier(0);     // one tile's table lookups at a time (register pressure)
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    f32x16 o[2];
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
    float l = 0.f;
    const float mxc = mx * LOG2E;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        V8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[kt][8 * m + j], LOG2E, -mxc));
          l += p;
          pf[j] = (E)p;
        }
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const uint32_t* vp = sV + (db * 32 + r31) * VS + (kt * 16 + 8 * m + 2 * half);
          const u32x2 lo = *reinterpret_cast<const u32x2*>(vp);
          const u32x2 hi = *reinterpret_cast<const u32x2*>(vp + 4);
          const u32x4 vv = {lo[0], lo[1], hi[0], hi[1]};
          o[db] = Op16<E>::mfma(__builtin_bit_cast(V8, vv), pf, o[db]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);     // one tile's exp / V^T reads at a time (register pressure)
    }
    l += __shfl_xor(l, 32, 64);
    if (qvalid) {
      const float inv = 1.0f / l;
      E* orow = out + (tok0 + tq) * D + h * 64;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const int d = db * 32 + 8 * q4 + 4 * half;
          *reinterpret_cast<u32x2*>(orow + d) = pack4<E>(o[db][4 * q4] * inv, o[db][4 * q4 + 1] * inv, o[db][4 * q4 + 2] * inv, o[db][4 * q4 + 3] * inv);
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// fp32 mode: one thread per query, K and V of the (image, head) in LDS (broadcast reads), online softmax in fp32 — the style of
// vit_ops.hip's attn_f32_kernel with the bias added to every score.  The parity path, not a throughput kernel.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int ATT32_T = BEIT_MAX_W * BEIT_MAX_W + 1;     // 197
__global__ __launch_bounds__(256) void beit_attn_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ table,
                                                            float* __restrict__ out, int W, int T, int heads) {
  __shared__ __attribute__((aligned(16))) float sK[ATT32_T * 64];
  __shared__ __attribute__((aligned(16))) float sV[ATT32_T * 64];
  __shared__ int sC[ATT32_T];
  __shared__ float tb[TB_MAX];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int D = heads * 64;
  const int64_t ld = 3 * (int64_t)D;
  const float* base = qkv + (int64_t)b * T * ld + h * 64;
  for (int id = tid; id < T * 16; id += 256) {
    const int t = id >> 4, c = id & 15;
    *reinterpret_cast<f32x4*>(sK + t * 64 + c * 4) = *reinterpret_cast<const f32x4*>(base + (int64_t)t * ld + D + c * 4);
    *reinterpret_cast<f32x4*>(sV + t * 64 + c * 4) = *reinterpret_cast<const f32x4*>(base + (int64_t)t * ld + 2 * D + c * 4);
  }
  stage_bias(table, heads, h, W, T, T, tb, sC);
  __syncthreads();
  const int EE = (2 * W - 1) * (2 * W - 1), off = 2 * W * (W - 1);
  for (int tq = tid; tq < T; tq += 256) {
    float q[64], o[64];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(base + (int64_t)tq * ld + c * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { q[c * 4 + e] = v[e]; o[c * 4 + e] = 0.f; }
    }
    const bool qcls = tq == 0;
    const int qbase = sC[tq] + off;
    float mx = -INFINITY, l = 0.f;
    for (int key = 0; key < T; ++key) {
      float sc = 0.f;
#pragma unroll
      for (int d = 0; d < 64; ++d) sc = fmaf(q[d], sK[key * 64 + d], sc);
      const int idx = key == 0 ? (qcls ? EE + 2 : EE + 1) : (qcls ? EE : qbase - sC[key]);
      sc = fmaf(sc, 0.125f, tb[idx]);
      const float mn = fmaxf(mx, sc);
      const float alpha = expf(mx - mn);
      const float p = expf(sc - mn);
      l = l * alpha + p;
#pragma unroll
      for (int d = 0; d < 64; ++d) o[d] = fmaf(p, sV[key * 64 + d], o[d] * alpha);
      mx = mn;
    }
    const float inv = 1.0f / l;
    float* orow = out + ((int64_t)b * T + tq) * D + h * 64;
#pragma unroll
    for (int c = 0; c < 16; ++c)
      *reinterpret_cast<f32x4*>(orow + c * 4) = f32x4{o[c * 4] * inv, o[c * 4 + 1] * inv, o[c * 4 + 2] * inv, o[c * 4 + 3] * inv};
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// head: mean of the T - 1 patch tokens (ascending token order) -> LayerNorm fc_norm (two-pass) -> (F.normalize) -> emb.  One crop per
// workgroup of D / 4 threads (a multiple of 32), thread t holds channels 4t .. 4t+3; a block sum is xor-shuffles inside each 32-lane
// half, then the halves through LDS in a fixed order.
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_sum(float v, float* hs, int halves) {      // two barriers: every thread must call it
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 31) == 0) hs[threadIdx.x >> 5] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < halves; ++i) t += hs[i];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(256) void beit_head_kernel(const float* __restrict__ x, int T, int D, const float* __restrict__ lnw,
                                                         const float* __restrict__ lnb, float eps, int l2norm, float* __restrict__ emb,
                                                         int* __restrict__ status) {
  __shared__ float hs[8];
  const int c4 = 4 * threadIdx.x, halves = blockDim.x >> 5;
  const int64_t b = blockIdx.x;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  for (int t = 1; t < T; ++t) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(x + (b * T + t) * (int64_t)D + c4);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += r[e];
  }
  const float invP = 1.0f / (float)(T - 1), invD = 1.0f / (float)D;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] *= invP;
  const float mean = block_sum((v[0] + v[1]) + (v[2] + v[3]), hs, halves) * invD;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] -= mean;
  const float var = block_sum((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]), hs, halves) * invD;
  const float rstd = 1.0f / sqrtf(var + eps);
  const f32x4 g = *reinterpret_cast<const f32x4*>(lnw + c4), bt = *reinterpret_cast<const f32x4*>(lnb + c4);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = v[e] * rstd * g[e] + bt[e];
  if (l2norm) {
    const float ss = block_sum((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]), hs, halves);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);            // F.normalize: x / max(||x||, eps)
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] / nrm;
  }
  bool bad = false;
#pragma unroll
  for (int e = 0; e < 4; ++e) bad |= !(fabsf(v[e]) <= 3.0e38f);
  *reinterpret_cast<f32x4*>(emb + b * D + c4) = v;
  if (status && bad) atomicOr(status, 1);
}

template <typename E>
int launch_attn16(const E* qkv, const float* table, E* out, int B, int W, int T, int heads, hipStream_t s) {
  const dim3 grid((unsigned)(B * heads)), blk(256);
  switch ((T + 31) / 32) {
    case 1: hipLaunchKernelGGL((beit_attn_mfma_kernel<E, 1>), grid, blk, 0, s, qkv, table, out, W, T, heads); break;
    case 2: hipLaunchKernelGGL((beit_attn_mfma_kernel<E, 2>), grid, blk, 0, s, qkv, table, out, W, T, heads); break;
    case 3: hipLaunchKernelGGL((beit_attn_mfma_kernel<E, 3>), grid, blk, 0, s, qkv, table, out, W, T, heads); break;
    case 4: hipLaunchKernelGGL((beit_attn_mfma_kernel<E, 4>), grid, blk, 0, s, qkv, table, out, W, T, heads); break;
    case 5: hipLaunchKernelGGL((beit_attn_mfma_kernel<E, 5>), grid, blk, 0, s, qkv, table, out, W, T, heads); break;
    case 6: hipLaunchKernelGGL((beit_attn_mfma_kernel<E, 6>), grid, blk, 0, s, qkv, table, out, W, T, heads); break;
    case 7: hipLaunchKernelGGL((beit_attn_mfma_kernel<E, 7>), grid, blk, 0, s, qkv, table, out, W, T, heads); break;
    default: return fail(EFFOCR_EUNSUPPORTED, "beit_attention: more than 224 tokens");
  }
  return check_launch("beit_attention");
}

}  // namespace

int beit_attention(int prec, const void* qkv, const float* table, int B, int W, int heads, void* out, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (W < 1 || W > BEIT_MAX_W || heads < 1) return fail(EFFOCR_EUNSUPPORTED, "beit_attention: 1 <= W <= 14 patches per side and heads >= 1 required");
  if ((int64_t)B * heads >= (int64_t)1 << 31) return fail(EFFOCR_EUNSUPPORTED, "beit_attention: too many (image, head) pairs for one launch");
  const int T = W * W + 1;
  switch (prec) {
    case PREC_BF16: return launch_attn16<__bf16>(static_cast<const __bf16*>(qkv), table, static_cast<__bf16*>(out), B, W, T, heads, s);
    case PREC_FP16: return launch_attn16<_Float16>(static_cast<const _Float16*>(qkv), table, static_cast<_Float16*>(out), B, W, T, heads, s);
    case PREC_FP32:
      hipLaunchKernelGGL(beit_attn_f32_kernel, dim3((unsigned)(B * heads)), dim3(256), 0, s, static_cast<const float*>(qkv), table,
                         static_cast<float*>(out), W, T, heads);
      return check_launch("beit_attention_f32");
  }
  return fail(EFFOCR_EINVAL, "beit_attention: unknown precision");
}

int beit_head(const float* x, int B, int T, int D, const float* lnw, const float* lnb, float eps, int l2norm, float* emb, int* status,
              hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (D % 128 || D > 1024 || T < 2) return fail(EFFOCR_EUNSUPPORTED, "beit_head: D must be a multiple of 128 (<= 1024) and T >= 2");
  hipLaunchKernelGGL(beit_head_kernel, dim3((unsigned)B), dim3(D / 4), 0, s, x, T, D, lnw, lnb, eps, l2norm, emb, status);
  return check_launch("beit_head");
}

}  // namespace effocr
