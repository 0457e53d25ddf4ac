// Patch-8 ViT kernels on gfx950 (timm vit_small_patch8_224 / vit_base_patch8_224 semantics; vit8_api.hip: vit8_forward).  Part of
// libeffocr_vit8.so only.  The LayerNorms, the cls row and the final norm come from vit_ops.hip, the linears from gemm.hip / gemm2.hip;
// what the 785-token crops add is an attention that streams its key tiles (the whole-row kernels of vit_ops.hip, qkvattn.hip and
// beit.hip stop at 224 tokens) and an im2col for 8x8 patches.  vit8.hpp states the interface, the walk and the rounding points.
#include "common.hpp"
#include "kernels.hpp"
#include "vit8.hpp"
#include <math.h>

namespace effocr {
namespace {

constexpr float LOG2E = 1.44269504088896340736f;

// ---------------------------------------------------------------------------------------------------------------------------
// 16-bit modes.  One workgroup (4 waves) per (crop, head, block of 128 queries); wave w owns queries 32 w .. 32 w + 31 of the block and
// keeps their q fragments, the running maximum m, the running sum l and O^T (2 x f32x16) in registers for the whole walk.  A key tile is
// 64 keys: K (144-B padded rows) and V^T (packed key pairs) in LDS, double-buffered — the next tile's global loads are issued before this
// tile's MFMAs and written to the other buffer after them, one barrier per tile.  As in beit.hip the scores are computed swapped
// (S^T = K Q^T, v_mfma_f32_32x32x16), so a lane holds one query and 16 of the 32 keys of a sub-tile — register r is key
// (r&3) + 8*(r>>2) + 4*half — the row maximum is lane-local plus one cross-half exchange, and the rounded P fragment feeds
// O^T = V^T P^T as it falls out.  The scale 1/8 rides in the exponent constant: m is kept in raw-score units.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(256, 2) void vit8_attn_mfma_kernel(const E* __restrict__ qkv, E* __restrict__ out, int T, int heads, int nqb) {
  typedef typename Op16<E>::V8 V8;
  constexpr int KT = VIT8_KTILE16;
  constexpr int KROW = 144;                 // bytes per K row: 64 elements + 16 B pad
  constexpr int VS = KT / 2 + 6;            // dwords per V^T row (even, VS/2 odd -> conflict-free b64 reads)
  constexpr int KBYTES = KT * KROW, BUF = KBYTES + 64 * VS * 4;
  static_assert(KT == 64 && VIT8_QBLK == 128, "the loaders below move one 64-key tile with 256 threads; 4 waves x 32 queries");
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];

  const int tid = threadIdx.x, lane = tid & 63, r31 = lane & 31, half = lane >> 5;
  const int w = wave_id();
  const int qb = blockIdx.x % nqb, bh = blockIdx.x / nqb;
  const int b = bh / heads, h = bh - b * heads;
  const int D = heads * 64;
  const int64_t ld = 3 * (int64_t)D;
  const int64_t tok0 = (int64_t)b * T;
  auto qkv_ptr = [&](int t, int sec, int c8) -> const u32x4* {
    return reinterpret_cast<const u32x4*>(qkv + (tok0 + t) * ld + sec * D + h * 64 + c8 * 8);
  };
  const int q0 = qb * VIT8_QBLK + w * 32;
  const bool active = q0 < T;               // wave-uniform: a wave whose 32 query slots all lie beyond T only helps to stage the tiles
  int tq = q0 + r31;
  const bool qvalid = tq < T;
  tq = qvalid ? tq : T - 1;
  V8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) qf[ks] = __builtin_bit_cast(V8, *qkv_ptr(tq, 0, 2 * ks + half));

  // one tile = 64 K rows (2 x 16 B per thread) and 32 V row pairs (2 x 16 B per thread); rows at or beyond T are zeros
  u32x4 kreg[2], v0reg, v1reg;
  const int lt = tid >> 3, lc = tid & 7;
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = k0 + lt + 32 * i;
      kreg[i] = u32x4{0u, 0u, 0u, 0u};
      if (t < T) kreg[i] = *qkv_ptr(t, 1, lc);
    }
    const int t0 = k0 + 2 * lt;
    v0reg = u32x4{0u, 0u, 0u, 0u}; v1reg = u32x4{0u, 0u, 0u, 0u};
    if (t0 < T) v0reg = *qkv_ptr(t0, 2, lc);
    if (t0 + 1 < T) v1reg = *qkv_ptr(t0 + 1, 2, lc);
  };
  auto swrite = [&](char* buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4*>(buf + (lt + 32 * i) * KROW + lc * 16) = kreg[i];
    uint32_t* sV = reinterpret_cast<uint32_t*>(buf + KBYTES);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {        // V transposed: dword (d, tp) = {V[2tp][d], V[2tp+1][d]}
      const uint32_t a = v0reg[jj], bq = v1reg[jj];
      sV[(lc * 8 + 2 * jj) * VS + lt] = (a & 0xffffu) | (bq << 16);
      sV[(lc * 8 + 2 * jj + 1) * VS + lt] = (a >> 16) | (bq & 0xffff0000u);
    }
  };

  constexpr float C = 0.125f * LOG2E;
  float m = -INFINITY, l = 0.f;
  f32x16 o[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;

  const int nt = (T + KT - 1) / KT;
  gload(0);
  swrite(smem);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const char* cur = smem + (t & 1) * BUF;
    const bool more = t + 1 < nt;
    if (more) gload((t + 1) * KT);
    if (active) {
      f32x16 s[2];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[sub][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const V8 kf = *reinterpret_cast<const V8*>(cur + (sub * 32 + r31) * KROW + (2 * ks + half) * 16);
          s[sub] = Op16<E>::mfma(kf, qf[ks], s[sub]);
        }
      }
      const int k0 = t * KT;
      if (k0 + KT > T) {                    // the last tile: keys at or beyond T score -inf -> weight exactly 0
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (k0 + sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * half >= T) s[sub][r] = -INFINITY;
      }
      float mx = -INFINITY;
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[sub][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      // key k0 < T is live in every tile, so mn is finite; m = -inf before the first tile makes alpha exactly 0
      const float mn = fmaxf(m, mx);
      const float alpha = __builtin_amdgcn_exp2f((m - mn) * C);
      const float mc = mn * C;
      m = mn;
      l *= alpha;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
      const uint32_t* sV = reinterpret_cast<const uint32_t*>(cur + KBYTES);
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int mm = 0; mm < 2; ++mm) {
          V8 pf;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float p = __builtin_amdgcn_exp2f(fmaf(s[sub][8 * mm + j], C, -mc));
            l += p;
            pf[j] = (E)p;
          }
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            const uint32_t* vp = sV + (db * 32 + r31) * VS + (sub * 16 + 8 * mm + 2 * half);
            const u32x2 lo = *reinterpret_cast<const u32x2*>(vp);
            const u32x2 hi = *reinterpret_cast<const u32x2*>(vp + 4);
            const u32x4 vv = {lo[0], lo[1], hi[0], hi[1]};
            o[db] = Op16<E>::mfma(__builtin_bit_cast(V8, vv), pf, o[db]);
          }
        }
      }
    }
    if (more) swrite(smem + ((t + 1) & 1) * BUF);
    __syncthreads();
  }
  l += __shfl_xor(l, 32, 64);
  if (active && qvalid) {
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

// ---------------------------------------------------------------------------------------------------------------------------
// fp32 mode: one workgroup of 128 threads per (crop, head, block of 128 queries), one query per thread (q and O in registers); a key tile
// is 32 keys, K and V in LDS (broadcast reads).  The same walk: tile maximum, one rescale per tile, expf.  The parity path, not a
// throughput kernel.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VIT8_QBLK) void vit8_attn_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int T, int heads, int nqb) {
  constexpr int KT = VIT8_KTILE32;
  __shared__ __attribute__((aligned(16))) float sK[KT * 64];
  __shared__ __attribute__((aligned(16))) float sV[KT * 64];
  const int tid = threadIdx.x;
  const int qb = blockIdx.x % nqb, bh = blockIdx.x / nqb;
  const int b = bh / heads, h = bh - b * heads;
  const int D = heads * 64;
  const int64_t ld = 3 * (int64_t)D;
  const float* base = qkv + (int64_t)b * T * ld + h * 64;
  int tq = qb * VIT8_QBLK + tid;
  const bool qvalid = tq < T;
  tq = qvalid ? tq : T - 1;
  float q[64], o[64];
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(base + (int64_t)tq * ld + c * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { q[c * 4 + e] = v[e]; o[c * 4 + e] = 0.f; }
  }
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < T; k0 += KT) {
    __syncthreads();                        // every thread is done with the previous tile
    for (int id = tid; id < KT * 16; id += VIT8_QBLK) {
      const int t = id >> 4, c = id & 15;
      f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
      if (k0 + t < T) {
        kv = *reinterpret_cast<const f32x4*>(base + (int64_t)(k0 + t) * ld + D + c * 4);
        vv = *reinterpret_cast<const f32x4*>(base + (int64_t)(k0 + t) * ld + 2 * D + c * 4);
      }
      *reinterpret_cast<f32x4*>(sK + t * 64 + c * 4) = kv;
      *reinterpret_cast<f32x4*>(sV + t * 64 + c * 4) = vv;
    }
    __syncthreads();
    float s[KT];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < KT; ++j) {
      float sc = 0.f;
#pragma unroll
      for (int d = 0; d < 64; ++d) sc = fmaf(q[d], sK[j * 64 + d], sc);
      sc = k0 + j < T ? sc * 0.125f : -INFINITY;          // keys at or beyond T: weight exactly 0
      s[j] = sc;
      mx = fmaxf(mx, sc);
    }
    const float mn = fmaxf(m, mx);                        // finite: key k0 < T is live
    const float alpha = expf(m - mn);
    m = mn;
    l *= alpha;
#pragma unroll
    for (int d = 0; d < 64; ++d) o[d] *= alpha;
#pragma unroll
    for (int j = 0; j < KT; ++j) {
      const float p = expf(s[j] - mn);
      l += p;
#pragma unroll
      for (int d = 0; d < 64; ++d) o[d] = fmaf(p, sV[j * 64 + d], o[d]);
    }
  }
  if (qvalid) {
    const float inv = 1.0f / l;
    float* orow = out + ((int64_t)b * T + tq) * D + h * 64;
#pragma unroll
    for (int c = 0; c < 16; ++c)
      *reinterpret_cast<f32x4*>(orow + c * 4) = f32x4{o[c * 4] * inv, o[c * 4 + 1] * inv, o[c * 4 + 2] * inv, o[c * 4 + 3] * inv};
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// im2col for the 8x8 / stride-8 patch-embedding conv: x [B,3,H,W] fp32 NCHW -> rows [(img,py,px)][k = c*64 + ky*8 + kx] in the GEMM
// operand type (k order = the conv weight's own [D,3,8,8] flattening).  One thread per 8 pixels of one patch row.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename TO>
__global__ __launch_bounds__(256) void im2col8_kernel(const float* __restrict__ x, int B, int H, int W, TO* __restrict__ out) {
  const int PH = H / 8, PW = W / 8;
  const int64_t total = (int64_t)B * PH * PW * 24;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= total) return;
  const int k8 = (int)(id % 24);
  const int64_t mrow = id / 24;
  const int px = (int)(mrow % PW), py = (int)((mrow / PW) % PH);
  const int64_t img = mrow / ((int64_t)PW * PH);
  const int c = k8 >> 3, ky = k8 & 7;
  const float* src = x + ((img * 3 + c) * H + (py * 8 + ky)) * (int64_t)W + px * 8;
  TO* dst = out + mrow * VIT8_PATCH_K + k8 * 8;
  const f32x4 a = *reinterpret_cast<const f32x4*>(src);
  const f32x4 b = *reinterpret_cast<const f32x4*>(src + 4);
  if constexpr (sizeof(TO) == 4) {
    *reinterpret_cast<f32x4*>(dst) = a;
    *reinterpret_cast<f32x4*>(dst + 4) = b;
  } else {
    const u32x2 lo = pack4<TO>(a[0], a[1], a[2], a[3]);
    const u32x2 hi = pack4<TO>(b[0], b[1], b[2], b[3]);
    *reinterpret_cast<u32x4*>(dst) = u32x4{lo[0], lo[1], hi[0], hi[1]};
  }
}

template <typename TO>
int launch_im2col8(const float* x, int B, int H, int W, TO* out, hipStream_t s) {
  const int64_t total = (int64_t)B * (H / 8) * (W / 8) * 24;
  hipLaunchKernelGGL((im2col8_kernel<TO>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, B, H, W, out);
  return check_launch("im2col8");
}

}  // namespace

int vit8_attention(int prec, const void* qkv, int B, int T, int heads, void* out, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (T < 1 || T > VIT8_MAX_T || heads < 1) return fail(EFFOCR_EUNSUPPORTED, "vit8_attention: 1 <= T <= 1024 tokens and heads >= 1 required");
  const int nqb = (T + VIT8_QBLK - 1) / VIT8_QBLK;
  if ((int64_t)B * heads * nqb >= (int64_t)1 << 31) return fail(EFFOCR_EUNSUPPORTED, "vit8_attention: too many (crop, head, query block) triples for one launch");
  const dim3 grid((unsigned)(B * heads * nqb));
  switch (prec) {
    case PREC_BF16:
      hipLaunchKernelGGL((vit8_attn_mfma_kernel<__bf16>), grid, dim3(256), 0, s, static_cast<const __bf16*>(qkv), static_cast<__bf16*>(out), T, heads, nqb);
      return check_launch("vit8_attention");
    case PREC_FP16:
      hipLaunchKernelGGL((vit8_attn_mfma_kernel<_Float16>), grid, dim3(256), 0, s, static_cast<const _Float16*>(qkv), static_cast<_Float16*>(out), T, heads, nqb);
      return check_launch("vit8_attention");
    case PREC_FP32:
      hipLaunchKernelGGL(vit8_attn_f32_kernel, grid, dim3(VIT8_QBLK), 0, s, static_cast<const float*>(qkv), static_cast<float*>(out), T, heads, nqb);
      return check_launch("vit8_attention_f32");
  }
  return fail(EFFOCR_EINVAL, "vit8_attention: unknown precision");
}

int vit8_patch_embed(int prec, const float* x, int B, int img, int D, const void* w, const float* bias, const float* cls_pos0,
                     const float* pos, void* col, float* out, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (img < VIT8_PATCH || img > VIT8_PATCH * VIT8_MAX_W || img % VIT8_PATCH) return fail(EFFOCR_EINVAL, "vit8_patch_embed: img_size must be a multiple of 8 from 8 to 224");
  const int P = (img / VIT8_PATCH) * (img / VIT8_PATCH);
  if ((int64_t)B * (P + 1) * D >= (int64_t)1 << 31) return fail(EFFOCR_EUNSUPPORTED, "vit8_patch_embed: too many crops for 32-bit GEMM indices");
  int rc;
  switch (prec) {
    case PREC_BF16: rc = launch_im2col8<__bf16>(x, B, img, img, static_cast<__bf16*>(col), s); break;
    case PREC_FP16: rc = launch_im2col8<_Float16>(x, B, img, img, static_cast<_Float16*>(col), s); break;
    case PREC_FP32: rc = launch_im2col8<float>(x, B, img, img, static_cast<float*>(col), s); break;
    default: return fail(EFFOCR_EINVAL, "vit8_patch_embed: unknown precision");
  }
  if (rc) return rc;
  GemmArgs g{};
  g.X = col; g.ldx = VIT8_PATCH_K; g.W = w; g.ldw = VIT8_PATCH_K; g.bias = bias; g.out = out; g.ldo = D;
  g.M = B * P; g.N = D; g.K = VIT8_PATCH_K; g.pos = pos; g.P = P;
  rc = gemm2_supported(prec, D, VIT8_PATCH_K) ? gemm2_nt(prec, EPI_PATCH, g, s) : gemm_nt(prec, EPI_PATCH, g, s);
  if (rc) return rc;
  return set_cls_rows(cls_pos0, out, B, P + 1, D, 0, nullptr, s);
}

}  // namespace effocr
