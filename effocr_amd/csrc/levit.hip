// LeViT encoder kernels on gfx950 (timm levit_128s .. levit_384 semantics; levit_api.hip: levit_forward).  Part of libeffocr_levit.so
// only.  The linears are gemm.hip / gemm2.hip; what LeViT adds is an attention whose queries and keys (16 or 32 wide) are narrower than
// its values (32 to 128 wide), with an additive per-head bias looked up by (|dy|, |dx|) and a form whose strided queries attend to the
// full key grid, a 3x3 stride-2 stem convolution, and the small row kernels between the GEMMs.  Contracts and rounding points: levit.hpp.
#include "common.hpp"
#include "kernels.hpp"
#include "levit.hpp"
#include <math.h>

namespace effocr {
namespace {

constexpr int TK_MAX = LEVIT_MAX_R * LEVIT_MAX_R;        // 196 keys
constexpr int TP_MAX = (TK_MAX + LEVIT_KTILE - 1) / LEVIT_KTILE * LEVIT_KTILE;   // 224 key slots

__device__ __forceinline__ float hardswish(float x) { return x * fminf(fmaxf(x + 3.0f, 0.0f), 6.0f) / 6.0f; }

// ---------------------------------------------------------------------------------------------------------------------------
// 16-bit modes.  One workgroup (4 waves) per (crop, head, VDB-wide slice of the values) — beit.hip's attention with narrow K rows, a
// key loop that runs to this launch's tile count instead of a template's, and the online softmax that loop needs.  K (rows padded by
// 16 B) and V^T (packed key pairs) are staged once; the scores are computed swapped (S^T = K Q^T, v_mfma_f32_32x32x16) so that a lane
// holds one query and 16 of a tile's keys — register r is key 32 kt + (r & 3) + 8 (r >> 2) + 4 half — and the P fragment feeds
// O^T = V^T P^T as it falls out.  kd = 16 is one MFMA step per key tile, kd = 32 two.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename E, int KD, int VDB>
__global__ __launch_bounds__(256) void levit_attn_mfma_kernel(LevitQKV a, const float* __restrict__ bias, E* __restrict__ out, int R, int Rq,
                                                              int stride, int heads, int vd, int act, float scale) {
  typedef typename Op16<E>::V8 V8;
  constexpr int KROW = KD * 2 + 16;         // bytes per K row
  constexpr int KC = KD / 8;                // 16-byte chunks per K row
  constexpr int VC = VDB / 8;               // ... per slice of a V row
  constexpr int VS = TP_MAX / 2 + 6;        // dwords per V^T row (even, VS / 2 odd -> conflict-free b64 reads)
  constexpr int NDB = VDB / 32;
  __shared__ __attribute__((aligned(16))) char sK[TP_MAX * KROW];
  __shared__ __attribute__((aligned(16))) uint32_t sV[VDB * VS];
  __shared__ int sC[TP_MAX];
  __shared__ float tb[TK_MAX];

  const int tid = threadIdx.x, lane = tid & 63, r31 = lane & 31, half = lane >> 5;
  const int w = wave_id();
  const int nvs = vd / VDB;
  const int vs = blockIdx.x % nvs, bh = blockIdx.x / nvs;
  const int b = bh / heads, h = bh - b * heads;
  const int Tk = R * R, Tq = Rq * Rq;
  const int nkt = (Tk + LEVIT_KTILE - 1) / LEVIT_KTILE, TP = nkt * LEVIT_KTILE;
  const E* qb_ = static_cast<const E*>(a.q) + (int64_t)b * Tq * a.ldq + h * a.qhs + a.qoff;
  const E* kb_ = static_cast<const E*>(a.kv) + (int64_t)b * Tk * a.ldkv + h * a.khs + a.koff;
  const E* vb_ = static_cast<const E*>(a.kv) + (int64_t)b * Tk * a.ldkv + h * a.khs + a.voff + vs * VDB;

  // K rows (zero rows from Tk on)
  for (int id = tid; id < TP * KC; id += 256) {
    const int t = id / KC, c = id - t * KC;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (t < Tk) v = *reinterpret_cast<const u32x4*>(kb_ + (int64_t)t * a.ldkv + c * 8);
    *reinterpret_cast<u32x4*>(sK + t * KROW + c * 16) = v;
  }
  // V transposed: dword (d, tp) = {V[2 tp][d], V[2 tp + 1][d]} (zeros from Tk on)
  for (int id = tid; id < (TP / 2) * VC; id += 256) {
    const int tp = id / VC, c = id - tp * VC, t0 = 2 * tp;
    u32x4 v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
    if (t0 < Tk) v0 = *reinterpret_cast<const u32x4*>(vb_ + (int64_t)t0 * a.ldkv + c * 8);
    if (t0 + 1 < Tk) v1 = *reinterpret_cast<const u32x4*>(vb_ + (int64_t)(t0 + 1) * a.ldkv + c * 8);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const uint32_t lo = v0[jj], hi = v1[jj];
      sV[(c * 8 + 2 * jj) * VS + tp] = (lo & 0xffffu) | (hi << 16);
      sV[(c * 8 + 2 * jj + 1) * VS + tp] = (lo >> 16) | (hi & 0xffff0000u);
    }
  }
  // this head's row of the bias table and (ky << 8 | kx) of every key slot (0 for the padded slots)
  for (int t = tid; t < TP; t += 256) {
    const int y = t / R;
    sC[t] = t < Tk ? (y << 8) | (t - y * R) : 0;
  }
  for (int i = tid; i < Tk; i += 256) tb[i] = bias[(int64_t)h * Tk + i];
  __syncthreads();

  constexpr float LOG2E = 1.44269504088896340736f;
  for (int qb = w; qb * LEVIT_QBLK < Tq; qb += 4) {
    int tq = qb * LEVIT_QBLK + r31;
    const bool qvalid = tq < Tq;
    tq = qvalid ? tq : Tq - 1;
    const int qyi = tq / Rq;
    const int qy = qyi * stride, qx = (tq - qyi * Rq) * stride;
    V8 qf[KD / 16];
#pragma unroll
    for (int ks = 0; ks < KD / 16; ++ks)
      qf[ks] = __builtin_bit_cast(V8, *reinterpret_cast<const u32x4*>(qb_ + (int64_t)tq * a.ldq + (2 * ks + half) * 8));

    f32x16 o[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int kt = 0; kt < nkt; ++kt) {
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KD / 16; ++ks) {
        const V8 kf = *reinterpret_cast<const V8*>(sK + (kt * 32 + r31) * KROW + (2 * ks + half) * 16);
        s = Op16<E>::mfma(kf, qf[ks], s);
      }
      // scale + bias, mask of the padded keys, tile maximum
      float tmax = -INFINITY;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int key0 = kt * 32 + 8 * r4 + 4 * half;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * r4 + e, c = sC[key0 + e];
          const int dy = abs(qy - (c >> 8)), dx = abs(qx - (c & 255));
          float v = fmaf(s[r], scale, tb[dy * R + dx]);
          if (key0 + e >= Tk) v = -INFINITY;
          s[r] = v;
          tmax = fmaxf(tmax, v);
        }
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
      const float mn = fmaxf(m, tmax);                       // every tile holds at least one live key: mn is finite unless a score is not
      const float alpha = __builtin_amdgcn_exp2f((m - mn) * LOG2E);
      l *= alpha;
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
      const float mc = mn * LOG2E;
#pragma unroll
      for (int mm = 0; mm < 2; ++mm) {
        V8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[8 * mm + j], LOG2E, -mc));
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
      m = mn;
    }
    l += __shfl_xor(l, 32, 64);
    if (qvalid) {
      const float inv = 1.0f / l;
      E* orow = out + ((int64_t)b * Tq + tq) * ((int64_t)heads * vd) + h * vd + vs * VDB;
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e] = o[db][4 * q4 + e] * inv;
            if (act) v[e] = hardswish(v[e]);
          }
          *reinterpret_cast<u32x2*>(orow + db * 32 + 8 * q4 + 4 * half) = pack4<E>(v[0], v[1], v[2], v[3]);
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// fp32 mode: one thread per (query, 32 values), keys and values read through the caches, online softmax key by key.  The parity path,
// not a throughput kernel.
// ---------------------------------------------------------------------------------------------------------------------------
template <int KD>
__global__ __launch_bounds__(256) void levit_attn_f32_kernel(LevitQKV a, const float* __restrict__ bias, float* __restrict__ out, int R, int Rq,
                                                             int stride, int heads, int vd, int act, float scale) {
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int Tk = R * R, Tq = Rq * Rq, nch = vd / 32;
  const float* qb_ = static_cast<const float*>(a.q) + (int64_t)b * Tq * a.ldq + h * a.qhs + a.qoff;
  const float* kb_ = static_cast<const float*>(a.kv) + (int64_t)b * Tk * a.ldkv + h * a.khs + a.koff;
  const float* vb_ = static_cast<const float*>(a.kv) + (int64_t)b * Tk * a.ldkv + h * a.khs + a.voff;
  const float* tb = bias + (int64_t)h * Tk;
  for (int id = threadIdx.x; id < Tq * nch; id += 256) {
    const int tq = id / nch, ch = id - tq * nch;
    const int qyi = tq / Rq;
    const int qy = qyi * stride, qx = (tq - qyi * Rq) * stride;
    float q[KD], o[32];
#pragma unroll
    for (int d = 0; d < KD; ++d) q[d] = qb_[(int64_t)tq * a.ldq + d];
#pragma unroll
    for (int d = 0; d < 32; ++d) o[d] = 0.f;
    float mx = -INFINITY, l = 0.f;
    for (int key = 0; key < Tk; ++key) {
      const float* kr = kb_ + (int64_t)key * a.ldkv;
      float sc = 0.f;
#pragma unroll
      for (int d = 0; d < KD; ++d) sc = fmaf(q[d], kr[d], sc);
      const int ky = key / R, kx = key - ky * R;
      sc = fmaf(sc, scale, tb[abs(qy - ky) * R + abs(qx - kx)]);
      const float mn = fmaxf(mx, sc);
      const float alpha = expf(mx - mn);
      const float p = expf(sc - mn);
      l = l * alpha + p;
      const float* vr = vb_ + (int64_t)key * a.ldkv + ch * 32;
#pragma unroll
      for (int d = 0; d < 32; ++d) o[d] = fmaf(p, vr[d], o[d] * alpha);
      mx = mn;
    }
    const float inv = 1.0f / l;
    float* orow = out + ((int64_t)b * Tq + tq) * ((int64_t)heads * vd) + h * vd + ch * 32;
#pragma unroll
    for (int d = 0; d < 32; ++d) {
      const float v = o[d] * inv;
      orow[d] = act ? hardswish(v) : v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// stem: direct 3x3 / stride 2 / pad 1 convolution, one thread per (output pixel, 4 output channels); neighbouring threads share the
// pixel (broadcast input reads) and read consecutive weights.  TI: input element (float = the NCHW crops), E: operand type the NCHW
// values are rounded to, TO: output element (E, or float for the residual stream).
// ---------------------------------------------------------------------------------------------------------------------------
template <typename E, bool NCHW, typename TO>
__global__ __launch_bounds__(256) void levit_conv_kernel(const void* __restrict__ in_, const float* __restrict__ wt, const float* __restrict__ bias,
                                                         TO* __restrict__ out, int B, int H, int Cin, int Cout, int OH, int act, int ldo) {
  const int ng = ldo / 4;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (int64_t)B * OH * OH * ng) return;
  const int g = (int)(id % ng);
  const int64_t pix = id / ng;
  const int ox = (int)(pix % OH), oy = (int)((pix / OH) % OH), b = (int)(pix / ((int64_t)OH * OH));
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (4 * g < Cout) {
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = 2 * oy - 1 + ky;
      if (iy < 0 || iy >= H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = 2 * ox - 1 + kx;
        if (ix < 0 || ix >= H) continue;
        const float* wr = wt + (int64_t)(ky * 3 + kx) * Cin * Cout + 4 * g;
        if constexpr (NCHW) {
          const float* in = static_cast<const float*>(in_);
          for (int c = 0; c < Cin; ++c) {
            const float v = (float)(E)in[(((int64_t)b * Cin + c) * H + iy) * H + ix];
            const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + (int64_t)c * Cout);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(v, wv[e], acc[e]);
          }
        } else {
          const E* in = static_cast<const E*>(in_) + (((int64_t)b * H + iy) * H + ix) * Cin;
          for (int c8 = 0; c8 < Cin; c8 += 8) {
            E xv[8];
            if constexpr (sizeof(E) == 2) {
              *reinterpret_cast<u32x4*>(xv) = *reinterpret_cast<const u32x4*>(in + c8);
            } else {
              *reinterpret_cast<u32x4*>(xv) = *reinterpret_cast<const u32x4*>(in + c8);
              *reinterpret_cast<u32x4*>(xv + 4) = *reinterpret_cast<const u32x4*>(in + c8 + 4);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float v = (float)xv[j];
              const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + (int64_t)(c8 + j) * Cout);
#pragma unroll
              for (int e = 0; e < 4; ++e) acc[e] = fmaf(v, wv[e], acc[e]);
            }
          }
        }
      }
    }
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + 4 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[e] += bv[e];
      if (act) acc[e] = hardswish(acc[e]);
    }
  }
  TO* o = out + pix * ldo + 4 * g;                         // channels from Cout on: zeros (the K padding of the next GEMM)
  if constexpr (sizeof(TO) == 4) *reinterpret_cast<f32x4*>(o) = acc;
  else *reinterpret_cast<u32x2*>(o) = pack4<TO>(acc[0], acc[1], acc[2], acc[3]);
}

template <typename E>
__global__ __launch_bounds__(256) void levit_cast_rows_kernel(const float* __restrict__ x, E* __restrict__ out, int B, int R, int Rq, int stride, int D) {
  const int d4 = D / 4, Tq = Rq * Rq;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (int64_t)B * Tq * d4) return;
  const int c = (int)(id % d4);
  const int64_t row = id / d4;
  const int b = (int)(row / Tq), i = (int)(row - (int64_t)b * Tq);
  const int qy = i / Rq, qx = i - qy * Rq;
  const int64_t src = (int64_t)b * R * R + (int64_t)qy * stride * R + qx * stride;
  const f32x4 v = *reinterpret_cast<const f32x4*>(x + src * D + 4 * c);
  if constexpr (sizeof(E) == 4) *reinterpret_cast<f32x4*>(out + row * D + 4 * c) = v;
  else *reinterpret_cast<u32x2*>(out + row * D + 4 * c) = pack4<E>(v[0], v[1], v[2], v[3]);
}

template <typename E>
__global__ __launch_bounds__(256) void levit_hardswish_kernel(E* __restrict__ buf, int64_t n4) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= n4) return;
  E* p = buf + 4 * id;
  if constexpr (sizeof(E) == 4) {
    f32x4 v = *reinterpret_cast<f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = hardswish(v[e]);
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
    E xv[4];
    *reinterpret_cast<u32x2*>(xv) = *reinterpret_cast<const u32x2*>(p);
    *reinterpret_cast<u32x2*>(p) = pack4<E>(hardswish((float)xv[0]), hardswish((float)xv[1]), hardswish((float)xv[2]), hardswish((float)xv[3]));
  }
}

// one crop per workgroup; a block sum is xor-shuffles inside each wave, then the four waves through LDS in a fixed order
__global__ __launch_bounds__(256) void levit_pool_kernel(const float* __restrict__ x, int T, int D, int ldx, int l2norm, float* __restrict__ emb,
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
      for (int t = 0; t < T; ++t) sum += x[(b * T + t) * (int64_t)ldx + c];
    v[k] = sum / (float)T;
    ss += v[k] * v[k];
  }
  if (l2norm) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 64);
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

template <typename E>
int launch_attn16(const LevitQKV& a, const float* bias, E* out, int B, int R, int Rq, int stride, int heads, int kd, int vd, int act, float scale,
                  hipStream_t s) {
  const dim3 blk(256);
  if (kd == 16 && vd == 32)
    hipLaunchKernelGGL((levit_attn_mfma_kernel<E, 16, 32>), dim3((unsigned)(B * heads)), blk, 0, s, a, bias, out, R, Rq, stride, heads, vd, act, scale);
  else if (kd == 16)
    hipLaunchKernelGGL((levit_attn_mfma_kernel<E, 16, 64>), dim3((unsigned)(B * heads * (vd / 64))), blk, 0, s, a, bias, out, R, Rq, stride, heads, vd, act, scale);
  else
    hipLaunchKernelGGL((levit_attn_mfma_kernel<E, 32, 64>), dim3((unsigned)(B * heads * (vd / 64))), blk, 0, s, a, bias, out, R, Rq, stride, heads, vd, act, scale);
  return check_launch("levit_attention");
}

template <typename E, typename TO>
int launch_conv(const void* in, int nchw, int B, int H, int Cin, const float* wt, const float* bias, int Cout, int OH, int act, TO* out, int ldo,
                hipStream_t s) {
  const int64_t n = (int64_t)B * OH * OH * (ldo / 4);
  const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
  if (nchw) hipLaunchKernelGGL((levit_conv_kernel<E, true, TO>), grid, blk, 0, s, in, wt, bias, out, B, H, Cin, Cout, OH, act, ldo);
  else hipLaunchKernelGGL((levit_conv_kernel<E, false, TO>), grid, blk, 0, s, in, wt, bias, out, B, H, Cin, Cout, OH, act, ldo);
  return check_launch("levit_conv3x3s2");
}

}  // namespace

int levit_attention(int prec, const LevitQKV& a, const float* bias, int B, int R, int stride, int heads, int kd, int vd, int act, void* out,
                    hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (R < 1 || R > LEVIT_MAX_R || heads < 1 || (stride != 1 && stride != 2))
    return fail(EFFOCR_EUNSUPPORTED, "levit_attention: 1 <= R <= 14, heads >= 1 and stride 1 or 2 required");
  if (!((kd == 16 && (vd == 32 || vd == 64)) || (kd == 32 && (vd == 64 || vd == 128))))
    return fail(EFFOCR_EUNSUPPORTED, "levit_attention: (kd, vd) must be (16, 32), (16, 64), (32, 64) or (32, 128)");
  if ((int64_t)B * heads * 2 >= (int64_t)1 << 31) return fail(EFFOCR_EUNSUPPORTED, "levit_attention: too many (crop, head) pairs for one launch");
  if (a.ldq % 8 || a.ldkv % 8 || a.qhs % 8 || a.qoff % 8 || a.khs % 8 || a.koff % 8 || a.voff % 8)
    return fail(EFFOCR_EINVAL, "levit_attention: row strides and head offsets must be multiples of 8 elements");
  const int Rq = stride == 2 ? levit_sub(R) : R;
  const float scale = 1.0f / sqrtf((float)kd);             // 0.25 / 0.17677669
  switch (prec) {
    case PREC_BF16: return launch_attn16<__bf16>(a, bias, static_cast<__bf16*>(out), B, R, Rq, stride, heads, kd, vd, act, scale, s);
    case PREC_FP16: return launch_attn16<_Float16>(a, bias, static_cast<_Float16*>(out), B, R, Rq, stride, heads, kd, vd, act, scale, s);
    case PREC_FP32:
      if (kd == 16)
        hipLaunchKernelGGL((levit_attn_f32_kernel<16>), dim3((unsigned)(B * heads)), dim3(256), 0, s, a, bias, static_cast<float*>(out), R, Rq, stride,
                           heads, vd, act, scale);
      else
        hipLaunchKernelGGL((levit_attn_f32_kernel<32>), dim3((unsigned)(B * heads)), dim3(256), 0, s, a, bias, static_cast<float*>(out), R, Rq, stride,
                           heads, vd, act, scale);
      return check_launch("levit_attention_f32");
  }
  return fail(EFFOCR_EINVAL, "levit_attention: unknown precision");
}

int levit_conv3x3s2(int prec, const void* in, int nchw, int B, int H, int Cin, const float* wt, const float* bias, int Cout, int act, void* out,
                    int ldo, int out_f32, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (H < 1 || Cin < 1 || Cout < 4 || Cout % 4 || ldo < Cout || ldo % 4 || (!nchw && Cin % 8))
    return fail(EFFOCR_EUNSUPPORTED, "levit_conv3x3s2: Cout and the row stride must be multiples of 4, token-major inputs need Cin % 8 == 0");
  const int OH = (H - 1) / 2 + 1;
  if ((int64_t)B * OH * OH * (ldo / 4) >= (int64_t)1 << 39) return fail(EFFOCR_EUNSUPPORTED, "levit_conv3x3s2: too many outputs for one launch");
  const bool f32out = out_f32 != 0;
  switch (prec) {
    case PREC_BF16:
      return f32out ? launch_conv<__bf16, float>(in, nchw, B, H, Cin, wt, bias, Cout, OH, act, static_cast<float*>(out), ldo, s)
                    : launch_conv<__bf16, __bf16>(in, nchw, B, H, Cin, wt, bias, Cout, OH, act, static_cast<__bf16*>(out), ldo, s);
    case PREC_FP16:
      return f32out ? launch_conv<_Float16, float>(in, nchw, B, H, Cin, wt, bias, Cout, OH, act, static_cast<float*>(out), ldo, s)
                    : launch_conv<_Float16, _Float16>(in, nchw, B, H, Cin, wt, bias, Cout, OH, act, static_cast<_Float16*>(out), ldo, s);
    case PREC_FP32: return launch_conv<float, float>(in, nchw, B, H, Cin, wt, bias, Cout, OH, act, static_cast<float*>(out), ldo, s);
  }
  return fail(EFFOCR_EINVAL, "levit_conv3x3s2: unknown precision");
}

int levit_cast_rows(int prec, const float* x, int B, int R, int stride, int D, void* out, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (R < 1 || D < 4 || D % 4 || (stride != 1 && stride != 2)) return fail(EFFOCR_EINVAL, "levit_cast_rows: bad geometry");
  const int Rq = stride == 2 ? levit_sub(R) : R;
  const int64_t n = (int64_t)B * Rq * Rq * (D / 4);
  const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
  switch (prec) {
    case PREC_BF16: hipLaunchKernelGGL(levit_cast_rows_kernel<__bf16>, grid, blk, 0, s, x, static_cast<__bf16*>(out), B, R, Rq, stride, D); break;
    case PREC_FP16: hipLaunchKernelGGL(levit_cast_rows_kernel<_Float16>, grid, blk, 0, s, x, static_cast<_Float16*>(out), B, R, Rq, stride, D); break;
    case PREC_FP32: hipLaunchKernelGGL(levit_cast_rows_kernel<float>, grid, blk, 0, s, x, static_cast<float*>(out), B, R, Rq, stride, D); break;
    default: return fail(EFFOCR_EINVAL, "levit_cast_rows: unknown precision");
  }
  return check_launch("levit_cast_rows");
}

int levit_hardswish(int prec, void* buf, int64_t n, hipStream_t s) {
  if (n <= 0) return EFFOCR_OK;
  if (n % 4) return fail(EFFOCR_EINVAL, "levit_hardswish: the element count must be a multiple of 4");
  const dim3 grid((unsigned)((n / 4 + 255) / 256)), blk(256);
  switch (prec) {
    case PREC_BF16: hipLaunchKernelGGL(levit_hardswish_kernel<__bf16>, grid, blk, 0, s, static_cast<__bf16*>(buf), n / 4); break;
    case PREC_FP16: hipLaunchKernelGGL(levit_hardswish_kernel<_Float16>, grid, blk, 0, s, static_cast<_Float16*>(buf), n / 4); break;
    case PREC_FP32: hipLaunchKernelGGL(levit_hardswish_kernel<float>, grid, blk, 0, s, static_cast<float*>(buf), n / 4); break;
    default: return fail(EFFOCR_EINVAL, "levit_hardswish: unknown precision");
  }
  return check_launch("levit_hardswish");
}

int levit_pool(const float* x, int B, int T, int D, int ldx, int l2norm, float* emb, int* status, hipStream_t s) {
  if (B <= 0) return EFFOCR_OK;
  if (T < 1 || D < 1 || D > 1024 || ldx < D) return fail(EFFOCR_EUNSUPPORTED, "levit_pool: 1 <= D <= 1024, D <= row stride and T >= 1 required");
  hipLaunchKernelGGL(levit_pool_kernel, dim3((unsigned)B), dim3(256), 0, s, x, T, D, ldx, l2norm, emb, status);
  return check_launch("levit_pool");
}

}  // namespace effocr
