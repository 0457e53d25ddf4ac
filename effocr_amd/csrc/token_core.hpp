// Host-side core of the token encoders, on top of enc_core.hpp: the one dense linear of Swin, BEiT and the patch-8 ViT, and what the
// two plain pre-norm ViT bodies (BEiT, patch-8 ViT) share — workspace, block offsets, block packing, the block loop and the index guard.
// No kernel: include it from the family's *_api.hip after enc_core.hpp's rules (one translation unit per library).
#pragma once
#include "enc_core.hpp"

namespace effocr {

// What an epilogue reads beyond the bias; zero-initialise it and set only what the epilogue of the call reads.
struct LinearExtras {
  const float* resid;   // EPI_BIAS_RESID, EPI_BIAS_SCALE_RESID: fp32 residual rows [rows][N] (may be `out` itself)
  const float* scale;   // EPI_BIAS_SCALE_RESID: [N] fp32 layer scale
  const float* pos;     // EPI_PATCH: position rows [1 + P][N] fp32
  int P;                // EPI_PATCH: patches per crop
};

// out [rows][N] = epilogue(X [rows][K] . W [N][K]^T + bias): dense rows (ldx = ldw = K, ldo = ldr = N), the kernel chosen by
// (precision, N, K) alone.
static inline int dense_linear(int prec, int epi, const void* X, int K, const void* W, const float* bias, void* out, int N, int64_t rows,
                               const LinearExtras& x, hipStream_t s) {
  GemmArgs g{};
  g.X = X; g.ldx = K; g.W = W; g.ldw = K; g.bias = bias; g.out = out; g.ldo = N; g.M = (int)rows; g.N = N; g.K = K;
  g.resid = x.resid; g.ldr = N; g.scale = x.scale; g.pos = x.pos; g.P = x.P;
  return gemm2_supported(prec, N, K) ? gemm2_nt(prec, epi, g, s) : gemm_nt(prec, epi, g, s);
}

// ---------------------------------------------------------------- BEiT and the patch-8 ViT
// workspace of one sub-batch of B crops of T tokens: status word, fp32 residual [B T][D], the operand buffer A (patch rows
// [B (T-1)][patch_k], LayerNorm and attention outputs [B T][D]) and the buffer Q of the qkv output [B T][3D] / the hidden [B T][4D]
// (never live at once).
struct TokenWs { size_t status, x, a, q, total; };
static inline TokenWs token_ws(int B, int T, int D, int patch_k, size_t es) {
  const size_t M = (size_t)B * T;
  Alloc a; TokenWs w;
  w.status = a.take(256);                   // int32 status word at workspace offset 0 (enc_check_status)
  w.x = a.take(M * D * 4);
  w.a = a.take(std::max(M * D, (size_t)B * (T - 1) * patch_k) * es);
  w.q = a.take(M * 4 * D * es);
  w.total = a.off;
  return w;
}

// the GEMMs index with 32 bits: the widest matrix of a sub-batch is the hidden [chunk T][4D]
static inline bool token_index_ok(int chunk, int T, int D) { return (int64_t)chunk * T * 4 * D < (int64_t)1 << 31; }

// blob offsets of one pre-norm block (mlp ratio 4); g1 / g2: the layer scales of EPI_BIAS_SCALE_RESID, unused otherwise.  The three
// take_* calls run in blob order, so a family can take a buffer of its own between them.
struct TokenBlockOff { size_t ln1w, ln1b, qkvw, qkvb, projw, projb, g1, ln2w, ln2b, fc1w, fc1b, fc2w, fc2b, g2; };
static inline void take_norm1_qkv(Alloc& a, TokenBlockOff& L, size_t D, size_t es) {
  L.ln1w = a.take(D * 4); L.ln1b = a.take(D * 4);
  L.qkvw = a.take(3 * D * D * es); L.qkvb = a.take(3 * D * 4);
}
static inline void take_proj(Alloc& a, TokenBlockOff& L, size_t D, size_t es) { L.projw = a.take(D * D * es); L.projb = a.take(D * 4); }
static inline void take_mlp(Alloc& a, TokenBlockOff& L, size_t D, size_t es) {
  L.ln2w = a.take(D * 4); L.ln2b = a.take(D * 4);
  L.fc1w = a.take(4 * D * D * es); L.fc1b = a.take(4 * D * 4);
  L.fc2w = a.take(4 * D * D * es); L.fc2b = a.take(D * 4);
}

// named parameters into the blob: fp32 as they are / linear weights [N][K] rounded once to the operand type
struct Packer {
  const EncoderCore* e; std::vector<char>& blob;
  void f32(size_t off, const std::string& n) const { const auto& v = e->P(n); put_f32(blob, off, v.data(), v.size()); }
  void op(size_t off, const std::string& n) const { const auto& v = e->P(n); put_op(blob, off, v.data(), v.size(), e->prec); }
};
// the parameters of block `q` ("blocks.<i>.") that both families name alike; the qkv bias is each family's own
static inline void pack_token_block(const Packer& p, const TokenBlockOff& L, const std::string& q) {
  p.f32(L.ln1w, q + "norm1.weight"); p.f32(L.ln1b, q + "norm1.bias");
  p.f32(L.ln2w, q + "norm2.weight"); p.f32(L.ln2b, q + "norm2.bias");
  p.op(L.qkvw, q + "attn.qkv.weight");
  p.op(L.projw, q + "attn.proj.weight"); p.f32(L.projb, q + "attn.proj.bias");
  p.op(L.fc1w, q + "mlp.fc1.weight"); p.f32(L.fc1b, q + "mlp.fc1.bias");
  p.op(L.fc2w, q + "mlp.fc2.weight"); p.f32(L.fc2b, q + "mlp.fc2.bias");
}

// The blocks of one sub-batch of M token rows: LN1 -> qkv -> attention -> proj + residual; LN2 -> fc1 + GELU -> fc2 + residual, the
// residual stream xs updated in place.  resid_epi: EPI_BIAS_RESID, or EPI_BIAS_SCALE_RESID with the block's g1 / g2.
// attn(L, qkv, out) -> rc launches the family's attention for block L.
struct TokenRun { int prec; const char* wb; int64_t M; int D; float eps; float* xs; void* A; void* Q; hipStream_t s; };
template <typename Block, typename Attn>
int token_blocks(const TokenRun& r, const std::vector<Block>& blocks, int resid_epi, Attn attn) {
  auto F = [&](size_t off) { return reinterpret_cast<const float*>(r.wb + off); };
  auto lin = [&](const void* X, int K, size_t woff, size_t boff, void* out, int N, int epi, const LinearExtras& x) {
    return dense_linear(r.prec, epi, X, K, r.wb + woff, F(boff), out, N, r.M, x, r.s);
  };
  const int D = r.D;
  const bool scaled = resid_epi == EPI_BIAS_SCALE_RESID;
  int rc;
  for (const Block& L : blocks) {
    const LinearExtras none{}, r1{r.xs, scaled ? F(L.g1) : nullptr}, r2{r.xs, scaled ? F(L.g2) : nullptr};
    if ((rc = layernorm_rows(r.prec, r.xs, r.M, D, F(L.ln1w), F(L.ln1b), r.eps, r.A, r.s))) return rc;
    if ((rc = lin(r.A, D, L.qkvw, L.qkvb, r.Q, 3 * D, EPI_BIAS, none))) return rc;
    if ((rc = attn(L, r.Q, r.A))) return rc;
    if ((rc = lin(r.A, D, L.projw, L.projb, r.xs, D, resid_epi, r1))) return rc;
    if ((rc = layernorm_rows(r.prec, r.xs, r.M, D, F(L.ln2w), F(L.ln2b), r.eps, r.A, r.s))) return rc;
    if ((rc = lin(r.A, D, L.fc1w, L.fc1b, r.Q, 4 * D, EPI_BIAS_GELU, none))) return rc;
    if ((rc = lin(r.Q, 4 * D, L.fc2w, L.fc2b, r.xs, D, resid_epi, r2))) return rc;
  }
  return EFFOCR_OK;
}

}  // namespace effocr
