// C ABI of libeffocr_beit.so (include/effocr_beit.h): the BEiT encoder handle (parameter table, host-side packing, forward
// orchestration over beit.hip's kernels, the helper kernels of vit_ops.hip and the GEMMs of gemm.hip / gemm2.hip, which this library
// compiles a second time with hidden visibility) and the library's own error state.  All device memory is caller-owned; this file
// allocates host memory only.
#include "../../include/effocr_beit.h"
#include "token_core.hpp"
#include "beit.hpp"

#include <memory>

#define BEIT_API extern "C" __attribute__((visibility("default")))

namespace effocr {
namespace {

constexpr float BEIT_EPS = 1e-6f;                        // timm's BEiT builds every LayerNorm with eps 1e-6
constexpr int BEIT_PATCH = 16, BEIT_PATCH_K = 3 * BEIT_PATCH * BEIT_PATCH;
// sub-batches: as many crops as keep the workspace under BEIT_WS_BUDGET (1 GB < 1 GiB), at most BEIT_MAX_CHUNK
constexpr size_t BEIT_WS_BUDGET = (size_t)1000 << 20;
constexpr int BEIT_MAX_CHUNK = 256;

struct BlockOff : TokenBlockOff { size_t table; };

}  // namespace
}  // namespace effocr

using namespace effocr;

struct effocr_beit : EncoderCore {
  int depth = 0, heads = 0, W = 0, T = 0;                // W patches per side, T = W^2 + 1 tokens per crop
  std::vector<BlockOff> blk;
  size_t cls = 0, patchw = 0, patchb = 0, pos0 = 0, fcnw = 0, fcnb = 0;
};

namespace effocr {
namespace {

// width D, `depth` blocks of D / 64 heads, mlp ratio 4, patch 16.  Key names and order: timm beit.py (a module's own parameters before
// its children's: gamma_1 / gamma_2 open a block, q_bias / v_bias / the table open its attention).
void build_beit(effocr_beit* e) {
  const int D = e->D, T = e->T, heads = e->heads;
  const size_t es = prec_esize(e->prec);
  const int64_t entries = beit_table_entries(e->W);
  Alloc a;
  e->add_param("cls_token", D);
  e->add_param("patch_embed.proj.weight", (int64_t)D * BEIT_PATCH_K);
  e->add_param("patch_embed.proj.bias", D);
  e->cls = a.take((size_t)D * 4);
  e->patchw = a.take((size_t)D * BEIT_PATCH_K * es); e->patchb = a.take((size_t)D * 4);
  e->pos0 = a.take((size_t)T * D * 4);                   // BEiT has no absolute position embedding: EPI_PATCH adds rows of zeros
  e->blk.resize(e->depth);
  for (int i = 0; i < e->depth; ++i) {
    const std::string q = "blocks." + std::to_string(i) + ".";
    e->add_param(q + "gamma_1", D); e->add_param(q + "gamma_2", D);
    e->add_param(q + "norm1.weight", D); e->add_param(q + "norm1.bias", D);
    e->add_param(q + "attn.q_bias", D); e->add_param(q + "attn.v_bias", D);
    e->add_param(q + "attn.relative_position_bias_table", entries * heads);
    e->add_param(q + "attn.qkv.weight", (int64_t)3 * D * D);
    e->add_param(q + "attn.proj.weight", (int64_t)D * D); e->add_param(q + "attn.proj.bias", D);
    e->add_param(q + "norm2.weight", D); e->add_param(q + "norm2.bias", D);
    e->add_param(q + "mlp.fc1.weight", (int64_t)4 * D * D); e->add_param(q + "mlp.fc1.bias", 4 * D);
    e->add_param(q + "mlp.fc2.weight", (int64_t)4 * D * D); e->add_param(q + "mlp.fc2.bias", D);
    BlockOff& L = e->blk[i];
    take_norm1_qkv(a, L, D, es); L.table = a.take((size_t)entries * heads * 4);
    take_proj(a, L, D, es); L.g1 = a.take((size_t)D * 4);
    take_mlp(a, L, D, es); L.g2 = a.take((size_t)D * 4);
  }
  e->add_param("fc_norm.weight", D); e->add_param("fc_norm.bias", D);
  e->fcnw = a.take((size_t)D * 4); e->fcnb = a.take((size_t)D * 4);
  e->wbytes = a.off;
}

// Packing: fp32 vectors and bias tables as they are; linear weights [N][K] rounded once to the operand type; the qkv bias vector is
// [q_bias | 0 | v_bias] (the key projection has no bias); the position rows of the patch-embedding epilogue stay zero.
void pack_beit(const effocr_beit* e, std::vector<char>& blob) {
  const Packer p{e, blob};
  p.f32(e->cls, "cls_token");
  p.op(e->patchw, "patch_embed.proj.weight"); p.f32(e->patchb, "patch_embed.proj.bias");
  for (int i = 0; i < e->depth; ++i) {
    const std::string q = "blocks." + std::to_string(i) + ".";
    const BlockOff& L = e->blk[i];
    pack_token_block(p, L, q);
    p.f32(L.g1, q + "gamma_1"); p.f32(L.g2, q + "gamma_2");
    p.f32(L.table, q + "attn.relative_position_bias_table");
    p.f32(L.qkvb, q + "attn.q_bias"); p.f32(L.qkvb + (size_t)2 * e->D * 4, q + "attn.v_bias");
  }
  p.f32(e->fcnw, "fc_norm.weight"); p.f32(e->fcnb, "fc_norm.bias");
}

// workspace of one sub-batch of B crops: token_core.hpp's layout with patch rows [B P][768]
TokenWs beit_ws(const effocr_beit* e, int B) { return token_ws(B, e->T, e->D, BEIT_PATCH_K, prec_esize(e->prec)); }

int beit_chunk(const effocr_beit* e, int batch) {
  return enc_default_chunk(e, batch, BEIT_WS_BUDGET, BEIT_MAX_CHUNK, [e](int B) { return beit_ws(e, B).total; });
}

// One sub-batch: im2col -> patch GEMM into rows 1.. of every crop, cls row -> blocks (LN1 -> qkv -> bias attention -> proj, layer scale
// + residual; LN2 -> fc1 + GELU -> fc2, layer scale + residual) -> head.  Every GEMM's kernel is chosen by (precision, N, K) alone and
// reduces K in a fixed order (no split-K); the attention kernel by the token count: a crop's embedding does not depend on B.
int beit_forward(const effocr_beit* e, const float* x, int B, float* emb, int l2, char* ws, hipStream_t s) {
  const TokenWs w = beit_ws(e, B);
  const char* wb = e->wdev;
  const int prec = e->prec, D = e->D, T = e->T, P = T - 1;
  auto F = [&](size_t off) { return reinterpret_cast<const float*>(wb + off); };
  float* xs = reinterpret_cast<float*>(ws + w.x);
  void* A = ws + w.a; void* Q = ws + w.q;
  int* status = reinterpret_cast<int*>(ws + w.status);
  int rc;
  LinearExtras patch{};
  patch.pos = F(e->pos0); patch.P = P;
  if ((rc = im2col_patch16(prec, x, 0, B, e->img, e->img, A, s))) return rc;
  if ((rc = dense_linear(prec, EPI_PATCH, A, BEIT_PATCH_K, wb + e->patchw, F(e->patchb), xs, D, (int64_t)B * P, patch, s))) return rc;
  if ((rc = set_cls_rows(F(e->cls), xs, B, T, D, 0, nullptr, s))) return rc;
  const TokenRun run{prec, wb, (int64_t)B * T, D, BEIT_EPS, xs, A, Q, s};
  if ((rc = token_blocks(run, e->blk, EPI_BIAS_SCALE_RESID, [&](const BlockOff& L, const void* qkv, void* out) {
         return beit_attention(prec, qkv, F(L.table), B, e->W, e->heads, out, s);
       }))) return rc;
  return beit_head(xs, B, T, D, F(e->fcnw), F(e->fcnb), BEIT_EPS, l2, emb, status, s);
}

}  // namespace
}  // namespace effocr

BEIT_API int effocr_beit_abi_version(void) { return EFFOCR_BEIT_ABI_VERSION; }
BEIT_API const char* effocr_beit_last_error(void) { return g_err.c_str(); }

BEIT_API int effocr_beit_create(const char* arch, int img_size, int precision, effocr_beit_t** out) {
  if (!arch || !out) return fail(EFFOCR_BEIT_EINVAL, "beit_create: NULL argument");
  if (precision < 0 || precision > 2) return fail(EFFOCR_BEIT_EINVAL, "beit_create: unknown precision");
  const std::string name(arch);
  int D, depth;
  if (name == "beit_base_patch16_224" || name == "beitv2_base_patch16_224") { D = 768; depth = 12; }
  else if (name == "beit_tiny_test") { D = 128; depth = 2; }
  else return fail(EFFOCR_BEIT_EUNSUPPORTED, "beit_create: unsupported architecture '" + name + "'");
  if (img_size < BEIT_PATCH || img_size > BEIT_PATCH * BEIT_MAX_W || img_size % BEIT_PATCH)
    return fail(EFFOCR_BEIT_EINVAL, "beit_create: img_size must be a multiple of 16 from 16 to 224");
  std::unique_ptr<effocr_beit> e(new effocr_beit());
  e->img = img_size; e->prec = precision; e->D = D; e->depth = depth; e->heads = D / 64;
  e->W = img_size / BEIT_PATCH; e->T = e->W * e->W + 1;
  build_beit(e.get());
  *out = e.release();
  return EFFOCR_BEIT_OK;
}

BEIT_API void effocr_beit_destroy(effocr_beit_t* enc) { delete enc; }
BEIT_API int effocr_beit_embed_dim(const effocr_beit_t* enc) { return enc ? enc->D : 0; }
BEIT_API int effocr_beit_num_params(const effocr_beit_t* enc) { return enc ? (int)enc->params.size() : 0; }
BEIT_API const char* effocr_beit_param_name(const effocr_beit_t* enc, int i) { return enc_param_name(enc, i); }
BEIT_API int64_t effocr_beit_param_numel(const effocr_beit_t* enc, int i) { return enc_param_numel(enc, i); }

BEIT_API int effocr_beit_set_param(effocr_beit_t* enc, const char* name, const float* host, int64_t numel) {
  return enc_set_param("beit", enc, name, host, numel);
}

BEIT_API size_t effocr_beit_weights_bytes(const effocr_beit_t* enc) { return enc ? enc->wbytes : 0; }

BEIT_API int effocr_beit_upload(effocr_beit_t* enc, void* weights_dev, size_t bytes) {
  return enc_upload("beit", enc, weights_dev, bytes, pack_beit);
}

BEIT_API size_t effocr_beit_workspace_bytes(const effocr_beit_t* enc, int batch) {
  if (!enc || batch <= 0) return 0;
  return beit_ws(enc, beit_chunk(enc, batch)).total;
}

BEIT_API int effocr_beit_set_chunk(effocr_beit_t* enc, int crops_per_chunk) { return enc_set_chunk("beit", enc, crops_per_chunk); }

BEIT_API int effocr_beit_forward(effocr_beit_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize, void* workspace_dev,
                                 size_t workspace_bytes, void* stream) {
  const int rc = enc_forward_args("beit", enc, x_dev, batch, emb_dev, workspace_dev, workspace_bytes, effocr_beit_workspace_bytes(enc, batch));
  if (rc || batch == 0) return rc;
  const int chunk = beit_chunk(enc, batch);
  if (!token_index_ok(chunk, enc->T, enc->D))
    return fail(EFFOCR_BEIT_EUNSUPPORTED, "beit_forward: chunk too large for 32-bit GEMM indices (effocr_beit_set_chunk)");
  return enc_forward_chunks(enc, x_dev, batch, chunk, emb_dev, [&](const float* x, int crops, float* emb) {
    return beit_forward(enc, x, crops, emb, l2_normalize, static_cast<char*>(workspace_dev), S(stream));
  });
}

BEIT_API int effocr_beit_check_status(const effocr_beit_t* enc, const void* workspace_dev, void* stream) {   // BeitWs::status = offset 0
  return enc_check_status("beit", enc, workspace_dev, stream, ENC_F16_OPERAND_OVERFLOW);
}

BEIT_API int effocr_beit_reset_status(const effocr_beit_t* enc, void* workspace_dev, void* stream) {
  return enc_reset_status("beit", enc, workspace_dev, stream);
}

BEIT_API int effocr_beit_op_attn(const void* qkv_dev, const float* table_dev, int batch, int patches_per_side, int heads, int dtype,
                                 void* out_dev, void* stream) {
  if (!qkv_dev || !table_dev || !out_dev) return fail(EFFOCR_BEIT_EINVAL, "beit_op_attn: NULL argument");
  if (batch <= 0 || heads <= 0) return fail(EFFOCR_BEIT_EINVAL, "beit_op_attn: bad geometry");
  return beit_attention(dtype, qkv_dev, table_dev, batch, patches_per_side, heads, out_dev, S(stream));
}
