// C ABI of libeffocr_vit8.so (include/effocr_vit8.h): the patch-8 ViT encoder handle (parameter table, host-side packing, forward
// orchestration over vit8.hip's kernels, the helper kernels of vit_ops.hip and the GEMMs of gemm.hip / gemm2.hip, which this library
// compiles once more with hidden visibility) and the library's own error state.  All device memory is caller-owned; this file
// allocates host memory only.
#include "../../include/effocr_vit8.h"
#include "token_core.hpp"
#include "vit8.hpp"

#include <memory>

#define VIT8_API extern "C" __attribute__((visibility("default")))

namespace effocr {
namespace {

constexpr float VIT8_EPS = 1e-6f;                        // timm's vision_transformer.py builds every LayerNorm with eps 1e-6
// sub-batches: as many crops as keep the workspace under VIT8_WS_BUDGET (1 GB < 1 GiB), at most VIT8_MAX_CHUNK
constexpr size_t VIT8_WS_BUDGET = (size_t)1000 << 20;
constexpr int VIT8_MAX_CHUNK = 256;

using BlockOff = TokenBlockOff;

}  // namespace
}  // namespace effocr

using namespace effocr;

struct effocr_vit8 : EncoderCore {
  int depth = 0, heads = 0, W = 0, T = 0;                // W patches per side, T = W^2 + 1 tokens per crop
  std::vector<BlockOff> blk;
  size_t cls0 = 0, patchw = 0, patchb = 0, pos = 0, normw = 0, normb = 0;
};

namespace effocr {
namespace {

// width D, `depth` pre-norm blocks of D / 64 heads, mlp ratio 4, patch 8.  Key names and order: timm vision_transformer.py (the ones
// weights.py reads for the patch-16 ViTs).
void build_vit8(effocr_vit8* e) {
  const int D = e->D, T = e->T;
  const size_t es = prec_esize(e->prec);
  Alloc a;
  e->add_param("cls_token", D);
  e->add_param("pos_embed", (int64_t)T * D);
  e->add_param("patch_embed.proj.weight", (int64_t)D * VIT8_PATCH_K);
  e->add_param("patch_embed.proj.bias", D);
  e->cls0 = a.take((size_t)D * 4);
  e->pos = a.take((size_t)T * D * 4);
  e->patchw = a.take((size_t)D * VIT8_PATCH_K * es); e->patchb = a.take((size_t)D * 4);
  e->blk.resize(e->depth);
  for (int i = 0; i < e->depth; ++i) {
    const std::string q = "blocks." + std::to_string(i) + ".";
    e->add_param(q + "norm1.weight", D); e->add_param(q + "norm1.bias", D);
    e->add_param(q + "attn.qkv.weight", (int64_t)3 * D * D); e->add_param(q + "attn.qkv.bias", 3 * D);
    e->add_param(q + "attn.proj.weight", (int64_t)D * D); e->add_param(q + "attn.proj.bias", D);
    e->add_param(q + "norm2.weight", D); e->add_param(q + "norm2.bias", D);
    e->add_param(q + "mlp.fc1.weight", (int64_t)4 * D * D); e->add_param(q + "mlp.fc1.bias", 4 * D);
    e->add_param(q + "mlp.fc2.weight", (int64_t)4 * D * D); e->add_param(q + "mlp.fc2.bias", D);
    BlockOff& L = e->blk[i];
    take_norm1_qkv(a, L, D, es); take_proj(a, L, D, es); take_mlp(a, L, D, es);
  }
  e->add_param("norm.weight", D); e->add_param("norm.bias", D);
  e->normw = a.take((size_t)D * 4); e->normb = a.take((size_t)D * 4);
  e->wbytes = a.off;
}

// Packing: fp32 vectors and pos_embed as they are; linear weights [N][K] rounded once to the operand type; the cls row is
// cls_token + pos_embed[0], added once here in fp32.
void pack_vit8(const effocr_vit8* e, std::vector<char>& blob) {
  const Packer p{e, blob};
  const int D = e->D;
  std::vector<float> c0(e->P("cls_token"));
  const std::vector<float>& pos = e->P("pos_embed");
  for (int d = 0; d < D; ++d) c0[d] += pos[d];
  put_f32(blob, e->cls0, c0.data(), c0.size());
  p.f32(e->pos, "pos_embed");
  p.op(e->patchw, "patch_embed.proj.weight"); p.f32(e->patchb, "patch_embed.proj.bias");
  for (int i = 0; i < e->depth; ++i) {
    const std::string q = "blocks." + std::to_string(i) + ".";
    pack_token_block(p, e->blk[i], q);
    p.f32(e->blk[i].qkvb, q + "attn.qkv.bias");
  }
  p.f32(e->normw, "norm.weight"); p.f32(e->normb, "norm.bias");
}

// workspace of one sub-batch of B crops: token_core.hpp's layout with patch rows [B P][192]
TokenWs vit8_ws(const effocr_vit8* e, int B) { return token_ws(B, e->T, e->D, VIT8_PATCH_K, prec_esize(e->prec)); }

int vit8_chunk(const effocr_vit8* e, int batch) {
  return enc_default_chunk(e, batch, VIT8_WS_BUDGET, VIT8_MAX_CHUNK, [e](int B) { return vit8_ws(e, B).total; });
}

// One sub-batch: im2col -> patch GEMM (+ bias + pos_embed) into rows 1.. of every crop, cls row -> blocks (LN1 -> qkv -> streaming
// attention -> proj + residual; LN2 -> fc1 + GELU -> fc2 + residual) -> final norm of the cls rows.  Every GEMM's kernel is chosen by
// (precision, N, K) alone and reduces K in a fixed order (no split-K); the attention kernel walks each crop's own keys: a crop's
// embedding does not depend on B.
int vit8_forward(const effocr_vit8* e, const float* x, int B, float* emb, int l2, char* ws, hipStream_t s) {
  const TokenWs w = vit8_ws(e, B);
  const char* wb = e->wdev;
  const int prec = e->prec, D = e->D, T = e->T;
  auto F = [&](size_t off) { return reinterpret_cast<const float*>(wb + off); };
  float* xs = reinterpret_cast<float*>(ws + w.x);
  void* A = ws + w.a; void* Q = ws + w.q;
  int* status = reinterpret_cast<int*>(ws + w.status);
  int rc;
  if ((rc = vit8_patch_embed(prec, x, B, e->img, D, wb + e->patchw, F(e->patchb), F(e->cls0), F(e->pos), A, xs, s))) return rc;
  const TokenRun run{prec, wb, (int64_t)B * T, D, VIT8_EPS, xs, A, Q, s};
  if ((rc = token_blocks(run, e->blk, EPI_BIAS_RESID, [&](const BlockOff&, const void* qkv, void* out) {
         return vit8_attention(prec, qkv, B, T, e->heads, out, s);
       }))) return rc;
  return final_cls_norm(xs, B, T, D, F(e->normw), F(e->normb), VIT8_EPS, l2, 0, emb, status, s);
}

}  // namespace
}  // namespace effocr

VIT8_API int effocr_vit8_abi_version(void) { return EFFOCR_VIT8_ABI_VERSION; }
VIT8_API const char* effocr_vit8_last_error(void) { return g_err.c_str(); }

VIT8_API int effocr_vit8_create(const char* arch, int img_size, int precision, effocr_vit8_t** out) {
  if (!arch || !out) return fail(EFFOCR_VIT8_EINVAL, "vit8_create: NULL argument");
  if (precision < 0 || precision > 2) return fail(EFFOCR_VIT8_EINVAL, "vit8_create: unknown precision");
  const std::string name(arch);
  int D, depth;
  if (name == "vit_small_patch8_224") { D = 384; depth = 12; }
  else if (name == "vit_base_patch8_224") { D = 768; depth = 12; }
  else if (name == "vit8_tiny_test") { D = 128; depth = 2; }
  else return fail(EFFOCR_VIT8_EUNSUPPORTED, "vit8_create: unsupported architecture '" + name + "'");
  if (img_size < VIT8_PATCH || img_size > VIT8_PATCH * VIT8_MAX_W || img_size % VIT8_PATCH)
    return fail(EFFOCR_VIT8_EINVAL, "vit8_create: img_size must be a multiple of 8 from 8 to 224");
  std::unique_ptr<effocr_vit8> e(new effocr_vit8());
  e->img = img_size; e->prec = precision; e->D = D; e->depth = depth; e->heads = D / 64;
  e->W = img_size / VIT8_PATCH; e->T = e->W * e->W + 1;
  build_vit8(e.get());
  *out = e.release();
  return EFFOCR_VIT8_OK;
}

VIT8_API void effocr_vit8_destroy(effocr_vit8_t* enc) { delete enc; }
VIT8_API int effocr_vit8_embed_dim(const effocr_vit8_t* enc) { return enc ? enc->D : 0; }
VIT8_API int effocr_vit8_num_params(const effocr_vit8_t* enc) { return enc ? (int)enc->params.size() : 0; }
VIT8_API const char* effocr_vit8_param_name(const effocr_vit8_t* enc, int i) { return enc_param_name(enc, i); }
VIT8_API int64_t effocr_vit8_param_numel(const effocr_vit8_t* enc, int i) { return enc_param_numel(enc, i); }

VIT8_API int effocr_vit8_set_param(effocr_vit8_t* enc, const char* name, const float* host, int64_t numel) {
  return enc_set_param("vit8", enc, name, host, numel);
}

VIT8_API size_t effocr_vit8_weights_bytes(const effocr_vit8_t* enc) { return enc ? enc->wbytes : 0; }

VIT8_API int effocr_vit8_upload(effocr_vit8_t* enc, void* weights_dev, size_t bytes) {
  return enc_upload("vit8", enc, weights_dev, bytes, pack_vit8);
}

VIT8_API size_t effocr_vit8_workspace_bytes(const effocr_vit8_t* enc, int batch) {
  if (!enc || batch <= 0) return 0;
  return vit8_ws(enc, vit8_chunk(enc, batch)).total;
}

VIT8_API int effocr_vit8_set_chunk(effocr_vit8_t* enc, int crops_per_chunk) { return enc_set_chunk("vit8", enc, crops_per_chunk); }

VIT8_API int effocr_vit8_forward(effocr_vit8_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize, void* workspace_dev,
                                 size_t workspace_bytes, void* stream) {
  const int rc = enc_forward_args("vit8", enc, x_dev, batch, emb_dev, workspace_dev, workspace_bytes, effocr_vit8_workspace_bytes(enc, batch));
  if (rc || batch == 0) return rc;
  const int chunk = vit8_chunk(enc, batch);
  if (!token_index_ok(chunk, enc->T, enc->D))
    return fail(EFFOCR_VIT8_EUNSUPPORTED, "vit8_forward: chunk too large for 32-bit GEMM indices (effocr_vit8_set_chunk)");
  return enc_forward_chunks(enc, x_dev, batch, chunk, emb_dev, [&](const float* x, int crops, float* emb) {
    return vit8_forward(enc, x, crops, emb, l2_normalize, static_cast<char*>(workspace_dev), S(stream));
  });
}

VIT8_API int effocr_vit8_check_status(const effocr_vit8_t* enc, const void* workspace_dev, void* stream) {   // Vit8Ws::status = offset 0
  return enc_check_status("vit8", enc, workspace_dev, stream, ENC_F16_OPERAND_OVERFLOW);
}

VIT8_API int effocr_vit8_reset_status(const effocr_vit8_t* enc, void* workspace_dev, void* stream) {
  return enc_reset_status("vit8", enc, workspace_dev, stream);
}

VIT8_API int effocr_vit8_op_attn(const void* qkv_dev, int batch, int tokens, int heads, int dtype, void* out_dev, void* stream) {
  if (!qkv_dev || !out_dev) return fail(EFFOCR_VIT8_EINVAL, "vit8_op_attn: NULL argument");
  if (batch <= 0 || heads <= 0) return fail(EFFOCR_VIT8_EINVAL, "vit8_op_attn: bad geometry");
  return vit8_attention(dtype, qkv_dev, batch, tokens, heads, out_dev, S(stream));
}

VIT8_API int effocr_vit8_op_patch_embed(const float* x_dev, int batch, int img_size, int embed_dim, int dtype, const void* w_dev,
                                        const float* bias_dev, const float* cls_pos0_dev, const float* pos_dev, void* col_dev,
                                        float* out_dev, void* stream) {
  if (!x_dev || !w_dev || !bias_dev || !cls_pos0_dev || !pos_dev || !col_dev || !out_dev) return fail(EFFOCR_VIT8_EINVAL, "vit8_op_patch_embed: NULL argument");
  if (batch <= 0 || embed_dim <= 0 || embed_dim % 128) return fail(EFFOCR_VIT8_EINVAL, "vit8_op_patch_embed: batch >= 1 and embed_dim a positive multiple of 128 required");
  if (dtype < 0 || dtype > 2) return fail(EFFOCR_VIT8_EINVAL, "vit8_op_patch_embed: unknown precision");
  return vit8_patch_embed(dtype, x_dev, batch, img_size, embed_dim, w_dev, bias_dev, cls_pos0_dev, pos_dev, col_dev, out_dev, S(stream));
}
