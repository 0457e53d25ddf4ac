// C ABI of libeffocr_swin.so (include/effocr_swin.h): the Swin-T encoder handle (parameter table, host-side packing, forward
// orchestration over swin.hip's kernels and the GEMMs of gemm.hip / gemm2.hip, which this library compiles a second time with hidden
// visibility) and the library's own error state.  All device memory is caller-owned; this file allocates host memory only.
#include "../../include/effocr_swin.h"
#include "token_core.hpp"
#include "swin.hpp"

#include <memory>

#define SWIN_API extern "C" __attribute__((visibility("default")))

namespace effocr {
namespace {

constexpr float SWIN_EPS = 1e-5f;                        // nn.LayerNorm's default: every LayerNorm of timm's Swin
constexpr int SWIN_WS = 7, SWIN_SHIFT = 3;
// sub-batches: as many crops as keep the workspace under SWIN_WS_BUDGET (1 GB < 1 GiB), at most SWIN_MAX_CHUNK
constexpr size_t SWIN_WS_BUDGET = (size_t)1000 << 20;
constexpr int SWIN_MAX_CHUNK = 192;

struct BlockOff { size_t ln1w, ln1b, qkvw, qkvb, table, projw, projb, ln2w, ln2b, fc1w, fc1b, fc2w, fc2b; int shift; };
struct StageOff { int C, Cp, H, depth; size_t mlnw, mlnb, redw, redb; std::vector<BlockOff> blocks; };

}  // namespace
}  // namespace effocr

using namespace effocr;

struct effocr_swin : EncoderCore {
  std::vector<StageOff> st;
  size_t stemw = 0, stemb = 0, stemlnw = 0, stemlnb = 0, normw = 0, normb = 0;
};

namespace effocr {
namespace {

// swin_tiny_patch4_window7_224: depths 2-2-6-2, widths 96-192-384-768, head dim 32, window 7, mlp ratio 4.  Key names: timm >= 0.9.
void build_swin(effocr_swin* e) {
  static const int depths[4] = {2, 2, 6, 2}, widths[4] = {96, 192, 384, 768};
  const size_t es = prec_esize(e->prec);
  Alloc a;
  e->add_param("patch_embed.proj.weight", (int64_t)widths[0] * 48);
  e->add_param("patch_embed.proj.bias", widths[0]);
  e->add_param("patch_embed.norm.weight", widths[0]);
  e->add_param("patch_embed.norm.bias", widths[0]);
  e->stemw = a.take((size_t)48 * 128 * 4);
  e->stemb = a.take(128 * 4); e->stemlnw = a.take(128 * 4); e->stemlnb = a.take(128 * 4);
  e->st.resize(4);
  int H = e->img / 4;
  for (int i = 0; i < 4; ++i) {
    StageOff& s = e->st[i];
    const int C = widths[i], Cp = (int)align_up((size_t)C, 128), heads = C / 32;
    if (i > 0) H /= 2;
    s.C = C; s.Cp = Cp; s.H = H; s.depth = depths[i];
    const std::string p = "layers." + std::to_string(i) + ".";
    if (i > 0) {
      const int Cv = widths[i - 1];
      e->add_param(p + "downsample.norm.weight", 4 * Cv);
      e->add_param(p + "downsample.norm.bias", 4 * Cv);
      e->add_param(p + "downsample.reduction.weight", (int64_t)C * 4 * Cv);
      s.mlnw = a.take((size_t)4 * Cv * 4); s.mlnb = a.take((size_t)4 * Cv * 4);
      s.redw = a.take((size_t)Cp * 4 * Cv * es); s.redb = a.take((size_t)Cp * 4);      // reduction has no bias: a zero vector
    }
    s.blocks.resize(depths[i]);
    for (int j = 0; j < depths[i]; ++j) {
      const std::string q = p + "blocks." + std::to_string(j) + ".";
      e->add_param(q + "norm1.weight", C); e->add_param(q + "norm1.bias", C);
      e->add_param(q + "attn.relative_position_bias_table", (int64_t)(2 * SWIN_WS - 1) * (2 * SWIN_WS - 1) * heads);
      e->add_param(q + "attn.qkv.weight", (int64_t)3 * C * C); e->add_param(q + "attn.qkv.bias", 3 * C);
      e->add_param(q + "attn.proj.weight", (int64_t)C * C); e->add_param(q + "attn.proj.bias", C);
      e->add_param(q + "norm2.weight", C); e->add_param(q + "norm2.bias", C);
      e->add_param(q + "mlp.fc1.weight", (int64_t)4 * C * C); e->add_param(q + "mlp.fc1.bias", 4 * C);
      e->add_param(q + "mlp.fc2.weight", (int64_t)4 * C * C); e->add_param(q + "mlp.fc2.bias", C);
      BlockOff& L = s.blocks[j];
      L.shift = (j % 2 == 1 && H > SWIN_WS) ? SWIN_SHIFT : 0;       // timm: no shift when the map is one window
      L.ln1w = a.take((size_t)Cp * 4); L.ln1b = a.take((size_t)Cp * 4);
      L.table = a.take((size_t)(2 * SWIN_WS - 1) * (2 * SWIN_WS - 1) * heads * 4);
      L.qkvw = a.take((size_t)3 * Cp * Cp * es); L.qkvb = a.take((size_t)3 * Cp * 4);
      L.projw = a.take((size_t)Cp * Cp * es); L.projb = a.take((size_t)Cp * 4);
      L.ln2w = a.take((size_t)Cp * 4); L.ln2b = a.take((size_t)Cp * 4);
      L.fc1w = a.take((size_t)4 * C * Cp * es); L.fc1b = a.take((size_t)4 * C * 4);
      L.fc2w = a.take((size_t)Cp * 4 * C * es); L.fc2b = a.take((size_t)Cp * 4);
    }
  }
  e->add_param("norm.weight", widths[3]); e->add_param("norm.bias", widths[3]);
  e->normw = a.take((size_t)e->st[3].Cp * 4); e->normb = a.take((size_t)e->st[3].Cp * 4);
  e->wbytes = a.off;
}

// [rows][cols] -> [rows_p][cols_p] zero-padded, rows mapped by rmap (row r of the source lands on row rmap(r))
template <typename F>
std::vector<float> pad2(const std::vector<float>& w, int rows, int cols, int rows_p, int cols_p, F rmap) {
  std::vector<float> t((size_t)rows_p * cols_p, 0.f);
  for (int r = 0; r < rows; ++r) memcpy(t.data() + (size_t)rmap(r) * cols_p, w.data() + (size_t)r * cols, (size_t)cols * 4);
  return t;
}

// Packing: fp32 vectors zero-padded to Cp; qkv [3C][C] -> [3][Cp][Cp] (q, k, v each padded on its own, so no head straddles padding);
// proj [C][C] -> [Cp][Cp]; fc1 [4C][C] -> [4C][Cp]; fc2 [C][4C] -> [Cp][4C]; reduction [C][4Cv] -> [Cp][4Cv]; patch_embed conv tap-major
// [48][128]; bias tables as they are ([169][heads] fp32).  Zero pad rows / columns keep the residual's pad channels exactly 0.
void pack_swin(const effocr_swin* e, std::vector<char>& blob) {
  auto padf = [&](size_t off, const std::string& n) { const auto& v = e->P(n); put_f32(blob, off, v.data(), v.size()); };
  const int prec = e->prec;
  {
    const auto& w = e->P("patch_embed.proj.weight");
    const int C0 = e->st[0].C;
    float* d = reinterpret_cast<float*>(blob.data() + e->stemw);
    for (int c = 0; c < C0; ++c)
      for (int k = 0; k < 48; ++k) d[k * 128 + c] = w[(size_t)c * 48 + k];
    padf(e->stemb, "patch_embed.proj.bias"); padf(e->stemlnw, "patch_embed.norm.weight"); padf(e->stemlnb, "patch_embed.norm.bias");
  }
  for (int i = 0; i < 4; ++i) {
    const StageOff& s = e->st[i];
    const int C = s.C, Cp = s.Cp;
    const std::string p = "layers." + std::to_string(i) + ".";
    if (i > 0) {
      const int Cv = e->st[i - 1].C;
      padf(s.mlnw, p + "downsample.norm.weight"); padf(s.mlnb, p + "downsample.norm.bias");
      const auto t = pad2(e->P(p + "downsample.reduction.weight"), C, 4 * Cv, Cp, 4 * Cv, [](int r) { return r; });
      put_op(blob, s.redw, t.data(), t.size(), prec);
    }
    for (int j = 0; j < s.depth; ++j) {
      const std::string q = p + "blocks." + std::to_string(j) + ".";
      const BlockOff& L = s.blocks[j];
      padf(L.ln1w, q + "norm1.weight"); padf(L.ln1b, q + "norm1.bias");
      padf(L.ln2w, q + "norm2.weight"); padf(L.ln2b, q + "norm2.bias");
      padf(L.table, q + "attn.relative_position_bias_table");
      padf(L.projb, q + "attn.proj.bias"); padf(L.fc1b, q + "mlp.fc1.bias"); padf(L.fc2b, q + "mlp.fc2.bias");
      auto qmap = [C, Cp](int r) { return (r / C) * Cp + r % C; };
      auto t = pad2(e->P(q + "attn.qkv.weight"), 3 * C, C, 3 * Cp, Cp, qmap);
      put_op(blob, L.qkvw, t.data(), t.size(), prec);
      {
        const auto& b = e->P(q + "attn.qkv.bias");
        float* d = reinterpret_cast<float*>(blob.data() + L.qkvb);
        for (int r = 0; r < 3 * C; ++r) d[qmap(r)] = b[r];
      }
      t = pad2(e->P(q + "attn.proj.weight"), C, C, Cp, Cp, [](int r) { return r; });
      put_op(blob, L.projw, t.data(), t.size(), prec);
      t = pad2(e->P(q + "mlp.fc1.weight"), 4 * C, C, 4 * C, Cp, [](int r) { return r; });
      put_op(blob, L.fc1w, t.data(), t.size(), prec);
      t = pad2(e->P(q + "mlp.fc2.weight"), C, 4 * C, Cp, 4 * C, [](int r) { return r; });
      put_op(blob, L.fc2w, t.data(), t.size(), prec);
    }
  }
  padf(e->normw, "norm.weight"); padf(e->normb, "norm.bias");
}

// workspace of one sub-batch of B crops: status word, fp32 residual [tokens][Cp], the operand buffer A (LayerNorm output, attention
// output, patch-merging rows) and the buffer Q of the qkv output [tokens][3 Cp] / the hidden [tokens][4C] (never live at once).
struct SwinWs { size_t status, x, a, q, total; };
SwinWs swin_ws(const effocr_swin* e, int B) {
  const size_t es = prec_esize(e->prec);
  size_t xb = 0, ab = 0, qb = 0;
  for (int i = 0; i < 4; ++i) {
    const StageOff& s = e->st[i];
    const size_t M = (size_t)B * s.H * s.H;
    xb = std::max(xb, M * s.Cp * 4); ab = std::max(ab, M * s.Cp * es);
    qb = std::max(qb, M * std::max<size_t>(3 * s.Cp, 4 * s.C) * es);
    if (i > 0) ab = std::max(ab, M * 4 * (size_t)e->st[i - 1].C * es);
  }
  Alloc a; SwinWs w;
  w.status = a.take(256);                   // int32 status word at workspace offset 0 (effocr_swin_check_status)
  w.x = a.take(xb); w.a = a.take(ab); w.q = a.take(qb);
  w.total = a.off;
  return w;
}

int swin_chunk(const effocr_swin* e, int batch) {
  return enc_default_chunk(e, batch, SWIN_WS_BUDGET, SWIN_MAX_CHUNK, [e](int B) { return swin_ws(e, B).total; });
}

// One sub-batch: patch_embed -> 4 stages of [patch merging] + blocks (LN1 -> qkv -> window attention -> proj + residual; LN2 -> fc1 + GELU
// -> fc2 + residual) -> head.  Every GEMM's kernel is chosen by (precision, N, K) alone and reduces K in a fixed order (no split-K):
// a crop's embedding does not depend on B.
int swin_forward(const effocr_swin* e, const float* x, int B, float* emb, int l2, char* ws, hipStream_t s) {
  const SwinWs w = swin_ws(e, B);
  const char* wb = e->wdev;
  const int prec = e->prec;
  auto F = [&](size_t off) { return reinterpret_cast<const float*>(wb + off); };
  float* xs = reinterpret_cast<float*>(ws + w.x);
  void* A = ws + w.a; void* Q = ws + w.q;
  int* status = reinterpret_cast<int*>(ws + w.status);
  int rc;
  auto lin = [&](const void* X, int K, size_t woff, size_t boff, void* out, int N, int epi, int64_t M) {
    LinearExtras r{};
    if (epi == EPI_BIAS_RESID) r.resid = xs;             // added into the residual stream in place
    return dense_linear(prec, epi, X, K, wb + woff, F(boff), out, N, M, r, s);
  };
  if ((rc = swin_stem(x, B, e->img, F(e->stemw), F(e->stemb), F(e->stemlnw), F(e->stemlnb), e->st[0].C, SWIN_EPS, xs, s))) return rc;
  for (int i = 0; i < 4; ++i) {
    const StageOff& st = e->st[i];
    const int C = st.C, Cp = st.Cp, H = st.H;
    const int64_t M = (int64_t)B * H * H;
    if (i > 0) {
      const StageOff& pv = e->st[i - 1];
      if ((rc = swin_merge(prec, xs, B, pv.H, pv.C, pv.Cp, F(st.mlnw), F(st.mlnb), SWIN_EPS, A, s))) return rc;
      if ((rc = lin(A, 4 * pv.C, st.redw, st.redb, xs, Cp, EPI_BIAS_F32, M))) return rc;
    }
    for (int j = 0; j < st.depth; ++j) {
      const BlockOff& L = st.blocks[j];
      if ((rc = swin_layernorm(prec, xs, M, C, Cp, F(L.ln1w), F(L.ln1b), SWIN_EPS, A, s))) return rc;
      if ((rc = lin(A, Cp, L.qkvw, L.qkvb, Q, 3 * Cp, EPI_BIAS, M))) return rc;
      if ((rc = swin_window_attention(prec, Q, B, H, C, Cp, L.shift, F(L.table), A, s))) return rc;
      if ((rc = lin(A, Cp, L.projw, L.projb, xs, Cp, EPI_BIAS_RESID, M))) return rc;
      if ((rc = swin_layernorm(prec, xs, M, C, Cp, F(L.ln2w), F(L.ln2b), SWIN_EPS, A, s))) return rc;
      if ((rc = lin(A, Cp, L.fc1w, L.fc1b, Q, 4 * C, EPI_BIAS_GELU, M))) return rc;
      if ((rc = lin(Q, 4 * C, L.fc2w, L.fc2b, xs, Cp, EPI_BIAS_RESID, M))) return rc;
    }
  }
  const StageOff& last = e->st[3];
  return swin_head(xs, B, last.H * last.H, last.C, last.Cp, F(e->normw), F(e->normb), SWIN_EPS, l2, emb, status, s);
}

}  // namespace
}  // namespace effocr

SWIN_API int effocr_swin_abi_version(void) { return EFFOCR_SWIN_ABI_VERSION; }
SWIN_API const char* effocr_swin_last_error(void) { return g_err.c_str(); }

SWIN_API int effocr_swin_create(const char* arch, int img_size, int precision, effocr_swin_t** out) {
  if (!arch || !out) return fail(EFFOCR_SWIN_EINVAL, "swin_create: NULL argument");
  if (precision < 0 || precision > 2) return fail(EFFOCR_SWIN_EINVAL, "swin_create: unknown precision");
  if (std::string(arch) != "swin_tiny_patch4_window7_224")
    return fail(EFFOCR_SWIN_EUNSUPPORTED, std::string("swin_create: unsupported architecture '") + arch + "'");
  if (img_size != 224)
    return fail(EFFOCR_SWIN_EUNSUPPORTED, "swin_create: img_size must be 224 (the reference builds swin_tiny_patch4_window7_224 at "
                                          "timm's default size; other sizes change the window grid)");
  std::unique_ptr<effocr_swin> e(new effocr_swin());
  e->img = img_size; e->prec = precision; e->D = 768;
  build_swin(e.get());
  *out = e.release();
  return EFFOCR_SWIN_OK;
}

SWIN_API void effocr_swin_destroy(effocr_swin_t* enc) { delete enc; }
SWIN_API int effocr_swin_embed_dim(const effocr_swin_t* enc) { return enc ? enc->D : 0; }
SWIN_API int effocr_swin_num_params(const effocr_swin_t* enc) { return enc ? (int)enc->params.size() : 0; }
SWIN_API const char* effocr_swin_param_name(const effocr_swin_t* enc, int i) { return enc_param_name(enc, i); }
SWIN_API int64_t effocr_swin_param_numel(const effocr_swin_t* enc, int i) { return enc_param_numel(enc, i); }

SWIN_API int effocr_swin_set_param(effocr_swin_t* enc, const char* name, const float* host, int64_t numel) {
  return enc_set_param("swin", enc, name, host, numel);
}

SWIN_API size_t effocr_swin_weights_bytes(const effocr_swin_t* enc) { return enc ? enc->wbytes : 0; }

SWIN_API int effocr_swin_upload(effocr_swin_t* enc, void* weights_dev, size_t bytes) {
  return enc_upload("swin", enc, weights_dev, bytes, pack_swin);
}

SWIN_API size_t effocr_swin_workspace_bytes(const effocr_swin_t* enc, int batch) {
  if (!enc || batch <= 0) return 0;
  return swin_ws(enc, swin_chunk(enc, batch)).total;
}

SWIN_API int effocr_swin_set_chunk(effocr_swin_t* enc, int crops_per_chunk) { return enc_set_chunk("swin", enc, crops_per_chunk); }

SWIN_API int effocr_swin_forward(effocr_swin_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize, void* workspace_dev,
                                 size_t workspace_bytes, void* stream) {
  const int rc = enc_forward_args("swin", enc, x_dev, batch, emb_dev, workspace_dev, workspace_bytes, effocr_swin_workspace_bytes(enc, batch));
  if (rc || batch == 0) return rc;
  const int chunk = swin_chunk(enc, batch);
  const int64_t tok0 = (int64_t)(enc->img / 4) * (enc->img / 4);
  if ((int64_t)chunk * tok0 * std::max(3 * enc->st[0].Cp, 4 * enc->st[0].C) >= (int64_t)1 << 31)
    return fail(EFFOCR_SWIN_EUNSUPPORTED, "swin_forward: chunk too large for 32-bit GEMM indices (effocr_swin_set_chunk)");
  return enc_forward_chunks(enc, x_dev, batch, chunk, emb_dev, [&](const float* x, int crops, float* emb) {
    return swin_forward(enc, x, crops, emb, l2_normalize, static_cast<char*>(workspace_dev), S(stream));
  });
}

SWIN_API int effocr_swin_check_status(const effocr_swin_t* enc, const void* workspace_dev, void* stream) {   // SwinWs::status = offset 0
  return enc_check_status("swin", enc, workspace_dev, stream, ENC_F16_OPERAND_OVERFLOW);
}

// ---- test entry points (tests/test_gpu_swin_ops.py): one launcher each, arguments checked before any launch ----------------------
#define SWIN_OP_PREC(name) if (precision < 0 || precision > 2) return fail(EFFOCR_SWIN_EINVAL, name ": unknown precision")

SWIN_API int effocr_swin_op_stem(const float* x_dev, int batch, int img_size, const float* w_dev, const float* b_dev, const float* lnw_dev,
                                 const float* lnb_dev, int channels, float* out_dev, void* stream) {
  if (!x_dev || !w_dev || !b_dev || !lnw_dev || !lnb_dev || !out_dev) return fail(EFFOCR_SWIN_EINVAL, "swin_op_stem: NULL argument");
  if (batch <= 0 || img_size <= 0 || channels <= 0) return fail(EFFOCR_SWIN_EINVAL, "swin_op_stem: bad geometry");
  if (img_size % 4 || channels > 128 || channels % 4)
    return fail(EFFOCR_SWIN_EUNSUPPORTED, "swin_op_stem: img_size % 4 == 0, channels % 4 == 0 and channels <= 128 required");
  return swin_stem(x_dev, batch, img_size, w_dev, b_dev, lnw_dev, lnb_dev, channels, SWIN_EPS, out_dev, S(stream));
}

SWIN_API int effocr_swin_op_layernorm(int precision, const float* x_dev, int64_t rows, int channels, int padded_channels, const float* lnw_dev,
                                      const float* lnb_dev, void* out_dev, void* stream) {
  if (!x_dev || !lnw_dev || !lnb_dev || !out_dev) return fail(EFFOCR_SWIN_EINVAL, "swin_op_layernorm: NULL argument");
  SWIN_OP_PREC("swin_op_layernorm");
  if (rows <= 0 || channels <= 0 || padded_channels <= 0) return fail(EFFOCR_SWIN_EINVAL, "swin_op_layernorm: bad geometry");
  if (padded_channels % 128 || padded_channels > 1024 || channels > padded_channels || channels % 4)
    return fail(EFFOCR_SWIN_EUNSUPPORTED, "swin_op_layernorm: padded_channels % 128 == 0 (<= 1024), channels % 4 == 0 and channels <= "
                                          "padded_channels required");
  return swin_layernorm(precision, x_dev, rows, channels, padded_channels, lnw_dev, lnb_dev, SWIN_EPS, out_dev, S(stream));
}

SWIN_API int effocr_swin_op_merge(int precision, const float* x_dev, int batch, int map_size, int channels, int padded_channels,
                                  const float* lnw_dev, const float* lnb_dev, void* out_dev, void* stream) {
  if (!x_dev || !lnw_dev || !lnb_dev || !out_dev) return fail(EFFOCR_SWIN_EINVAL, "swin_op_merge: NULL argument");
  SWIN_OP_PREC("swin_op_merge");
  if (batch <= 0 || map_size <= 0 || channels <= 0 || padded_channels <= 0) return fail(EFFOCR_SWIN_EINVAL, "swin_op_merge: bad geometry");
  if (channels % 32 || channels > 384 || channels > padded_channels || padded_channels % 4 || map_size % 2)
    return fail(EFFOCR_SWIN_EUNSUPPORTED, "swin_op_merge: channels % 32 == 0 (<= 384, <= padded_channels), padded_channels % 4 == 0 and an "
                                          "even map_size required");
  return swin_merge(precision, x_dev, batch, map_size, channels, padded_channels, lnw_dev, lnb_dev, SWIN_EPS, out_dev, S(stream));
}

SWIN_API int effocr_swin_op_window_attention(int precision, const void* qkv_dev, int batch, int map_size, int channels, int padded_channels,
                                             int shift, const float* table_dev, void* out_dev, void* stream) {
  if (!qkv_dev || !table_dev || !out_dev) return fail(EFFOCR_SWIN_EINVAL, "swin_op_window_attention: NULL argument");
  SWIN_OP_PREC("swin_op_window_attention");
  if (batch <= 0 || map_size <= 0 || channels <= 0 || padded_channels <= 0)
    return fail(EFFOCR_SWIN_EINVAL, "swin_op_window_attention: bad geometry");
  if (map_size % SWIN_WS || channels % 32 || channels > padded_channels || padded_channels % 8 || shift < 0 || shift >= SWIN_WS ||
      (shift && map_size <= SWIN_WS))
    return fail(EFFOCR_SWIN_EUNSUPPORTED, "swin_op_window_attention: map_size % 7 == 0, channels % 32 == 0 (<= padded_channels), "
                                          "padded_channels % 8 == 0 and 0 <= shift < 7 (0 for a single window) required");
  if ((int64_t)batch * (map_size / SWIN_WS) * (map_size / SWIN_WS) * (channels / 32) >= (int64_t)1 << 31)
    return fail(EFFOCR_SWIN_EUNSUPPORTED, "swin_op_window_attention: more (crop, window, head) workgroups than a grid holds");
  return swin_window_attention(precision, qkv_dev, batch, map_size, channels, padded_channels, shift, table_dev, out_dev, S(stream));
}

SWIN_API int effocr_swin_op_head(const float* x_dev, int batch, int tokens, int channels, int padded_channels, const float* lnw_dev,
                                 const float* lnb_dev, int l2_normalize, float* emb_dev, int* status_dev, void* stream) {
  if (!x_dev || !lnw_dev || !lnb_dev || !emb_dev || !status_dev) return fail(EFFOCR_SWIN_EINVAL, "swin_op_head: NULL argument");
  if (batch <= 0 || tokens <= 0 || channels <= 0 || padded_channels <= 0) return fail(EFFOCR_SWIN_EINVAL, "swin_op_head: bad geometry");
  if (channels % 128 || channels > 1024 || channels > padded_channels || padded_channels % 4)
    return fail(EFFOCR_SWIN_EUNSUPPORTED, "swin_op_head: channels % 128 == 0 (<= 1024, <= padded_channels) and padded_channels % 4 == 0 "
                                          "required");
  return swin_head(x_dev, batch, tokens, channels, padded_channels, lnw_dev, lnb_dev, SWIN_EPS, l2_normalize, emb_dev, status_dev, S(stream));
}

SWIN_API int effocr_swin_op_linear(int precision, int epilogue, const void* x_dev, const void* w_dev, const float* bias_dev, const float* resid_dev,
                                   void* out_dev, int64_t rows, int n, int k, void* stream) {
  if (!x_dev || !w_dev || !bias_dev || !out_dev) return fail(EFFOCR_SWIN_EINVAL, "swin_op_linear: NULL argument");
  SWIN_OP_PREC("swin_op_linear");
  if (epilogue != EPI_BIAS && epilogue != EPI_BIAS_GELU && epilogue != EPI_BIAS_RESID && epilogue != EPI_BIAS_F32)
    return fail(EFFOCR_SWIN_EINVAL, "swin_op_linear: unknown epilogue (0 bias, 1 bias + GELU, 2 bias + residual, 5 bias with fp32 output)");
  if (epilogue == EPI_BIAS_RESID && !resid_dev) return fail(EFFOCR_SWIN_EINVAL, "swin_op_linear: NULL residual");
  if (rows <= 0 || n <= 0 || k <= 0) return fail(EFFOCR_SWIN_EINVAL, "swin_op_linear: bad geometry");
  if (n % 128 || (k * prec_esize(precision)) % 128)
    return fail(EFFOCR_SWIN_EUNSUPPORTED, "swin_op_linear: n % 128 == 0 and rows of k elements a multiple of 128 bytes required");
  if (rows * std::max(n, k) >= (int64_t)1 << 31) return fail(EFFOCR_SWIN_EUNSUPPORTED, "swin_op_linear: rows * max(n, k) beyond 32-bit GEMM indices");
  LinearExtras r{};
  if (epilogue == EPI_BIAS_RESID) r.resid = resid_dev;
  return dense_linear(precision, epilogue, x_dev, k, w_dev, bias_dev, out_dev, n, rows, r, S(stream));
}
