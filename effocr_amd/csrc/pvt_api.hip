// C ABI of libeffocr_pvt.so (include/effocr_pvt.h): the PVTv2 encoder handle (parameter table, host-side packing, forward orchestration
// over pvt.hip's kernels) and the library's own error state.  All device memory is caller-owned; this file allocates host memory only.
//
// Widths.  PVTv2's linears are 32 to 512 wide with K from 32 to 4608: pvt.hip's GEMM takes any N % 32 == 0 and K % 16 == 0, so nothing is
// padded but the stem's 147 taps (to PVT_STEM_K = 160, zero weight columns: exact zeros, never a rounding).
#include "../../include/effocr_pvt.h"
#include "token_core.hpp"
#include "pvt.hpp"

#include <memory>

#define PVT_API extern "C" __attribute__((visibility("default")))

namespace effocr {
namespace {

constexpr float PVT_EPS = 1e-6f;                         // every LayerNorm of timm's pvt_v2.py
// sub-batches: as many crops as keep the workspace under PVT_WS_BUDGET (1 GB < 1 GiB), at most PVT_MAX_CHUNK
constexpr size_t PVT_WS_BUDGET = (size_t)1000 << 20;
constexpr int PVT_MAX_CHUNK = 256;
constexpr int PVT_SR[4] = {8, 4, 2, 1};                  // spatial-reduction ratio per stage

struct PvtCfg { const char* name; int width[4], heads[4], depth[4], ratio[4]; };
constexpr PvtCfg PVT_CFGS[] = {
    {"pvt_v2_b0", {32, 64, 160, 256}, {1, 2, 5, 8}, {2, 2, 2, 2}, {8, 8, 4, 4}},
    {"pvt_v2_b1", {64, 128, 320, 512}, {1, 2, 5, 8}, {2, 2, 2, 2}, {8, 8, 4, 4}},
    {"pvt_v2_b2", {64, 128, 320, 512}, {1, 2, 5, 8}, {3, 4, 6, 3}, {8, 8, 4, 4}},
    {"pvt_v2_b3", {64, 128, 320, 512}, {1, 2, 5, 8}, {3, 4, 18, 3}, {8, 8, 4, 4}},
    {"pvt_v2_b4", {64, 128, 320, 512}, {1, 2, 5, 8}, {3, 8, 27, 3}, {8, 8, 4, 4}},
    {"pvt_v2_b5", {64, 128, 320, 512}, {1, 2, 5, 8}, {3, 6, 40, 3}, {4, 4, 4, 4}},
    {"pvt_v2_mini32_test", {32, 64, 96, 128}, {1, 2, 3, 4}, {1, 1, 1, 1}, {8, 8, 4, 4}},   // miniatures used only by fast tests: head width 32 ...
    {"pvt_v2_mini64_test", {64, 128, 192, 256}, {1, 2, 3, 4}, {1, 1, 2, 1}, {8, 8, 4, 4}}, // ... and 64
};
constexpr const char* PVT_SUPPORTED = "pvt_v2_b0, pvt_v2_b1, pvt_v2_b2, pvt_v2_b3, pvt_v2_b4, pvt_v2_b5";

// one linear or convolution in the blob: W [N][K] in the operand type, bias [N] fp32
struct Lin { size_t w, b; int N, K; std::string key; };
struct Norm { size_t w, b; std::string key; };
struct Block { Norm n1, an, n2; Lin q, kv, proj, sr, fc1, fc2; size_t dww, dwb; std::string dwkey; };
struct Stage { int C, heads, hid, sr, H, M; Lin pe; Norm pen, norm; std::vector<Block> blocks; };   // H: tokens per side, M: keys per crop

}  // namespace
}  // namespace effocr

using namespace effocr;

struct effocr_pvt : EncoderCore {
  Stage st[4];
  size_t x_per = 0, h_per = 0, r_per = 0, kv_per = 0, t_per = 0;   // per-crop elements of the workspace buffers (pvt_ws)
};

namespace effocr {
namespace {

void add_lin(effocr_pvt* e, Alloc& a, Lin& L, const std::string& key, int N, int K, int64_t numel) {
  L.key = key; L.N = N; L.K = K;
  e->add_param(key + ".weight", numel); e->add_param(key + ".bias", N);
  L.w = a.take((size_t)N * K * prec_esize(e->prec)); L.b = a.take((size_t)N * 4);
}
void add_norm(effocr_pvt* e, Alloc& a, Norm& n, const std::string& key, int C) {
  n.key = key;
  e->add_param(key + ".weight", C); e->add_param(key + ".bias", C);
  n.w = a.take((size_t)C * 4); n.b = a.take((size_t)C * 4);
}

// The parameter table in timm's state-dict order (pvt_v2.py: a stage is its downsample, its blocks, its norm) and the blob layout.
void build_pvt(effocr_pvt* e, const PvtCfg& c) {
  Alloc a;
  int H = e->img / 4;
  for (int i = 0; i < 4; ++i) {
    Stage& s = e->st[i];
    s.C = c.width[i]; s.heads = c.heads[i]; s.hid = c.width[i] * c.ratio[i]; s.sr = PVT_SR[i]; s.H = H;
    s.M = (H / s.sr) * (H / s.sr);
    const std::string sp = "stages." + std::to_string(i) + ".";
    if (i == 0) {
      add_lin(e, a, s.pe, "patch_embed.proj", s.C, PVT_STEM_K, (int64_t)s.C * 147);
      add_norm(e, a, s.pen, "patch_embed.norm", s.C);
    } else {
      const int cin = c.width[i - 1];
      add_lin(e, a, s.pe, sp + "downsample.proj", s.C, 9 * cin, (int64_t)s.C * 9 * cin);
      add_norm(e, a, s.pen, sp + "downsample.norm", s.C);
    }
    s.blocks.resize(c.depth[i]);
    for (int j = 0; j < c.depth[i]; ++j) {
      Block& b = s.blocks[j];
      const std::string p = sp + "blocks." + std::to_string(j) + ".";
      add_norm(e, a, b.n1, p + "norm1", s.C);
      add_lin(e, a, b.q, p + "attn.q", s.C, s.C, (int64_t)s.C * s.C);
      add_lin(e, a, b.kv, p + "attn.kv", 2 * s.C, s.C, (int64_t)2 * s.C * s.C);
      add_lin(e, a, b.proj, p + "attn.proj", s.C, s.C, (int64_t)s.C * s.C);
      if (s.sr > 1) {
        add_lin(e, a, b.sr, p + "attn.sr", s.C, s.sr * s.sr * s.C, (int64_t)s.C * s.sr * s.sr * s.C);
        add_norm(e, a, b.an, p + "attn.norm", s.C);
      }
      add_norm(e, a, b.n2, p + "norm2", s.C);
      add_lin(e, a, b.fc1, p + "mlp.fc1", s.hid, s.C, (int64_t)s.hid * s.C);
      b.dwkey = p + "mlp.dwconv";
      e->add_param(b.dwkey + ".weight", (int64_t)s.hid * 9); e->add_param(b.dwkey + ".bias", s.hid);
      b.dww = a.take((size_t)9 * s.hid * 4); b.dwb = a.take((size_t)s.hid * 4);
      add_lin(e, a, b.fc2, p + "mlp.fc2", s.C, s.hid, (int64_t)s.C * s.hid);
    }
    add_norm(e, a, s.norm, sp + "norm", s.C);
    const size_t T = (size_t)H * H;
    e->x_per = std::max(e->x_per, T * s.C);
    e->h_per = std::max(e->h_per, T * s.hid);
    e->r_per = std::max(e->r_per, (size_t)s.M * s.C);
    e->kv_per = std::max(e->kv_per, (size_t)s.M * 2 * s.C);
    e->t_per = std::max(e->t_per, std::max((size_t)s.M * s.C, i == 3 ? T * s.C : (size_t)0));
    H /= 2;
  }
  e->wbytes = a.off;
}

float round_op(float v, int prec) {
  if (prec == PREC_BF16) { const uint32_t u = (uint32_t)f32_to_bf16(v) << 16; float f; memcpy(&f, &u, 4); return f; }
  if (prec == PREC_FP16) return (float)(_Float16)v;
  return v;
}

// a convolution weight [N][Cin][k][k] -> [N][(ky k + kx) Cin + c] in the operand type
void pack_conv(const effocr_pvt* e, std::vector<char>& blob, const Lin& L, int cin, int k) {
  const std::vector<float>& w = e->P(L.key + ".weight");
  std::vector<float> row(L.K);
  const size_t es = prec_esize(e->prec);
  for (int n = 0; n < L.N; ++n) {
    for (int c = 0; c < cin; ++c)
      for (int t = 0; t < k * k; ++t) row[(size_t)t * cin + c] = w[((size_t)n * cin + c) * k * k + t];
    put_op(blob, L.w + (size_t)n * L.K * es, row.data(), L.K, e->prec);
  }
  const Packer p{e, blob};
  p.f32(L.b, L.key + ".bias");
}

// Packing: LayerNorm vectors and biases fp32 as they are; linear weights [N][K] rounded once to the operand type; convolution weights
// re-ordered to the implicit GEMM's k order (the stem's rows zero padded to PVT_STEM_K); depthwise weights rounded, then stored as fp32 in
// [tap][channel] order.
void pack_pvt(const effocr_pvt* e, std::vector<char>& blob) {
  const Packer p{e, blob};
  const size_t es = prec_esize(e->prec);
  auto lin = [&](const Lin& L) { p.op(L.w, L.key + ".weight"); p.f32(L.b, L.key + ".bias"); };
  auto norm = [&](const Norm& n) { p.f32(n.w, n.key + ".weight"); p.f32(n.b, n.key + ".bias"); };
  for (int i = 0; i < 4; ++i) {
    const Stage& s = e->st[i];
    if (i == 0) {
      const std::vector<float>& w = e->P(s.pe.key + ".weight");   // [C0][3][7][7] = [C0][147] in the stem's k order
      for (int n = 0; n < s.C; ++n) put_op(blob, s.pe.w + (size_t)n * PVT_STEM_K * es, w.data() + (size_t)n * 147, 147, e->prec);
      p.f32(s.pe.b, s.pe.key + ".bias");
    } else {
      pack_conv(e, blob, s.pe, e->st[i - 1].C, 3);
    }
    norm(s.pen);
    for (const Block& b : s.blocks) {
      norm(b.n1); lin(b.q); lin(b.kv); lin(b.proj);
      if (s.sr > 1) { pack_conv(e, blob, b.sr, s.C, s.sr); norm(b.an); }
      norm(b.n2); lin(b.fc1); lin(b.fc2);
      const std::vector<float>& w = e->P(b.dwkey + ".weight");    // [hid][1][3][3]
      std::vector<float> wt((size_t)9 * s.hid);
      for (int c = 0; c < s.hid; ++c)
        for (int t = 0; t < 9; ++t) wt[(size_t)t * s.hid + c] = round_op(w[(size_t)c * 9 + t], e->prec);
      put_f32(blob, b.dww, wt.data(), wt.size());
      p.f32(b.dwb, b.dwkey + ".bias");
    }
    norm(s.norm);
  }
}

// workspace of one sub-batch of B crops: status word, the fp32 residual stream X, an fp32 scratch T (reduced rows before their LayerNorm;
// the last stage's normalised tokens), and in the operand type A (LayerNorm and attention outputs), H1 (q; the fc1 output), H2 (the
// depthwise output), R (reduced rows) and KV
struct PvtWs { size_t status, x, t, a, h1, h2, r, kv, total; };
PvtWs pvt_ws(const effocr_pvt* e, int B) {
  const size_t es = prec_esize(e->prec);
  Alloc a; PvtWs w;
  w.status = a.take(256);
  w.x = a.take((size_t)B * e->x_per * 4);
  w.t = a.take((size_t)B * e->t_per * 4);
  w.a = a.take((size_t)B * e->x_per * es);
  w.h1 = a.take((size_t)B * e->h_per * es);
  w.h2 = a.take((size_t)B * e->h_per * es);
  w.r = a.take((size_t)B * e->r_per * es);
  w.kv = a.take((size_t)B * e->kv_per * es);
  w.total = a.off;
  return w;
}

int pvt_chunk(const effocr_pvt* e, int batch) {
  return enc_default_chunk(e, batch, PVT_WS_BUDGET, PVT_MAX_CHUNK, [e](int B) { return pvt_ws(e, B).total; });
}

// convolution (implicit GEMM into the fp32 rows tmp) + LayerNorm of those rows into out (fp32 — may be tmp — or the operand type): the
// patch embeddings and the spatial reduction
int conv_ln(int prec, int amode, const void* in, int B, int side, int cin, int cout, int ksize, int stride, int pad, const void* w, const float* bias,
            const float* lnw, const float* lnb, float* tmp, void* out, int out_f32, hipStream_t s) {
  PvtGemm g{};
  g.amode = amode; g.X = in; g.B = B; g.H = side; g.Cin = cin; g.ksize = ksize; g.stride = stride; g.pad = pad;
  g.W = w; g.bias = bias; g.out = tmp; g.N = cout;
  const int oside = amode == PVT_A_STEM ? side / 4 : (side + 2 * pad - ksize) / stride + 1;
  g.K = amode == PVT_A_STEM ? PVT_STEM_K : ksize * ksize * cin;
  g.rows = (int64_t)B * oside * oside;
  int rc;
  if ((rc = pvt_gemm(prec, PVT_EPI_F32, g, s))) return rc;
  return pvt_layernorm(prec, tmp, g.rows, cout, lnw, lnb, PVT_EPS, out, out_f32, s);
}

// One sub-batch.  Per stage: patch embedding (implicit GEMM + LayerNorm) into the fp32 stream; per block LN1 -> q; reduction (implicit
// GEMM + LayerNorm) -> kv; attention; proj + residual; LN2 -> fc1 -> depthwise 3x3 + GELU -> fc2 + residual; the stage norm into the
// operand rows the next stage's embedding reads, or — last stage — into fp32 rows for the token mean.  Every kernel is chosen by the
// shape alone and reduces in a fixed order: a crop's embedding does not depend on B.
int pvt_forward(const effocr_pvt* e, const float* x, int B, float* emb, int l2, char* ws, hipStream_t s) {
  const PvtWs w = pvt_ws(e, B);
  const char* wb = e->wdev;
  const int prec = e->prec;
  auto F = [&](size_t off) { return reinterpret_cast<const float*>(wb + off); };
  float* xs = reinterpret_cast<float*>(ws + w.x);
  float* T = reinterpret_cast<float*>(ws + w.t);
  void *A = ws + w.a, *H1 = ws + w.h1, *H2 = ws + w.h2, *R = ws + w.r, *KV = ws + w.kv;
  int* status = reinterpret_cast<int*>(ws + w.status);
  auto lin = [&](const void* X, const Lin& L, void* out, int64_t rows, int epi) {
    PvtGemm g{};
    g.amode = PVT_A_DENSE; g.X = X; g.W = wb + L.w; g.bias = F(L.b); g.out = out; g.resid = epi == PVT_EPI_RESID ? xs : nullptr;
    g.rows = rows; g.N = L.N; g.K = L.K;
    return pvt_gemm(prec, epi, g, s);
  };
  auto ln = [&](const float* in, const Norm& n, int64_t rows, int C, void* out, int f32) {
    return pvt_layernorm(prec, in, rows, C, F(n.w), F(n.b), PVT_EPS, out, f32, s);
  };
  int rc;
  for (int i = 0; i < 4; ++i) {
    const Stage& st = e->st[i];
    const int C = st.C, H = st.H;
    const int64_t rows = (int64_t)B * H * H, krows = (int64_t)B * st.M;
    if (i == 0) rc = conv_ln(prec, PVT_A_STEM, x, B, e->img, 3, C, 7, 4, 3, wb + st.pe.w, F(st.pe.b), F(st.pen.w), F(st.pen.b), xs, xs, 1, s);
    else rc = conv_ln(prec, PVT_A_CONV, A, B, 2 * H, e->st[i - 1].C, C, 3, 2, 1, wb + st.pe.w, F(st.pe.b), F(st.pen.w), F(st.pen.b), xs, xs, 1, s);
    if (rc) return rc;
    for (const Block& b : st.blocks) {
      if ((rc = ln(xs, b.n1, rows, C, A, 0))) return rc;
      if ((rc = lin(A, b.q, H1, rows, PVT_EPI_OP))) return rc;
      if (st.sr > 1) {
        if ((rc = conv_ln(prec, PVT_A_CONV, A, B, H, C, C, st.sr, st.sr, 0, wb + b.sr.w, F(b.sr.b), F(b.an.w), F(b.an.b), T, R, 0, s))) return rc;
        if ((rc = lin(R, b.kv, KV, krows, PVT_EPI_OP))) return rc;
      } else {
        if ((rc = lin(A, b.kv, KV, krows, PVT_EPI_OP))) return rc;
      }
      if ((rc = pvt_attention(prec, H1, KV, B, H * H, st.M, st.heads, C / st.heads, A, s))) return rc;
      if ((rc = lin(A, b.proj, xs, rows, PVT_EPI_RESID))) return rc;
      if ((rc = ln(xs, b.n2, rows, C, A, 0))) return rc;
      if ((rc = lin(A, b.fc1, H1, rows, PVT_EPI_OP))) return rc;
      if ((rc = pvt_dwconv_gelu(prec, H1, B, H, H, st.hid, F(b.dww), F(b.dwb), H2, s))) return rc;
      if ((rc = lin(H2, b.fc2, xs, rows, PVT_EPI_RESID))) return rc;
    }
    if (i < 3) rc = ln(xs, st.norm, rows, C, A, 0);
    else rc = ln(xs, st.norm, rows, C, T, 1);
    if (rc) return rc;
  }
  return pvt_pool(T, B, e->st[3].H * e->st[3].H, e->D, l2, emb, status, s);
}

}  // namespace
}  // namespace effocr

PVT_API int effocr_pvt_abi_version(void) { return EFFOCR_PVT_ABI_VERSION; }
PVT_API const char* effocr_pvt_last_error(void) { return g_err.c_str(); }

PVT_API int effocr_pvt_create(const char* arch, int img_size, int precision, effocr_pvt_t** out) {
  if (!arch || !out) return fail(EFFOCR_PVT_EINVAL, "pvt_create: NULL argument");
  if (precision < 0 || precision > 2) return fail(EFFOCR_PVT_EINVAL, "pvt_create: unknown precision");
  const std::string name(arch);
  const PvtCfg* cfg = nullptr;
  for (const PvtCfg& c : PVT_CFGS)
    if (name == c.name) cfg = &c;
  if (!cfg) return fail(EFFOCR_PVT_EUNSUPPORTED, "pvt_create: unsupported architecture '" + name + "' (supported: " + PVT_SUPPORTED + ")");
  if (img_size < 32 || img_size > 224 || img_size % 32) return fail(EFFOCR_PVT_EINVAL, "pvt_create: img_size must be a multiple of 32 from 32 to 224");
  std::unique_ptr<effocr_pvt> e(new effocr_pvt());
  e->img = img_size; e->prec = precision; e->D = cfg->width[3];
  build_pvt(e.get(), *cfg);
  *out = e.release();
  return EFFOCR_PVT_OK;
}

PVT_API void effocr_pvt_destroy(effocr_pvt_t* enc) { delete enc; }
PVT_API int effocr_pvt_embed_dim(const effocr_pvt_t* enc) { return enc ? enc->D : 0; }
PVT_API int effocr_pvt_num_params(const effocr_pvt_t* enc) { return enc ? (int)enc->params.size() : 0; }
PVT_API const char* effocr_pvt_param_name(const effocr_pvt_t* enc, int i) { return enc_param_name(enc, i); }
PVT_API int64_t effocr_pvt_param_numel(const effocr_pvt_t* enc, int i) { return enc_param_numel(enc, i); }

PVT_API int effocr_pvt_set_param(effocr_pvt_t* enc, const char* name, const float* host, int64_t numel) {
  return enc_set_param("pvt", enc, name, host, numel);
}

PVT_API size_t effocr_pvt_weights_bytes(const effocr_pvt_t* enc) { return enc ? enc->wbytes : 0; }

PVT_API int effocr_pvt_upload(effocr_pvt_t* enc, void* weights_dev, size_t bytes) { return enc_upload("pvt", enc, weights_dev, bytes, pack_pvt); }

PVT_API size_t effocr_pvt_workspace_bytes(const effocr_pvt_t* enc, int batch) {
  if (!enc || batch <= 0) return 0;
  return pvt_ws(enc, pvt_chunk(enc, batch)).total;
}

PVT_API int effocr_pvt_set_chunk(effocr_pvt_t* enc, int crops_per_chunk) { return enc_set_chunk("pvt", enc, crops_per_chunk); }

PVT_API int effocr_pvt_forward(effocr_pvt_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize, void* workspace_dev,
                               size_t workspace_bytes, void* stream) {
  const int rc = enc_forward_args("pvt", enc, x_dev, batch, emb_dev, workspace_dev, workspace_bytes, effocr_pvt_workspace_bytes(enc, batch));
  if (rc || batch == 0) return rc;
  return enc_forward_chunks(enc, x_dev, batch, pvt_chunk(enc, batch), emb_dev, [&](const float* x, int crops, float* emb) {
    return pvt_forward(enc, x, crops, emb, l2_normalize, static_cast<char*>(workspace_dev), S(stream));
  });
}

PVT_API int effocr_pvt_check_status(const effocr_pvt_t* enc, const void* workspace_dev, void* stream) {   // PvtWs::status = offset 0
  return enc_check_status("pvt", enc, workspace_dev, stream, ENC_F16_OPERAND_OVERFLOW);
}

PVT_API int effocr_pvt_reset_status(const effocr_pvt_t* enc, void* workspace_dev, void* stream) {
  return enc_reset_status("pvt", enc, workspace_dev, stream);
}

PVT_API int effocr_pvt_op_attention(const void* q_dev, const void* kv_dev, int batch, int n, int m, int heads, int hd, int dtype, void* out_dev,
                                    void* stream) {
  if (batch <= 0) return fail(EFFOCR_PVT_EINVAL, "pvt_op_attention: batch >= 1 required");
  return pvt_attention(dtype, q_dev, kv_dev, batch, n, m, heads, hd, out_dev, S(stream));
}

PVT_API int effocr_pvt_op_dwconv_gelu(const void* in_dev, int batch, int h, int w, int c, const float* w_dev, const float* bias_dev, int dtype,
                                      void* out_dev, void* stream) {
  if (batch <= 0) return fail(EFFOCR_PVT_EINVAL, "pvt_op_dwconv_gelu: batch >= 1 required");
  return pvt_dwconv_gelu(dtype, in_dev, batch, h, w, c, w_dev, bias_dev, out_dev, S(stream));
}

PVT_API int effocr_pvt_op_stem(const float* x_dev, int batch, int img, int cout, const void* w_dev, const float* bias_dev, const float* lnw_dev,
                               const float* lnb_dev, int dtype, float* out_dev, void* stream) {
  if (!lnw_dev || !lnb_dev) return fail(EFFOCR_PVT_EINVAL, "pvt_op_stem: NULL argument");
  if (batch <= 0 || img <= 0) return fail(EFFOCR_PVT_EINVAL, "pvt_op_stem: batch >= 1 and img >= 4 required");
  return conv_ln(dtype, PVT_A_STEM, x_dev, batch, img, 3, cout, 7, 4, 3, w_dev, bias_dev, lnw_dev, lnb_dev, out_dev, out_dev, 1, S(stream));
}

PVT_API int effocr_pvt_op_conv_ln(const void* in_dev, int batch, int side, int cin, int cout, int ksize, int stride, int pad, const void* w_dev,
                                  const float* bias_dev, const float* lnw_dev, const float* lnb_dev, int dtype, float* out_dev, void* stream) {
  if (!lnw_dev || !lnb_dev) return fail(EFFOCR_PVT_EINVAL, "pvt_op_conv_ln: NULL argument");
  if (batch <= 0 || side <= 0 || ksize <= 0 || stride <= 0 || pad < 0 || side + 2 * pad < ksize)
    return fail(EFFOCR_PVT_EINVAL, "pvt_op_conv_ln: bad geometry");
  return conv_ln(dtype, PVT_A_CONV, in_dev, batch, side, cin, cout, ksize, stride, pad, w_dev, bias_dev, lnw_dev, lnb_dev, out_dev, out_dev, 1, S(stream));
}
