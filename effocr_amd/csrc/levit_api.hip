// C ABI of libeffocr_levit.so (include/effocr_levit.h): the LeViT encoder handle (parameter table, BatchNorm folding and host-side
// packing, forward orchestration over levit.hip's kernels and the GEMMs of gemm.hip / gemm2.hip, which this library compiles once more
// with hidden visibility) and the library's own error state.  All device memory is caller-owned; this file allocates host memory only.
//
// Widths.  gemm.hip wants N % 128 == 0 and K % 64 == 0 (16-bit), which 192, 288, 576 (= 2 x 288), 960 and 1440 do not meet.  Every
// linear is therefore packed with its output rows padded to the next multiple of 128 (zero rows, zero bias) and the residual stream, the
// operand rows and the MLP hidden carry those padded widths: a padded column is acc 0 + bias 0 (+ residual 0), hardswish(0) = 0, and it
// meets zero weight columns in the next linear — exact zeros throughout, never a rounding.  The 128-multiples (levit_128s, levit_128,
// levit_256, levit_384) pad nothing.
#include "../../include/effocr_levit.h"
#include "token_core.hpp"
#include "levit.hpp"

#include <math.h>
#include <memory>

#define LEVIT_API extern "C" __attribute__((visibility("default")))

namespace effocr {
namespace {

constexpr double LEVIT_BN_EPS = 1e-5;                    // every BatchNorm of timm's levit.py
// sub-batches: as many crops as keep the workspace under LEVIT_WS_BUDGET (1 GB < 1 GiB), at most LEVIT_MAX_CHUNK
constexpr size_t LEVIT_WS_BUDGET = (size_t)1000 << 20;
constexpr int LEVIT_MAX_CHUNK = 256;

struct LevitCfg { const char* name; int width[3], kd, heads[3], depth[3]; };
constexpr LevitCfg LEVIT_CFGS[] = {
    {"levit_128s", {128, 256, 384}, 16, {4, 6, 8}, {2, 3, 4}},
    {"levit_128", {128, 256, 384}, 16, {4, 8, 12}, {4, 4, 4}},
    {"levit_192", {192, 288, 384}, 32, {3, 5, 6}, {4, 4, 4}},
    {"levit_256", {256, 384, 512}, 32, {4, 6, 8}, {4, 4, 4}},
    {"levit_384", {384, 512, 768}, 32, {6, 9, 12}, {4, 4, 4}},
    {"levit_tiny_test", {128, 128, 128}, 16, {2, 2, 4}, {1, 1, 1}},      // miniatures used only by fast tests: kd 16 ...
    {"levit_tiny32_test", {128, 192, 256}, 32, {1, 3, 2}, {1, 1, 1}},    // ... and kd 32 with a width that needs padding
};
constexpr const char* LEVIT_SUPPORTED = "levit_128s, levit_128, levit_192, levit_256, levit_384";

int pad128(int n) { return (n + 127) / 128 * 128; }

// one LinearNorm in the blob: W [Np][Kp] in the operand type (BN folded, zero padded), bias [Np] fp32
struct Lin { size_t w, b; int N, K, Np, Kp; std::string key; };
struct Mlp { Lin ln1, ln2; };
// an attention block: stride 1 (qkv in one linear, residual) or 2 (kv + q on the sub-sampled rows, no residual)
struct Block { int stride, R, Din, Dout, heads, kd, vd; size_t table; std::string tkey; Lin qkv, q, proj; Mlp mlp; };
struct Conv { size_t w, b; int Cin, Cout; std::string key; };

}  // namespace
}  // namespace effocr

using namespace effocr;

struct effocr_levit : EncoderCore {
  int R0 = 0;                                              // token grid per side after the stem: img / 16
  Conv stem[4];
  std::vector<Block> blocks;
  int Rlast = 0, Dlast_p = 0;
  size_t xs_per = 0, a_per = 0, q_per = 0;                 // per-crop elements of the residual stream, the operand and the wide buffers
};

namespace effocr {
namespace {

void add_linear_norm(effocr_levit* e, Alloc& a, Lin& L, const std::string& key, int N, int K, int Kp) {
  const size_t es = prec_esize(e->prec);
  L.key = key; L.N = N; L.K = K; L.Np = pad128(N); L.Kp = Kp;
  e->add_param(key + ".linear.weight", (int64_t)N * K);
  e->add_bn(key + ".bn", N);
  L.w = a.take((size_t)L.Np * L.Kp * es); L.b = a.take((size_t)L.Np * 4);
}

void add_mlp(effocr_levit* e, Alloc& a, Mlp& m, const std::string& key, int D) {
  add_linear_norm(e, a, m.ln1, key + ".ln1", 2 * D, D, pad128(D));
  add_linear_norm(e, a, m.ln2, key + ".ln2", D, 2 * D, pad128(2 * D));
}

// The parameter table in timm's state-dict order (levit.py, timm >= 0.9: a stage is its downsample, then its blocks) and the blob layout.
void build_levit(effocr_levit* e, const LevitCfg& c) {
  Alloc a;
  int cin = 3;
  for (int i = 0; i < 4; ++i) {
    Conv& cv = e->stem[i];
    cv.Cin = cin; cv.Cout = c.width[0] >> (3 - i); cv.key = "stem.conv" + std::to_string(i + 1);
    e->add_param(cv.key + ".linear.weight", (int64_t)cv.Cout * cin * 9);
    e->add_bn(cv.key + ".bn", cv.Cout);
    cv.w = a.take((size_t)9 * cin * cv.Cout * 4); cv.b = a.take((size_t)cv.Cout * 4);
    cin = cv.Cout;
  }
  int R = e->R0;
  size_t xs = 0, ap = 0, qp = 0;
  // stem activations alternate between the wide and the operand buffer: conv1 -> Q, conv2 -> A, conv3 -> Q, conv4 -> the stream
  qp = std::max<size_t>((size_t)(8 * R) * (8 * R) * e->stem[0].Cout, (size_t)(2 * R) * (2 * R) * e->stem[2].Cout);
  ap = (size_t)(4 * R) * (4 * R) * e->stem[1].Cout;
  for (int st = 0; st < 3; ++st) {
    const int D = c.width[st];
    const std::string sp = "stages." + std::to_string(st) + ".";
    if (st > 0) {
      Block b{};
      b.stride = 2; b.R = R; b.Din = c.width[st - 1]; b.Dout = D; b.kd = c.kd; b.heads = b.Din / c.kd; b.vd = 4 * c.kd;
      const std::string p = sp + "downsample.attn_downsample";
      b.tkey = p + ".attention_biases";
      e->add_param(b.tkey, (int64_t)b.heads * R * R);
      b.table = a.take((size_t)b.heads * R * R * 4);
      add_linear_norm(e, a, b.qkv, p + ".kv", b.heads * (b.kd + b.vd), b.Din, pad128(b.Din));
      add_linear_norm(e, a, b.q, p + ".q.ln", b.heads * b.kd, b.Din, pad128(b.Din));
      add_linear_norm(e, a, b.proj, p + ".proj.ln", D, b.heads * b.vd, b.heads * b.vd);
      add_mlp(e, a, b.mlp, sp + "downsample.mlp", D);
      const int Rq = levit_sub(R);
      const size_t T = (size_t)R * R, Tq = (size_t)Rq * Rq;
      xs = std::max(xs, std::max(T * pad128(b.Din), Tq * pad128(D)));
      ap = std::max(ap, std::max(T * pad128(b.Din), std::max(Tq * (size_t)b.heads * b.vd, Tq * pad128(D))));
      qp = std::max(qp, std::max(T * b.qkv.Np + Tq * b.q.Np, Tq * b.mlp.ln1.Np));
      e->blocks.push_back(b);
      R = Rq;
    }
    for (int j = 0; j < c.depth[st]; ++j) {
      Block b{};
      b.stride = 1; b.R = R; b.Din = b.Dout = D; b.kd = c.kd; b.heads = c.heads[st]; b.vd = 2 * c.kd;
      const std::string p = sp + "blocks." + std::to_string(j) + ".";
      b.tkey = p + "attn.attention_biases";
      e->add_param(b.tkey, (int64_t)b.heads * R * R);
      b.table = a.take((size_t)b.heads * R * R * 4);
      add_linear_norm(e, a, b.qkv, p + "attn.qkv", b.heads * (2 * b.kd + b.vd), D, pad128(D));
      add_linear_norm(e, a, b.proj, p + "attn.proj.ln", D, b.heads * b.vd, b.heads * b.vd);
      add_mlp(e, a, b.mlp, p + "mlp", D);
      const size_t T = (size_t)R * R;
      xs = std::max(xs, T * pad128(D));
      ap = std::max(ap, std::max(T * pad128(D), T * (size_t)b.heads * b.vd));
      qp = std::max(qp, std::max(T * b.qkv.Np, T * b.mlp.ln1.Np));
      e->blocks.push_back(b);
    }
  }
  e->Rlast = R; e->Dlast_p = pad128(c.width[2]);
  e->xs_per = xs; e->a_per = ap; e->q_per = qp;
  e->wbytes = a.off;
}

float round_op(float v, int prec) {
  if (prec == PREC_BF16) { const uint32_t u = (uint32_t)f32_to_bf16(v) << 16; float f; memcpy(&f, &u, 4); return f; }
  if (prec == PREC_FP16) return (float)(_Float16)v;
  return v;
}

// BatchNorm (eval) folded in double: scale[n] = gamma / sqrt(var + eps), shift[n] = beta - mean * scale
void bn_fold(const effocr_levit* e, const std::string& bn, int n, std::vector<double>& scale, std::vector<double>& shift) {
  const auto &g = e->P(bn + ".weight"), &b = e->P(bn + ".bias"), &m = e->P(bn + ".running_mean"), &v = e->P(bn + ".running_var");
  scale.resize(n); shift.resize(n);
  for (int i = 0; i < n; ++i) {
    scale[i] = (double)g[i] / sqrt((double)v[i] + LEVIT_BN_EPS);
    shift[i] = (double)b[i] - (double)m[i] * scale[i];
  }
}

void pack_linear(const effocr_levit* e, std::vector<char>& blob, const Lin& L) {
  std::vector<double> sc, sh;
  bn_fold(e, L.key + ".bn", L.N, sc, sh);
  const std::vector<float>& w = e->P(L.key + ".linear.weight");
  std::vector<float> row(L.Kp, 0.f), bias(L.Np, 0.f);
  const size_t es = prec_esize(e->prec);
  for (int n = 0; n < L.N; ++n) {
    for (int k = 0; k < L.K; ++k) row[k] = (float)((double)w[(size_t)n * L.K + k] * sc[n]);
    put_op(blob, L.w + (size_t)n * L.Kp * es, row.data(), L.Kp, e->prec);
    bias[n] = (float)sh[n];
  }
  put_f32(blob, L.b, bias.data(), bias.size());
}

// Packing: every BatchNorm folded in double into the linear or convolution in front of it, the result rounded once to the operand type
// (stem weights: rounded, then stored as fp32 in [tap][Cout] order); bias tables as they are.
void pack_levit(const effocr_levit* e, std::vector<char>& blob) {
  const Packer p{e, blob};
  for (const Conv& cv : e->stem) {
    std::vector<double> sc, sh;
    bn_fold(e, cv.key + ".bn", cv.Cout, sc, sh);
    const std::vector<float>& w = e->P(cv.key + ".linear.weight");   // [Cout][Cin][3][3]
    std::vector<float> wt((size_t)9 * cv.Cin * cv.Cout), bias(cv.Cout);
    for (int o = 0; o < cv.Cout; ++o) {
      for (int c = 0; c < cv.Cin; ++c)
        for (int t = 0; t < 9; ++t)
          wt[((size_t)t * cv.Cin + c) * cv.Cout + o] = round_op((float)((double)w[((size_t)o * cv.Cin + c) * 9 + t] * sc[o]), e->prec);
      bias[o] = (float)sh[o];
    }
    put_f32(blob, cv.w, wt.data(), wt.size());
    put_f32(blob, cv.b, bias.data(), bias.size());
  }
  for (const Block& b : e->blocks) {
    p.f32(b.table, b.tkey);
    pack_linear(e, blob, b.qkv);
    if (b.stride == 2) pack_linear(e, blob, b.q);
    pack_linear(e, blob, b.proj);
    pack_linear(e, blob, b.mlp.ln1);
    pack_linear(e, blob, b.mlp.ln2);
  }
}

// workspace of one sub-batch of B crops: status word, two fp32 residual streams (a down-sampling block writes the other one), the
// operand buffer A and the wide buffer Q (qkv / kv + q / hidden rows; the stem's activations alternate between Q and A)
struct LevitWs { size_t status, x0, x1, a, q, total; };
LevitWs levit_ws(const effocr_levit* e, int B) {
  const size_t es = prec_esize(e->prec);
  Alloc a; LevitWs w;
  w.status = a.take(256);
  w.x0 = a.take((size_t)B * e->xs_per * 4);
  w.x1 = a.take((size_t)B * e->xs_per * 4);
  w.a = a.take((size_t)B * e->a_per * es);
  w.q = a.take((size_t)B * e->q_per * es);
  w.total = a.off;
  return w;
}

int levit_chunk(const effocr_levit* e, int batch) {
  return enc_default_chunk(e, batch, LEVIT_WS_BUDGET, LEVIT_MAX_CHUNK, [e](int B) { return levit_ws(e, B).total; });
}

// One sub-batch.  Stem: four direct convolutions down to the R0 x R0 token grid, the last one into the fp32 residual stream.  A block:
// stream -> operand rows -> qkv -> attention (+ hardswish) -> proj + residual; operand rows -> ln1 -> hardswish -> ln2 + residual.  A
// down-sampling block projects kv from every row and q from the rows at even grid positions, and its proj starts a new stream.  Every GEMM's
// kernel is chosen by (precision, N, K) alone and reduces K in a fixed order; the attention walks each crop's own keys: a crop's
// embedding does not depend on B.
int levit_forward(const effocr_levit* e, const float* x, int B, float* emb, int l2, char* ws, hipStream_t s) {
  const LevitWs w = levit_ws(e, B);
  const char* wb = e->wdev;
  const int prec = e->prec;
  auto F = [&](size_t off) { return reinterpret_cast<const float*>(wb + off); };
  float* xs = reinterpret_cast<float*>(ws + w.x0);
  float* xo = reinterpret_cast<float*>(ws + w.x1);
  void* A = ws + w.a; char* Q = ws + w.q;
  int* status = reinterpret_cast<int*>(ws + w.status);
  const size_t es = prec_esize(prec);
  const LinearExtras none{};
  auto lin = [&](const void* X, const Lin& L, void* out, int64_t rows, int epi, const LinearExtras& ex) {
    return dense_linear(prec, epi, X, L.Kp, wb + L.w, F(L.b), out, L.Np, rows, ex, s);
  };
  int rc;
  const Conv* cv = e->stem;
  const int Dp0 = pad128(cv[3].Cout);
  if ((rc = levit_conv3x3s2(prec, x, 1, B, e->img, 3, F(cv[0].w), F(cv[0].b), cv[0].Cout, 1, Q, cv[0].Cout, 0, s))) return rc;
  if ((rc = levit_conv3x3s2(prec, Q, 0, B, e->img / 2, cv[1].Cin, F(cv[1].w), F(cv[1].b), cv[1].Cout, 1, A, cv[1].Cout, 0, s))) return rc;
  if ((rc = levit_conv3x3s2(prec, A, 0, B, e->img / 4, cv[2].Cin, F(cv[2].w), F(cv[2].b), cv[2].Cout, 1, Q, cv[2].Cout, 0, s))) return rc;
  if ((rc = levit_conv3x3s2(prec, Q, 0, B, e->img / 8, cv[3].Cin, F(cv[3].w), F(cv[3].b), cv[3].Cout, 0, xs, Dp0, 1, s))) return rc;
  for (const Block& b : e->blocks) {
    const int R = b.R, Rq = b.stride == 2 ? levit_sub(R) : R;
    const int64_t M = (int64_t)B * R * R, Mq = (int64_t)B * Rq * Rq;
    const int Dinp = pad128(b.Din), Dp = pad128(b.Dout);
    if ((rc = levit_cast_rows(prec, xs, B, R, 1, Dinp, A, s))) return rc;
    if ((rc = lin(A, b.qkv, Q, M, EPI_BIAS, none))) return rc;
    LevitQKV qa{};
    if (b.stride == 1) {
      const int hs = 2 * b.kd + b.vd;
      qa = LevitQKV{Q, b.qkv.Np, hs, 0, Q, b.qkv.Np, hs, b.kd, 2 * b.kd};
    } else {
      char* Q2 = Q + (size_t)M * b.qkv.Np * es;            // the q rows behind the kv rows
      if ((rc = levit_cast_rows(prec, xs, B, R, 2, Dinp, A, s))) return rc;
      if ((rc = lin(A, b.q, Q2, Mq, EPI_BIAS, none))) return rc;
      qa = LevitQKV{Q2, b.q.Np, b.kd, 0, Q, b.qkv.Np, b.kd + b.vd, 0, b.kd};
    }
    if ((rc = levit_attention(prec, qa, F(b.table), B, R, b.stride, b.heads, b.kd, b.vd, 1, A, s))) return rc;
    if (b.stride == 1) {
      const LinearExtras r1{xs};
      if ((rc = lin(A, b.proj, xs, Mq, EPI_BIAS_RESID, r1))) return rc;
    } else {
      if ((rc = lin(A, b.proj, xo, Mq, EPI_BIAS_F32, none))) return rc;
      std::swap(xs, xo);
    }
    const LinearExtras r2{xs};
    if ((rc = levit_cast_rows(prec, xs, B, Rq, 1, Dp, A, s))) return rc;
    if ((rc = lin(A, b.mlp.ln1, Q, Mq, EPI_BIAS, none))) return rc;
    if ((rc = levit_hardswish(prec, Q, Mq * b.mlp.ln1.Np, s))) return rc;
    if ((rc = lin(Q, b.mlp.ln2, xs, Mq, EPI_BIAS_RESID, r2))) return rc;
  }
  return levit_pool(xs, B, e->Rlast * e->Rlast, e->D, e->Dlast_p, l2, emb, status, s);
}

// the GEMMs index with 32 bits: the widest matrix of a sub-batch
bool levit_index_ok(const effocr_levit* e, int chunk) {
  return (int64_t)chunk * (int64_t)std::max(e->q_per, std::max(e->a_per, e->xs_per)) < (int64_t)1 << 31;
}

}  // namespace
}  // namespace effocr

LEVIT_API int effocr_levit_abi_version(void) { return EFFOCR_LEVIT_ABI_VERSION; }
LEVIT_API const char* effocr_levit_last_error(void) { return g_err.c_str(); }

LEVIT_API int effocr_levit_create(const char* arch, int img_size, int precision, effocr_levit_t** out) {
  if (!arch || !out) return fail(EFFOCR_LEVIT_EINVAL, "levit_create: NULL argument");
  if (precision < 0 || precision > 2) return fail(EFFOCR_LEVIT_EINVAL, "levit_create: unknown precision");
  const std::string name(arch);
  const LevitCfg* cfg = nullptr;
  for (const LevitCfg& c : LEVIT_CFGS)
    if (name == c.name) cfg = &c;
  if (!cfg) return fail(EFFOCR_LEVIT_EUNSUPPORTED, "levit_create: unsupported architecture '" + name + "' (supported: " + LEVIT_SUPPORTED + ")");
  if (img_size < 32 || img_size > 16 * LEVIT_MAX_R || img_size % 16)
    return fail(EFFOCR_LEVIT_EINVAL, "levit_create: img_size must be a multiple of 16 from 32 to 224");
  std::unique_ptr<effocr_levit> e(new effocr_levit());
  e->img = img_size; e->prec = precision; e->D = cfg->width[2]; e->R0 = img_size / 16;
  build_levit(e.get(), *cfg);
  *out = e.release();
  return EFFOCR_LEVIT_OK;
}

LEVIT_API void effocr_levit_destroy(effocr_levit_t* enc) { delete enc; }
LEVIT_API int effocr_levit_embed_dim(const effocr_levit_t* enc) { return enc ? enc->D : 0; }
LEVIT_API int effocr_levit_num_params(const effocr_levit_t* enc) { return enc ? (int)enc->params.size() : 0; }
LEVIT_API const char* effocr_levit_param_name(const effocr_levit_t* enc, int i) { return enc_param_name(enc, i); }
LEVIT_API int64_t effocr_levit_param_numel(const effocr_levit_t* enc, int i) { return enc_param_numel(enc, i); }

LEVIT_API int effocr_levit_set_param(effocr_levit_t* enc, const char* name, const float* host, int64_t numel) {
  return enc_set_param("levit", enc, name, host, numel);
}

LEVIT_API size_t effocr_levit_weights_bytes(const effocr_levit_t* enc) { return enc ? enc->wbytes : 0; }

LEVIT_API int effocr_levit_upload(effocr_levit_t* enc, void* weights_dev, size_t bytes) {
  return enc_upload("levit", enc, weights_dev, bytes, pack_levit);
}

LEVIT_API size_t effocr_levit_workspace_bytes(const effocr_levit_t* enc, int batch) {
  if (!enc || batch <= 0) return 0;
  return levit_ws(enc, levit_chunk(enc, batch)).total;
}

LEVIT_API int effocr_levit_set_chunk(effocr_levit_t* enc, int crops_per_chunk) { return enc_set_chunk("levit", enc, crops_per_chunk); }

LEVIT_API int effocr_levit_forward(effocr_levit_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize, void* workspace_dev,
                                   size_t workspace_bytes, void* stream) {
  const int rc = enc_forward_args("levit", enc, x_dev, batch, emb_dev, workspace_dev, workspace_bytes, effocr_levit_workspace_bytes(enc, batch));
  if (rc || batch == 0) return rc;
  const int chunk = levit_chunk(enc, batch);
  if (!levit_index_ok(enc, chunk))
    return fail(EFFOCR_LEVIT_EUNSUPPORTED, "levit_forward: chunk too large for 32-bit GEMM indices (effocr_levit_set_chunk)");
  return enc_forward_chunks(enc, x_dev, batch, chunk, emb_dev, [&](const float* x, int crops, float* emb) {
    return levit_forward(enc, x, crops, emb, l2_normalize, static_cast<char*>(workspace_dev), S(stream));
  });
}

LEVIT_API int effocr_levit_check_status(const effocr_levit_t* enc, const void* workspace_dev, void* stream) {   // LevitWs::status = offset 0
  return enc_check_status("levit", enc, workspace_dev, stream, ENC_F16_ACTIVATION_OVERFLOW);
}

LEVIT_API int effocr_levit_reset_status(const effocr_levit_t* enc, void* workspace_dev, void* stream) {
  return enc_reset_status("levit", enc, workspace_dev, stream);
}

LEVIT_API int effocr_levit_op_attention(const void* q_dev, int64_t ldq, int q_head_stride, int q_off, const void* kv_dev, int64_t ldkv,
                                        int kv_head_stride, int k_off, int v_off, const float* bias_dev, int batch, int grid, int stride, int heads,
                                        int kd, int vd, int act, int dtype, void* out_dev, void* stream) {
  if (!q_dev || !kv_dev || !bias_dev || !out_dev) return fail(EFFOCR_LEVIT_EINVAL, "levit_op_attention: NULL argument");
  if (batch <= 0 || heads <= 0) return fail(EFFOCR_LEVIT_EINVAL, "levit_op_attention: bad geometry");
  if (dtype < 0 || dtype > 2) return fail(EFFOCR_LEVIT_EINVAL, "levit_op_attention: unknown precision");
  if (q_off < 0 || k_off < 0 || v_off < 0 || q_off + kd > q_head_stride || k_off + kd > kv_head_stride || v_off + vd > kv_head_stride ||
      (int64_t)heads * q_head_stride > ldq || (int64_t)heads * kv_head_stride > ldkv)
    return fail(EFFOCR_LEVIT_EINVAL, "levit_op_attention: q / k / v do not fit their rows");
  const LevitQKV a{q_dev, ldq, q_head_stride, q_off, kv_dev, ldkv, kv_head_stride, k_off, v_off};
  return levit_attention(dtype, a, bias_dev, batch, grid, stride, heads, kd, vd, act, out_dev, S(stream));
}

LEVIT_API int effocr_levit_op_stem_conv(const void* in_dev, int nchw, int batch, int size, int cin, const float* wt_dev, const float* bias_dev,
                                        int cout, int act, int dtype, void* out_dev, int ldo, int out_f32, void* stream) {
  if (!in_dev || !wt_dev || !bias_dev || !out_dev) return fail(EFFOCR_LEVIT_EINVAL, "levit_op_stem_conv: NULL argument");
  if (batch <= 0 || size <= 0 || size > 224) return fail(EFFOCR_LEVIT_EINVAL, "levit_op_stem_conv: batch >= 1 and 1 <= size <= 224 required");
  if (dtype < 0 || dtype > 2) return fail(EFFOCR_LEVIT_EINVAL, "levit_op_stem_conv: unknown precision");
  return levit_conv3x3s2(dtype, in_dev, nchw, batch, size, cin, wt_dev, bias_dev, cout, act, out_dev, ldo, out_f32, S(stream));
}
