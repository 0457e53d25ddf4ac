// C ABI of libeffocr_regnet.so (include/effocr_regnet.h): the RegNetX / RegNetY encoder handle (block list derived from the architecture
// name, parameter table in timm's state-dict order, host-side BN folding in double and packing, sub-batched forward orchestration) and
// the library's own error state.  The kernels are regnet.hip's (stem, grouped 3x3 + tile sums, squeeze-excite gate, shortcut rows, ReLU)
// and mnv3g.hip's (pointwise GEMM, pool, normalise).  All device memory is caller-owned; this file allocates host memory only.
#include "../../include/effocr_regnet.h"
#include "mbconv_pack.hpp"
#include "mnv3g.hpp"
#include "regnet.hpp"

#include <memory>

#define REGNET_API extern "C" __attribute__((visibility("default")))

namespace effocr {
namespace {

// sub-batches: as many crops as keep the workspace under RG_WS_BUDGET, at most RG_MAX_CHUNK
constexpr size_t RG_WS_BUDGET = ((size_t)1 << 30) - 1;
constexpr int RG_MAX_CHUNK = 256;
constexpr int RG_CHUNK_LIMIT = 65535;                       // crops are the grid's z dimension in rg_gconv
constexpr double RG_BN_EPS = 1e-5;

// what the width generator of timm's regnet.py gives for each name (effocr_amd/weights.py: regnet_widths reproduces it from
// w0, wa, wm, depth and the group width; tests/test_regnet_host.py)
struct Model { const char* name; int se, gw; int widths[4], depths[4]; };
const Model MODELS[] = {
    {"regnetx_002", 0, 8, {24, 56, 152, 368}, {1, 1, 4, 7}},    {"regnetx_004", 0, 16, {32, 64, 160, 384}, {1, 2, 7, 12}},
    {"regnetx_006", 0, 24, {48, 96, 240, 528}, {1, 3, 5, 7}},   {"regnetx_008", 0, 16, {64, 128, 288, 672}, {1, 3, 7, 5}},
    {"regnetx_016", 0, 24, {72, 168, 408, 912}, {2, 4, 10, 2}}, {"regnety_002", 1, 8, {24, 56, 152, 368}, {1, 1, 4, 7}},
    {"regnety_004", 1, 8, {48, 104, 208, 440}, {1, 3, 6, 6}},   {"regnety_006", 1, 16, {48, 112, 256, 608}, {1, 3, 7, 4}},
    {"regnety_008", 1, 16, {64, 128, 320, 768}, {1, 3, 8, 2}},  {"regnety_016", 1, 24, {48, 120, 336, 888}, {2, 6, 17, 2}},
    // miniatures used only by fast tests: odd group counts (half-filled channel tiles), every group width
    {"regnetx_mini8_test", 0, 8, {8, 24, 40, 56}, {1, 1, 2, 1}},
    {"regnetx_mini16_test", 0, 16, {16, 32, 48, 80}, {1, 1, 2, 1}},
    {"regnety_mini24_test", 1, 24, {24, 48, 72, 120}, {1, 1, 2, 1}},
};
const char* const SUPPORTED =
    "regnetx_002, regnetx_004, regnetx_006, regnetx_008, regnetx_016, regnety_002, regnety_004, regnety_006, regnety_008, regnety_016";

// one block of the table: geometry and blob offsets (c1 / c2 / c3 = conv1 / conv2 / conv3, ds = downsample, f1 / f2 = se.fc1 / se.fc2)
struct Block { std::string key; int cin, w, stride, se, down; ConvOff c1, c2, c3, ds, f1, f2; };

}  // namespace
}  // namespace effocr

using namespace effocr;

struct effocr_regnet : EncoderCore {
  int gw = 8;
  bool se = false;
  std::vector<Block> blocks;
  ConvOff stem;
};

namespace effocr {
namespace {

// The block list, the parameter table in timm's state-dict order and the blob layout.
void build_regnet(effocr_regnet* e, const Model& m) {
  e->gw = m.gw; e->se = m.se != 0;
  int cin = RG_STEM_C;
  for (int st = 0; st < 4; ++st)
    for (int j = 0; j < m.depths[st]; ++j) {
      Block b;
      b.key = "s" + std::to_string(st + 1) + ".b" + std::to_string(j + 1);
      b.cin = cin; b.w = m.widths[st];
      b.stride = j == 0 ? 2 : 1;
      b.se = m.se ? (int)nearbyint(cin * 0.25) : 0;          // round(the block's INPUT width x 0.25), no make_divisible
      b.down = (b.stride != 1 || cin != b.w) ? 1 : 0;
      e->blocks.push_back(b);
      cin = b.w;
    }
  e->D = cin;
  e->add_param("stem.conv.weight", (int64_t)RG_STEM_C * 27);
  e->add_bn("stem.bn", RG_STEM_C);
  for (const Block& b : e->blocks) {
    const std::string& p = b.key;
    e->add_param(p + ".conv1.conv.weight", (int64_t)b.w * b.cin); e->add_bn(p + ".conv1.bn", b.w);
    e->add_param(p + ".conv2.conv.weight", (int64_t)b.w * e->gw * 9); e->add_bn(p + ".conv2.bn", b.w);
    if (b.se) {
      e->add_param(p + ".se.fc1.weight", (int64_t)b.se * b.w); e->add_param(p + ".se.fc1.bias", b.se);
      e->add_param(p + ".se.fc2.weight", (int64_t)b.w * b.se); e->add_param(p + ".se.fc2.bias", b.w);
    }
    e->add_param(p + ".conv3.conv.weight", (int64_t)b.w * b.w); e->add_bn(p + ".conv3.bn", b.w);
    if (b.down) { e->add_param(p + ".downsample.conv.weight", (int64_t)b.w * b.cin); e->add_bn(p + ".downsample.bn", b.w); }
  }
  Alloc a;
  e->stem.w = a.take((size_t)27 * RG_STEM_C * 4); e->stem.b = a.take((size_t)RG_STEM_C * 4);
  for (Block& b : e->blocks) {
    b.c1.w = a.take(pw_bytes(e->prec, b.w, b.cin)); b.c1.b = a.take((size_t)b.w * 4);
    b.c2.w = a.take(rg_gconv_bytes(e->prec, b.w, e->gw)); b.c2.b = a.take((size_t)b.w * 4);
    if (b.se) {
      b.f1.w = a.take((size_t)b.se * b.w * 4); b.f1.b = a.take((size_t)b.se * 4);
      b.f2.w = a.take((size_t)b.w * b.se * 4); b.f2.b = a.take((size_t)b.w * 4);
    }
    b.c3.w = a.take(pw_bytes(e->prec, b.w, b.w)); b.c3.b = a.take((size_t)b.w * 4);
    if (b.down) { b.ds.w = a.take(pw_bytes(e->prec, b.w, b.cin)); b.ds.b = a.take((size_t)b.w * 4); }
  }
  e->wbytes = a.off;
}

// A BatchNorm (eval) folded into the conv in front of it in DOUBLE, rounded once to fp32: w' = w g / sqrt(v + eps),
// b' = beta - m g / sqrt(v + eps)
void fold_bn(const effocr_regnet* e, const std::string& conv, const std::string& bn, std::vector<float>& wf, std::vector<float>& bf) {
  const auto& W = e->P(conv + ".weight");
  const auto& g = e->P(bn + ".weight"); const auto& be = e->P(bn + ".bias");
  const auto& m = e->P(bn + ".running_mean"); const auto& v = e->P(bn + ".running_var");
  const size_t C = g.size(), per = W.size() / C;
  wf.resize(W.size()); bf.resize(C);
  for (size_t c = 0; c < C; ++c) {
    const double sc = (double)g[c] / sqrt((double)v[c] + RG_BN_EPS);
    for (size_t k = 0; k < per; ++k) wf[c * per + k] = (float)((double)W[c * per + k] * sc);
    bf[c] = (float)((double)be[c] - (double)m[c] * sc);
  }
}

// grouped weight w [C][gw][3][3] fp32 -> the layout of regnet.hpp: fp32 [9][C][gw]; 16-bit [ct][tap][j][16 out][16 in], rounded once,
// zeros where the output and the input channel are in different groups or outside C (dst starts zeroed)
void pack_gconv(int prec, int C, int gw, const float* w, char* dst) {
  if (prec == PREC_FP32) {
    float* d = reinterpret_cast<float*>(dst);
    for (int o = 0; o < C; ++o)
      for (int ci = 0; ci < gw; ++ci)
        for (int t = 0; t < 9; ++t) d[((size_t)t * C + o) * gw + ci] = w[((size_t)o * gw + ci) * 9 + t];
    return;
  }
  uint16_t* d = reinterpret_cast<uint16_t*>(dst);
  const int NKT = rg_nkt(gw), ntiles = (C + 15) / 16;
  for (int ct = 0; ct < ntiles; ++ct) {
    int kt0, nkt;
    rg_window(gw, C, ct, &kt0, &nkt);
    for (int t = 0; t < 9; ++t)
      for (int j = 0; j < nkt; ++j)
        for (int r = 0; r < 16; ++r)
          for (int k = 0; k < 16; ++k) {
            const int o = ct * 16 + r, c = (kt0 + j) * 16 + k;
            if (o >= C || c >= C || o / gw != c / gw) continue;
            const float v = w[((size_t)o * gw + (c - o / gw * gw)) * 9 + t];
            d[(((size_t)ct * 9 + t) * NKT + j) * 256 + r * 16 + k] = prec == PREC_BF16 ? f32_to_bf16(v) : f32_to_f16(v);
          }
  }
}

void pack_regnet(const effocr_regnet* e, std::vector<char>& blob) {
  std::vector<float> wf, bf;
  auto pw = [&](const ConvOff& c, const std::string& p, int N, int K) {
    fold_bn(e, p + ".conv", p + ".bn", wf, bf);
    put_pw(e->prec, blob, c.w, wf.data(), N, K); put_f32(blob, c.b, bf.data(), bf.size());
  };
  fold_bn(e, "stem.conv", "stem.bn", wf, bf);                               // [32][ci][ky][kx] -> tap-major [27][32]
  float* sw = reinterpret_cast<float*>(blob.data() + e->stem.w);
  for (int ch = 0; ch < RG_STEM_C; ++ch)
    for (int t = 0; t < 27; ++t) sw[(size_t)t * RG_STEM_C + ch] = wf[(size_t)ch * 27 + t];
  put_f32(blob, e->stem.b, bf.data(), bf.size());
  for (const Block& b : e->blocks) {
    const std::string& p = b.key;
    pw(b.c1, p + ".conv1", b.w, b.cin);
    fold_bn(e, p + ".conv2.conv", p + ".conv2.bn", wf, bf);
    pack_gconv(e->prec, b.w, e->gw, wf.data(), blob.data() + b.c2.w); put_f32(blob, b.c2.b, bf.data(), bf.size());
    if (b.se) {
      const auto& w1 = e->P(p + ".se.fc1.weight"); const auto& b1 = e->P(p + ".se.fc1.bias");
      const auto& w2 = e->P(p + ".se.fc2.weight"); const auto& b2 = e->P(p + ".se.fc2.bias");
      put_f32(blob, b.f1.w, w1.data(), w1.size()); put_f32(blob, b.f1.b, b1.data(), b1.size());
      float* d = reinterpret_cast<float*>(blob.data() + b.f2.w);              // fc2 [C][R] -> [R][C]
      for (int c = 0; c < b.w; ++c)
        for (int j = 0; j < b.se; ++j) d[(size_t)j * b.w + c] = w2[(size_t)c * b.se + j];
      put_f32(blob, b.f2.b, b2.data(), b2.size());
    }
    pw(b.c3, p + ".conv3", b.w, b.w);
    if (b.down) pw(b.ds, p + ".downsample", b.w, b.cin);
  }
}

// Workspace of one sub-batch of B crops: the status word; two block input / output maps (ping-pong); conv1's output (at the block's
// input resolution); conv2's output; the shortcut's gathered rows and its 1x1 output; the tile sums; the gates.  All fp32.
struct RgWs { size_t status, io[2], t1, t2, rows, sc, part, gate, total; };
RgWs regnet_ws(const effocr_regnet* e, int B) {
  size_t io = 0, t1 = 0, t2 = 0, rows = 0, sc = 0, part = 0, gate = 0;
  int H = e->img / 2;
  io = (size_t)H * H * RG_STEM_C;
  for (const Block& b : e->blocks) {
    const int Ho = out_size(H, b.stride);
    t1 = std::max(t1, (size_t)H * H * b.w);
    t2 = std::max(t2, (size_t)Ho * Ho * b.w);
    if (b.down) {
      if (b.stride == 2) rows = std::max(rows, (size_t)Ho * Ho * b.cin);
      sc = std::max(sc, (size_t)Ho * Ho * b.w);
    }
    if (b.se) { part = std::max(part, (size_t)rg_tiles(Ho) * b.w); gate = std::max(gate, (size_t)b.w); }
    io = std::max(io, (size_t)Ho * Ho * b.w);
    H = Ho;
  }
  Alloc a; RgWs w;
  w.status = a.take(256);                   // int32 status word at workspace offset 0 (effocr_regnet_check_status)
  w.io[0] = a.take(B * io * 4); w.io[1] = a.take(B * io * 4);
  w.t1 = a.take(B * t1 * 4);
  w.t2 = a.take(B * t2 * 4);
  w.rows = a.take(B * rows * 4);
  w.sc = a.take(B * sc * 4);
  w.part = a.take(B * part * 4);
  w.gate = a.take(B * gate * 4);
  w.total = a.off;
  return w;
}

int regnet_chunk(const effocr_regnet* e, int batch) {
  return enc_default_chunk(e, batch, RG_WS_BUDGET, RG_MAX_CHUNK, [e](int B) { return regnet_ws(e, B).total; });
}

// One sub-batch: stem -> blocks -> global average pool -> F.normalize / status.  A block:
//   conv1 1x1 + ReLU (mg_pw) -> conv2 grouped 3x3 + ReLU (+ tile sums) -> [Y: gate] -> [first block of a stage: shortcut rows -> 1x1]
//   -> conv3 1x1 (gate prologue, + shortcut) -> ReLU in place                     4 launches, + 1 for RegNetY, + 2 in a stage's first block
int regnet_forward(const effocr_regnet* e, const float* x, int B, float* emb, int l2, char* ws, hipStream_t s) {
  const RgWs w = regnet_ws(e, B);
  const char* wb = e->wdev;
  auto F = [&](size_t off) { return reinterpret_cast<const float*>(wb + off); };
  auto Wp = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
  float* io[2] = {Wp(w.io[0]), Wp(w.io[1])};
  float *t1 = Wp(w.t1), *t2 = Wp(w.t2), *rows = Wp(w.rows), *sc = Wp(w.sc), *part = Wp(w.part), *gate = Wp(w.gate);
  int* status = reinterpret_cast<int*>(ws + w.status);
  int rc;
  int H = e->img / 2, cur = 0;
  if ((rc = rg_stem(x, B, e->img, F(e->stem.w), F(e->stem.b), io[0], s))) return rc;
  for (const Block& b : e->blocks) {
    const int Ho = out_size(H, b.stride);
    const int64_t M = (int64_t)B * Ho * Ho;
    if ((rc = mg_pw(e->prec, io[cur], (int64_t)B * H * H, b.cin, wb + b.c1.w, b.w, F(b.c1.b), nullptr, 1, MG_ACT_RELU, nullptr, t1, s))) return rc;
    if ((rc = rg_gconv(e->prec, t1, B, H, b.w, b.stride, e->gw, wb + b.c2.w, F(b.c2.b), t2, Ho, b.se ? part : nullptr, s))) return rc;
    if (b.se && (rc = rg_se_gate(part, B, rg_tiles(Ho), Ho * Ho, b.w, b.se, F(b.f1.w), F(b.f1.b), F(b.f2.w), F(b.f2.b), gate, s))) return rc;
    const float* shortcut = io[cur];
    if (b.down) {
      const float* in = io[cur];
      if (b.stride == 2) {
        if ((rc = rg_gather2(io[cur], B, H, b.cin, rows, s))) return rc;
        in = rows;
      }
      if ((rc = mg_pw(e->prec, in, M, b.cin, wb + b.ds.w, b.w, F(b.ds.b), nullptr, 1, MG_ACT_NONE, nullptr, sc, s))) return rc;
      shortcut = sc;
    }
    if ((rc = mg_pw(e->prec, t2, M, b.w, wb + b.c3.w, b.w, F(b.c3.b), b.se ? gate : nullptr, Ho * Ho, MG_ACT_NONE, shortcut, io[cur ^ 1], s)))
      return rc;
    if ((rc = rg_relu(io[cur ^ 1], M * b.w, s))) return rc;
    cur ^= 1;
    H = Ho;
  }
  if ((rc = mg_pool(io[cur], B, H * H, e->D, emb, s))) return rc;
  return mg_finish(emb, B, e->D, l2, status, s);
}

}  // namespace
}  // namespace effocr

REGNET_API int effocr_regnet_abi_version(void) { return EFFOCR_REGNET_ABI_VERSION; }
REGNET_API const char* effocr_regnet_last_error(void) { return g_err.c_str(); }

REGNET_API int effocr_regnet_create(const char* arch, int img_size, int precision, effocr_regnet_t** out) {
  if (!arch || !out) return fail(EFFOCR_REGNET_EINVAL, "regnet_create: NULL argument");
  if (precision < 0 || precision > 2) return fail(EFFOCR_REGNET_EINVAL, "regnet_create: unknown precision");
  const std::string a = arch;
  const Model* m = nullptr;
  for (const Model& c : MODELS)
    if (a == c.name) m = &c;
  if (!m) return fail(EFFOCR_REGNET_EUNSUPPORTED, "regnet_create: unsupported architecture '" + a + "' (supported: " + SUPPORTED + ")");
  if (img_size < 32 || img_size > 4096 || img_size % 32) return fail(EFFOCR_REGNET_EINVAL, "regnet_create: img_size must be a positive multiple of 32 (at most 4096)");
  std::unique_ptr<effocr_regnet> e(new effocr_regnet());
  e->img = img_size; e->prec = precision;
  build_regnet(e.get(), *m);
  *out = e.release();
  return EFFOCR_REGNET_OK;
}

REGNET_API void effocr_regnet_destroy(effocr_regnet_t* enc) { delete enc; }
REGNET_API int effocr_regnet_embed_dim(const effocr_regnet_t* enc) { return enc ? enc->D : 0; }
REGNET_API int effocr_regnet_num_params(const effocr_regnet_t* enc) { return enc ? (int)enc->params.size() : 0; }
REGNET_API const char* effocr_regnet_param_name(const effocr_regnet_t* enc, int i) { return enc_param_name(enc, i); }
REGNET_API int64_t effocr_regnet_param_numel(const effocr_regnet_t* enc, int i) { return enc_param_numel(enc, i); }

REGNET_API int effocr_regnet_set_param(effocr_regnet_t* enc, const char* name, const float* host, int64_t numel) {
  return enc_set_param("regnet", enc, name, host, numel);
}

REGNET_API size_t effocr_regnet_weights_bytes(const effocr_regnet_t* enc) { return enc ? enc->wbytes : 0; }

REGNET_API int effocr_regnet_upload(effocr_regnet_t* enc, void* weights_dev, size_t bytes) {
  return enc_upload("regnet", enc, weights_dev, bytes, pack_regnet);
}

REGNET_API size_t effocr_regnet_workspace_bytes(const effocr_regnet_t* enc, int batch) {
  if (!enc || batch <= 0) return 0;
  return regnet_ws(enc, regnet_chunk(enc, batch)).total;
}

REGNET_API int effocr_regnet_set_chunk(effocr_regnet_t* enc, int crops_per_chunk) {
  if (enc && crops_per_chunk > RG_CHUNK_LIMIT) return fail(EFFOCR_REGNET_EINVAL, "regnet_set_chunk: at most 65535 crops per sub-batch");
  return enc_set_chunk("regnet", enc, crops_per_chunk);
}

REGNET_API int effocr_regnet_forward(effocr_regnet_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize, void* workspace_dev,
                                     size_t workspace_bytes, void* stream) {
  const int rc = enc_forward_args("regnet", enc, x_dev, batch, emb_dev, workspace_dev, workspace_bytes, effocr_regnet_workspace_bytes(enc, batch));
  if (rc || batch == 0) return rc;
  return enc_forward_chunks(enc, x_dev, batch, regnet_chunk(enc, batch), emb_dev, [&](const float* x, int crops, float* emb) {
    return regnet_forward(enc, x, crops, emb, l2_normalize, static_cast<char*>(workspace_dev), S(stream));
  });
}

REGNET_API int effocr_regnet_check_status(const effocr_regnet_t* enc, const void* workspace_dev, void* stream) {   // RgWs::status = offset 0
  return enc_check_status("regnet", enc, workspace_dev, stream, MBCONV_FP16_OVERFLOW);
}

REGNET_API int effocr_regnet_reset_status(const effocr_regnet_t* enc, void* workspace_dev, void* stream) {
  return enc_reset_status("regnet", enc, workspace_dev, stream);
}

// ---------------------------------------------------------------------------------------------------------------------------
REGNET_API int effocr_regnet_op_tiles(int out_size) { return out_size > 0 ? rg_tiles(out_size) : 0; }

static bool gconv_shape_ok(int precision, int channels, int gw) {
  return precision >= 0 && precision <= 2 && (gw == 8 || gw == 16 || gw == 24) && channels > 0 && channels % gw == 0;
}

REGNET_API size_t effocr_regnet_op_gconv_weight_bytes(int precision, int channels, int group_width) {
  return gconv_shape_ok(precision, channels, group_width) ? rg_gconv_bytes(precision, channels, group_width) : 0;
}

REGNET_API int effocr_regnet_op_pack_gconv(int precision, int channels, int group_width, const float* w_host, void* packed_host) {
  if (!w_host || !packed_host) return fail(EFFOCR_REGNET_EINVAL, "regnet_op_pack_gconv: NULL argument");
  if (!gconv_shape_ok(precision, channels, group_width)) return fail(EFFOCR_REGNET_EINVAL, "regnet_op_pack_gconv: bad geometry");
  memset(packed_host, 0, rg_gconv_bytes(precision, channels, group_width));
  pack_gconv(precision, channels, group_width, w_host, static_cast<char*>(packed_host));
  return EFFOCR_REGNET_OK;
}

REGNET_API int effocr_regnet_op_gconv(int precision, const float* in_dev, int batch, int in_size, int channels, int stride, int group_width,
                                      const void* w_dev, const float* b_dev, float* out_dev, float* part_dev, void* stream) {
  if (!in_dev || !w_dev || !b_dev || !out_dev) return fail(EFFOCR_REGNET_EINVAL, "regnet_op_gconv: NULL argument");
  if (batch <= 0 || in_size <= 0 || (stride != 1 && stride != 2) || !gconv_shape_ok(precision, channels, group_width))
    return fail(EFFOCR_REGNET_EINVAL, "regnet_op_gconv: bad geometry");
  return rg_gconv(precision, in_dev, batch, in_size, channels, stride, group_width, w_dev, b_dev, out_dev, out_size(in_size, stride), part_dev,
                  S(stream));
}

REGNET_API int effocr_regnet_op_se_gate(const float* part_dev, int batch, int tiles, int pixels, int channels, int se_width, const float* fc1_w_dev,
                                        const float* fc1_b_dev, const float* fc2_wt_dev, const float* fc2_b_dev, float* gate_dev, void* stream) {
  if (!part_dev || !fc1_w_dev || !fc1_b_dev || !fc2_wt_dev || !fc2_b_dev || !gate_dev) return fail(EFFOCR_REGNET_EINVAL, "regnet_op_se_gate: NULL argument");
  if (batch <= 0 || tiles <= 0 || pixels <= 0) return fail(EFFOCR_REGNET_EINVAL, "regnet_op_se_gate: bad geometry");
  return rg_se_gate(part_dev, batch, tiles, pixels, channels, se_width, fc1_w_dev, fc1_b_dev, fc2_wt_dev, fc2_b_dev, gate_dev, S(stream));
}

REGNET_API int effocr_regnet_op_stem(const float* x_dev, int batch, int img_size, const float* w_dev, const float* b_dev, float* out_dev, void* stream) {
  if (!x_dev || !w_dev || !b_dev || !out_dev) return fail(EFFOCR_REGNET_EINVAL, "regnet_op_stem: NULL argument");
  if (batch <= 0 || img_size <= 0) return fail(EFFOCR_REGNET_EINVAL, "regnet_op_stem: bad geometry");
  return rg_stem(x_dev, batch, img_size, w_dev, b_dev, out_dev, S(stream));
}

REGNET_API int effocr_regnet_op_gather2(const float* in_dev, int batch, int in_size, int channels, float* out_dev, void* stream) {
  if (!in_dev || !out_dev) return fail(EFFOCR_REGNET_EINVAL, "regnet_op_gather2: NULL argument");
  if (batch <= 0 || in_size <= 0) return fail(EFFOCR_REGNET_EINVAL, "regnet_op_gather2: bad geometry");
  return rg_gather2(in_dev, batch, in_size, channels, out_dev, S(stream));
}

REGNET_API int effocr_regnet_op_relu(float* x_dev, int64_t numel, void* stream) {
  if (!x_dev) return fail(EFFOCR_REGNET_EINVAL, "regnet_op_relu: NULL argument");
  return rg_relu(x_dev, numel, S(stream));
}
