// C ABI of libeffocr_mnv3.so (include/effocr_mnv3.h): the MobileNetV3 encoder handle (block list derived from the architecture name,
// parameter table in timm's state-dict order, host-side BN folding and packing, sub-batched forward orchestration) and the library's own
// error state.  The kernels are mnv3g.hip's.  All device memory is caller-owned; this file allocates host memory only.
#include "../../include/effocr_mnv3.h"
#include "mbconv_pack.hpp"
#include "mnv3g.hpp"

#include <memory>

#define MNV3_API extern "C" __attribute__((visibility("default")))

namespace effocr {
namespace {

// sub-batches: as many crops as keep the workspace under MG_WS_BUDGET, at most MG_MAX_CHUNK
constexpr size_t MG_WS_BUDGET = (size_t)512 << 20;
constexpr int MG_MAX_CHUNK = 256;

enum { BLK_DS = 0, BLK_IR = 1, BLK_CN = 2 };
// one block of the table: geometry and blob offsets (pw = expand, dw = depthwise, ser / see = squeeze-excite reduce / expand, pwl = project
// — for a ds block its conv_pw, for the cn block its conv)
struct Block { std::string key; int type, cin, mid, cout, k, stride, se, hs, res; ConvOff pw, dw, ser, see, pwl; };

// timm layers/helpers.py make_divisible(v, 8, round_limit=0.9)
int make_divisible(double v) {
  int nv = std::max(8, (int)(v + 4.0) / 8 * 8);
  if (nv < 0.9 * v) nv += 8;
  return nv;
}

// timm's arch definitions (_gen_mobilenet_v3), one row per arch-def string: type, repeats, kernel, stride, expansion, channels,
// squeeze-excite ratio (0 = none), hard-swish (0 = "nre", ReLU)
struct DefRow { int stage, type, r, k, s; double e; int c; double se; int hs; };
const DefRow DEF_SMALL[] = {
    {0, BLK_DS, 1, 3, 2, 1.0, 16, 0.25, 0},
    {1, BLK_IR, 1, 3, 2, 4.5, 24, 0.0, 0}, {1, BLK_IR, 1, 3, 1, 3.67, 24, 0.0, 0},
    {2, BLK_IR, 1, 5, 2, 4.0, 40, 0.25, 1}, {2, BLK_IR, 2, 5, 1, 6.0, 40, 0.25, 1},
    {3, BLK_IR, 2, 5, 1, 3.0, 48, 0.25, 1},
    {4, BLK_IR, 3, 5, 2, 6.0, 96, 0.25, 1},
    {5, BLK_CN, 1, 1, 1, 1.0, 576, 0.0, 1},
};
const DefRow DEF_LARGE[] = {
    {0, BLK_DS, 1, 3, 1, 1.0, 16, 0.0, 0},
    {1, BLK_IR, 1, 3, 2, 4.0, 24, 0.0, 0}, {1, BLK_IR, 1, 3, 1, 3.0, 24, 0.0, 0},
    {2, BLK_IR, 3, 5, 2, 3.0, 40, 0.25, 0},
    {3, BLK_IR, 1, 3, 2, 6.0, 80, 0.0, 1}, {3, BLK_IR, 1, 3, 1, 2.5, 80, 0.0, 1}, {3, BLK_IR, 2, 3, 1, 2.3, 80, 0.0, 1},
    {4, BLK_IR, 2, 3, 1, 6.0, 112, 0.25, 1},
    {5, BLK_IR, 3, 5, 2, 6.0, 160, 0.25, 1},
    {6, BLK_CN, 1, 1, 1, 1.0, 960, 0.0, 1},
};

}  // namespace
}  // namespace effocr

using namespace effocr;

struct effocr_mnv3 : EncoderCore {
  int stem_c = 16;
  std::vector<Block> blocks;
  ConvOff stem, head;
};

namespace effocr {
namespace {

// The block list the way timm's _efficientnet_builder derives it, the parameter table in timm's state-dict order (a module's own
// parameters, then its children's) and the blob layout.
void build_mnv3(effocr_mnv3* e, bool large, double mult) {
  e->stem_c = mult < 0.75 ? 16 : make_divisible(16 * mult);   // fix_stem below 0.75
  const DefRow* def = large ? DEF_LARGE : DEF_SMALL;
  const int ndef = large ? (int)(sizeof(DEF_LARGE) / sizeof(DefRow)) : (int)(sizeof(DEF_SMALL) / sizeof(DefRow));
  int cin = e->stem_c, stage = -1, bi = 0;
  for (int d = 0; d < ndef; ++d) {
    const DefRow& r = def[d];
    if (r.stage != stage) { stage = r.stage; bi = 0; }
    for (int rep = 0; rep < r.r; ++rep, ++bi) {
      Block b;
      b.key = "blocks." + std::to_string(stage) + "." + std::to_string(bi);
      b.type = r.type; b.cin = cin; b.k = r.k; b.hs = r.hs;
      b.cout = make_divisible(r.c * mult);
      b.stride = rep == 0 ? r.s : 1;
      b.mid = r.type == BLK_DS ? cin : r.type == BLK_IR ? make_divisible(cin * r.e) : b.cout;
      b.se = r.se > 0 ? make_divisible(b.mid * r.se) : 0;
      b.res = r.type != BLK_CN && b.stride == 1 && cin == b.cout;
      e->blocks.push_back(b);
      cin = b.cout;
    }
  }
  e->D = large ? 1280 : 1024;                                 // conv_head: not scaled by the multiplier

  e->add_param("conv_stem.weight", (int64_t)e->stem_c * 27);
  e->add_bn("bn1", e->stem_c);
  for (const Block& b : e->blocks) {
    const std::string& p = b.key;
    if (b.type == BLK_DS) {
      e->add_param(p + ".conv_dw.weight", (int64_t)b.cin * b.k * b.k); e->add_bn(p + ".bn1", b.cin);
      if (b.se) add_se(e, p, b.cin, b.se);
      e->add_param(p + ".conv_pw.weight", (int64_t)b.cout * b.cin); e->add_bn(p + ".bn2", b.cout);
    } else if (b.type == BLK_IR) {
      e->add_param(p + ".conv_pw.weight", (int64_t)b.mid * b.cin); e->add_bn(p + ".bn1", b.mid);
      e->add_param(p + ".conv_dw.weight", (int64_t)b.mid * b.k * b.k); e->add_bn(p + ".bn2", b.mid);
      if (b.se) add_se(e, p, b.mid, b.se);
      e->add_param(p + ".conv_pwl.weight", (int64_t)b.cout * b.mid); e->add_bn(p + ".bn3", b.cout);
    } else {
      e->add_param(p + ".conv.weight", (int64_t)b.cout * b.cin); e->add_bn(p + ".bn1", b.cout);
    }
  }
  e->add_param("conv_head.weight", (int64_t)e->D * cin);
  e->add_param("conv_head.bias", e->D);

  Alloc a;
  e->stem.w = a.take((size_t)27 * e->stem_c * 4); e->stem.b = a.take((size_t)e->stem_c * 4);
  for (Block& b : e->blocks) {
    if (b.type == BLK_IR) { b.pw.w = a.take(pw_bytes(e->prec, b.mid, b.cin)); b.pw.b = a.take((size_t)b.mid * 4); }
    if (b.type != BLK_CN) { b.dw.w = a.take((size_t)b.k * b.k * b.mid * 4); b.dw.b = a.take((size_t)b.mid * 4); }
    if (b.se) {
      b.ser.w = a.take((size_t)b.se * b.mid * 4); b.ser.b = a.take((size_t)b.se * 4);
      b.see.w = a.take((size_t)b.mid * b.se * 4); b.see.b = a.take((size_t)b.mid * 4);
    }
    const int K = b.type == BLK_CN ? b.cin : b.mid;
    b.pwl.w = a.take(pw_bytes(e->prec, b.cout, K)); b.pwl.b = a.take((size_t)b.cout * 4);
  }
  e->head.w = a.take(pw_bytes(e->prec, e->D, cin)); e->head.b = a.take((size_t)e->D * 4);
  e->wbytes = a.off;
}

// Every BatchNorm (eval, eps 1e-5) folded into the conv in front of it in fp32, as libeffocr_hip.so does for mobilenetv3_small_050:
// w' = w g / sqrt(v + eps), b' = beta - m g / sqrt(v + eps).  Depthwise and stem weights tap-major; SE convs fp32 as they are.
void pack_mnv3(const effocr_mnv3* e, std::vector<char>& blob) {
  BnFolder f{e, blob, 1e-5f};
  auto plain = [&](const ConvOff& c, const std::string& p) {
    const auto& w = e->P(p + ".weight"); const auto& b = e->P(p + ".bias");
    put_f32(blob, c.w, w.data(), w.size()); put_f32(blob, c.b, b.data(), b.size());
  };
  f.tapmajor(e->stem, "conv_stem.weight", "bn1", e->stem_c, 27);           // [ci][ky][kx] taps
  for (const Block& b : e->blocks) {
    const std::string& p = b.key;
    if (b.type == BLK_DS) {
      f.tapmajor(b.dw, p + ".conv_dw.weight", p + ".bn1", b.cin, b.k * b.k);
      f.pw(b.pwl, p + ".conv_pw.weight", p + ".bn2", b.cout, b.cin);
    } else if (b.type == BLK_IR) {
      f.pw(b.pw, p + ".conv_pw.weight", p + ".bn1", b.mid, b.cin);
      f.tapmajor(b.dw, p + ".conv_dw.weight", p + ".bn2", b.mid, b.k * b.k);
      f.pw(b.pwl, p + ".conv_pwl.weight", p + ".bn3", b.cout, b.mid);
    } else {
      f.pw(b.pwl, p + ".conv.weight", p + ".bn1", b.cout, b.cin);
    }
    if (b.se) { plain(b.ser, p + ".se.conv_reduce"); plain(b.see, p + ".se.conv_expand"); }
  }
  const Block& last = e->blocks.back();
  put_pw(e->prec, blob, e->head.w, e->P("conv_head.weight").data(), e->D, last.cout);
  put_f32(blob, e->head.b, e->P("conv_head.bias").data(), e->D);
}

// Workspace of one sub-batch of B crops: the status word; two block input / output maps (ping-pong); the expansion (at the block's input
// resolution; the ConvBnAct's output too); the depthwise output; the squeeze-excite gates; the pooled features.  All fp32.
struct MgWs { size_t status, io[2], exp, dw, gate, pooled, total; };
MgWs mnv3_ws(const effocr_mnv3* e, int B) {
  size_t io = 0, ex = 0, dw = 0, gate = 0;
  int H = e->img / 2;
  io = (size_t)H * H * e->stem_c;
  for (const Block& b : e->blocks) {
    const int Ho = out_size(H, b.stride);
    if (b.type == BLK_CN) { ex = std::max(ex, (size_t)H * H * b.cout); break; }
    if (b.type == BLK_IR) ex = std::max(ex, (size_t)H * H * b.mid);
    dw = std::max(dw, (size_t)Ho * Ho * b.mid);
    io = std::max(io, (size_t)Ho * Ho * b.cout);
    if (b.se) gate = std::max(gate, (size_t)b.mid);
    H = Ho;
  }
  Alloc a; MgWs w;
  w.status = a.take(256);                   // int32 status word at workspace offset 0 (effocr_mnv3_check_status)
  w.io[0] = a.take(B * io * 4); w.io[1] = a.take(B * io * 4);
  w.exp = a.take(B * ex * 4);
  w.dw = a.take(B * dw * 4);
  w.gate = a.take(B * std::max<size_t>(gate, 4) * 4);
  w.pooled = a.take((size_t)B * e->blocks.back().cout * 4);
  w.total = a.off;
  return w;
}

int mnv3_chunk(const effocr_mnv3* e, int batch) {
  return enc_default_chunk(e, batch, MG_WS_BUDGET, MG_MAX_CHUNK, [e](int B) { return mnv3_ws(e, B).total; });
}

// One sub-batch: stem -> blocks -> ConvBnAct -> global average pool -> conv_head (+ hard-swish) -> F.normalize / status.
//   ds block: depthwise -> [SE gate] -> 1x1 (+ residual)                          2-3 launches
//   ir block: 1x1 expand -> depthwise -> [SE gate] -> 1x1 project (+ residual)     3-4 launches
int mnv3_forward(const effocr_mnv3* e, const float* x, int B, float* emb, int l2, char* ws, hipStream_t s) {
  const MgWs w = mnv3_ws(e, B);
  const char* wb = e->wdev;
  auto F = [&](size_t off) { return reinterpret_cast<const float*>(wb + off); };
  float* io[2] = {reinterpret_cast<float*>(ws + w.io[0]), reinterpret_cast<float*>(ws + w.io[1])};
  float* ex = reinterpret_cast<float*>(ws + w.exp);
  float* dw = reinterpret_cast<float*>(ws + w.dw);
  float* gate = reinterpret_cast<float*>(ws + w.gate);
  float* pooled = reinterpret_cast<float*>(ws + w.pooled);
  int* status = reinterpret_cast<int*>(ws + w.status);
  int rc;
  int H = e->img / 2, cur = 0;
  if ((rc = mg_stem(x, B, e->img, F(e->stem.w), F(e->stem.b), io[0], s))) return rc;
  for (const Block& b : e->blocks) {
    const int act = b.hs ? MG_ACT_HS : MG_ACT_RELU;
    if (b.type == BLK_CN) {
      if ((rc = mg_pw(e->prec, io[cur], (int64_t)B * H * H, b.cin, wb + b.pwl.w, b.cout, F(b.pwl.b), nullptr, 1, act, nullptr, ex, s))) return rc;
      if ((rc = mg_pool(ex, B, H * H, b.cout, pooled, s))) return rc;
      break;
    }
    const int Ho = out_size(H, b.stride);
    const float* dwin = io[cur];
    if (b.type == BLK_IR) {
      if ((rc = mg_pw(e->prec, io[cur], (int64_t)B * H * H, b.cin, wb + b.pw.w, b.mid, F(b.pw.b), nullptr, 1, act, nullptr, ex, s))) return rc;
      dwin = ex;
    }
    if ((rc = mg_dw(dwin, B, H, b.mid, b.k, b.stride, F(b.dw.w), F(b.dw.b), act, dw, Ho, s))) return rc;
    if (b.se && (rc = mg_se_gate(dw, B, Ho * Ho, b.mid, b.se, F(b.ser.w), F(b.ser.b), F(b.see.w), F(b.see.b), gate, s))) return rc;
    if ((rc = mg_pw(e->prec, dw, (int64_t)B * Ho * Ho, b.mid, wb + b.pwl.w, b.cout, F(b.pwl.b), b.se ? gate : nullptr, Ho * Ho, MG_ACT_NONE,
                    b.res ? io[cur] : nullptr, io[cur ^ 1], s))) return rc;
    cur ^= 1;
    H = Ho;
  }
  if ((rc = mg_pw(e->prec, pooled, B, e->blocks.back().cout, wb + e->head.w, e->D, F(e->head.b), nullptr, 1, MG_ACT_HS, nullptr, emb, s))) return rc;
  return mg_finish(emb, B, e->D, l2, status, s);
}

}  // namespace
}  // namespace effocr

MNV3_API int effocr_mnv3_abi_version(void) { return EFFOCR_MNV3_ABI_VERSION; }
MNV3_API const char* effocr_mnv3_last_error(void) { return g_err.c_str(); }

MNV3_API int effocr_mnv3_create(const char* arch, int img_size, int precision, effocr_mnv3_t** out) {
  if (!arch || !out) return fail(EFFOCR_MNV3_EINVAL, "mnv3_create: NULL argument");
  if (precision < 0 || precision > 2) return fail(EFFOCR_MNV3_EINVAL, "mnv3_create: unknown precision");
  const std::string a = arch;
  bool large = false; double mult = 0.0;
  if (a == "mobilenetv3_small_050") mult = 0.5;
  else if (a == "mobilenetv3_small_075") mult = 0.75;
  else if (a == "mobilenetv3_small_100") mult = 1.0;
  else if (a == "mobilenetv3_large_100") { large = true; mult = 1.0; }
  else
    return fail(EFFOCR_MNV3_EUNSUPPORTED, "mnv3_create: unsupported architecture '" + a +
                                              "' (mobilenetv3_small_050, mobilenetv3_small_075, mobilenetv3_small_100, mobilenetv3_large_100)");
  if (img_size < 32 || img_size > 224 || img_size % 32) return fail(EFFOCR_MNV3_EINVAL, "mnv3_create: img_size must be a multiple of 32 in [32, 224]");
  std::unique_ptr<effocr_mnv3> e(new effocr_mnv3());
  e->img = img_size; e->prec = precision;
  build_mnv3(e.get(), large, mult);
  if (e->stem_c != MG_STEM_C) return fail(EFFOCR_MNV3_EUNSUPPORTED, "mnv3_create: the stem kernel is built for 16 channels");
  *out = e.release();
  return EFFOCR_MNV3_OK;
}

MNV3_API void effocr_mnv3_destroy(effocr_mnv3_t* enc) { delete enc; }
MNV3_API int effocr_mnv3_embed_dim(const effocr_mnv3_t* enc) { return enc ? enc->D : 0; }
MNV3_API int effocr_mnv3_num_params(const effocr_mnv3_t* enc) { return enc ? (int)enc->params.size() : 0; }
MNV3_API const char* effocr_mnv3_param_name(const effocr_mnv3_t* enc, int i) { return enc_param_name(enc, i); }
MNV3_API int64_t effocr_mnv3_param_numel(const effocr_mnv3_t* enc, int i) { return enc_param_numel(enc, i); }

MNV3_API int effocr_mnv3_set_param(effocr_mnv3_t* enc, const char* name, const float* host, int64_t numel) {
  return enc_set_param("mnv3", enc, name, host, numel);
}

MNV3_API size_t effocr_mnv3_weights_bytes(const effocr_mnv3_t* enc) { return enc ? enc->wbytes : 0; }

MNV3_API int effocr_mnv3_upload(effocr_mnv3_t* enc, void* weights_dev, size_t bytes) {
  return enc_upload("mnv3", enc, weights_dev, bytes, pack_mnv3);
}

MNV3_API size_t effocr_mnv3_workspace_bytes(const effocr_mnv3_t* enc, int batch) {
  if (!enc || batch <= 0) return 0;
  return mnv3_ws(enc, mnv3_chunk(enc, batch)).total;
}

MNV3_API int effocr_mnv3_set_chunk(effocr_mnv3_t* enc, int crops_per_chunk) { return enc_set_chunk("mnv3", enc, crops_per_chunk); }

MNV3_API int effocr_mnv3_forward(effocr_mnv3_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize, void* workspace_dev,
                                 size_t workspace_bytes, void* stream) {
  const int rc = enc_forward_args("mnv3", enc, x_dev, batch, emb_dev, workspace_dev, workspace_bytes, effocr_mnv3_workspace_bytes(enc, batch));
  if (rc || batch == 0) return rc;
  return enc_forward_chunks(enc, x_dev, batch, mnv3_chunk(enc, batch), emb_dev, [&](const float* x, int crops, float* emb) {
    return mnv3_forward(enc, x, crops, emb, l2_normalize, static_cast<char*>(workspace_dev), S(stream));
  });
}

MNV3_API int effocr_mnv3_check_status(const effocr_mnv3_t* enc, const void* workspace_dev, void* stream) {   // MgWs::status = offset 0
  return enc_check_status("mnv3", enc, workspace_dev, stream, MBCONV_FP16_OVERFLOW);
}

// ---------------------------------------------------------------------------------------------------------------------------
// TEST ENTRY POINTS (include/effocr_mnv3.h): thin wrappers over mnv3g.hpp's launchers with their layouts, every argument checked before
// the launch.  No product code calls them.
MNV3_API int effocr_mnv3_op_stem(const float* x_dev, int batch, int img_size, const float* w_dev, const float* b_dev, float* out_dev,
                                 void* stream) {
  if (!x_dev || !w_dev || !b_dev || !out_dev) return fail(EFFOCR_MNV3_EINVAL, "mnv3_op_stem: NULL argument");
  if (batch <= 0 || img_size <= 0) return fail(EFFOCR_MNV3_EINVAL, "mnv3_op_stem: bad geometry");
  if (img_size % 2) return fail(EFFOCR_MNV3_EUNSUPPORTED, "mnv3_op_stem: odd img_size");
  return mg_stem(x_dev, batch, img_size, w_dev, b_dev, out_dev, S(stream));
}

MNV3_API int effocr_mnv3_op_dw(const float* in_dev, int batch, int in_size, int channels, int kernel, int stride, const float* w_dev,
                               const float* b_dev, int act, float* out_dev, void* stream) {
  if (!in_dev || !w_dev || !b_dev || !out_dev) return fail(EFFOCR_MNV3_EINVAL, "mnv3_op_dw: NULL argument");
  if (batch <= 0 || in_size <= 0 || channels <= 0 || act < MG_ACT_NONE || act > MG_ACT_SILU) return fail(EFFOCR_MNV3_EINVAL, "mnv3_op_dw: bad geometry");
  if (channels % 4 || (kernel != 3 && kernel != 5) || (stride != 1 && stride != 2))
    return fail(EFFOCR_MNV3_EUNSUPPORTED, "mnv3_op_dw: channels % 4 == 0, kernel 3 or 5, stride 1 or 2");
  return mg_dw(in_dev, batch, in_size, channels, kernel, stride, w_dev, b_dev, act, out_dev, out_size(in_size, stride), S(stream));
}

MNV3_API int effocr_mnv3_op_se_gate(const float* t_dev, int batch, int pixels, int channels, int se_width, const float* reduce_w_dev,
                                    const float* reduce_b_dev, const float* expand_w_dev, const float* expand_b_dev, float* gate_dev,
                                    void* stream) {
  if (!t_dev || !reduce_w_dev || !reduce_b_dev || !expand_w_dev || !expand_b_dev || !gate_dev)
    return fail(EFFOCR_MNV3_EINVAL, "mnv3_op_se_gate: NULL argument");
  if (batch <= 0 || pixels <= 0 || channels <= 0 || se_width <= 0) return fail(EFFOCR_MNV3_EINVAL, "mnv3_op_se_gate: bad geometry");
  // (mg_se_gate refuses channels > 1024 and se_width > 256: its LDS tables)
  return mg_se_gate(t_dev, batch, pixels, channels, se_width, reduce_w_dev, reduce_b_dev, expand_w_dev, expand_b_dev, gate_dev, S(stream));
}

MNV3_API int effocr_mnv3_op_pw(int precision, const float* a_dev, int64_t rows, int k, const void* w_dev, int n, const float* bias_dev,
                               const float* gate_dev, int pixels_per_crop, int act, const float* resid_dev, float* out_dev, void* stream) {
  if (!a_dev || !w_dev || !bias_dev || !out_dev) return fail(EFFOCR_MNV3_EINVAL, "mnv3_op_pw: NULL argument");
  if (precision < 0 || precision > 2) return fail(EFFOCR_MNV3_EINVAL, "mnv3_op_pw: unknown precision");
  if (rows <= 0 || k <= 0 || n <= 0 || pixels_per_crop <= 0 || act < MG_ACT_NONE || act > MG_ACT_SILU)
    return fail(EFFOCR_MNV3_EINVAL, "mnv3_op_pw: bad geometry");
  if (k % 4 || n % 4) return fail(EFFOCR_MNV3_EUNSUPPORTED, "mnv3_op_pw: K and N must be multiples of 4");
  if (n > 65535 * 64) return fail(EFFOCR_MNV3_EUNSUPPORTED, "mnv3_op_pw: N beyond the grid");
  return mg_pw(precision, a_dev, rows, k, w_dev, n, bias_dev, gate_dev, pixels_per_crop, act, resid_dev, out_dev, S(stream));
}

MNV3_API int effocr_mnv3_op_pool(const float* t_dev, int batch, int pixels, int channels, float* out_dev, void* stream) {
  if (!t_dev || !out_dev) return fail(EFFOCR_MNV3_EINVAL, "mnv3_op_pool: NULL argument");
  if (batch <= 0 || pixels <= 0 || channels <= 0) return fail(EFFOCR_MNV3_EINVAL, "mnv3_op_pool: bad geometry");
  return mg_pool(t_dev, batch, pixels, channels, out_dev, S(stream));
}

MNV3_API int effocr_mnv3_op_finish(float* emb_dev, int batch, int dim, int l2_normalize, int* status_dev, void* stream) {
  if (!emb_dev || !status_dev) return fail(EFFOCR_MNV3_EINVAL, "mnv3_op_finish: NULL argument");
  if (batch <= 0 || dim <= 0) return fail(EFFOCR_MNV3_EINVAL, "mnv3_op_finish: bad geometry");
  return mg_finish(emb_dev, batch, dim, l2_normalize, status_dev, S(stream));
}
