// C ABI of libeffocr_mnv3.so (include/effocr_mnv3.h): the MobileNetV3 encoder handle (block list derived from the architecture name,
// parameter table in timm's state-dict order, host-side BN folding and packing, sub-batched forward orchestration) and the library's own
// error state.  The kernels are mnv3g.hip's.  All device memory is caller-owned; this file allocates host memory only.
#include "../../include/effocr_mnv3.h"
#include "common.hpp"
#include "kernels.hpp"
#include "mnv3g.hpp"

#include <math.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <vector>

#define MNV3_API extern "C" __attribute__((visibility("default")))

namespace effocr {

// the error plumbing common.hpp declares, for the kernels linked into this library (its own thread-local message)
static thread_local std::string g_mnv3_err;
void set_error(const std::string& msg) { g_mnv3_err = msg; }
int fail(int code, const std::string& msg) { g_mnv3_err = msg; return code; }
int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EFFOCR_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  return EFFOCR_OK;
}

namespace {

// sub-batches: as many crops as keep the workspace under MG_WS_BUDGET, at most MG_MAX_CHUNK
constexpr size_t MG_WS_BUDGET = (size_t)512 << 20;
constexpr int MG_MAX_CHUNK = 256;

struct Param { std::string name; int64_t numel; std::vector<float> data; bool set; };
struct ConvOff { size_t w = 0, b = 0; };
enum { BLK_DS = 0, BLK_IR = 1, BLK_CN = 2 };
// one block of the table: geometry and blob offsets (pw = expand, dw = depthwise, ser / see = squeeze-excite reduce / expand, pwl = project
// — for a ds block its conv_pw, for the cn block its conv)
struct Block { std::string key; int type, cin, mid, cout, k, stride, se, hs, res; ConvOff pw, dw, ser, see, pwl; };

struct Alloc {
  size_t off = 0;
  size_t take(size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; }
};

uint16_t f32_to_bf16(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN
  u += 0x7fffu + ((u >> 16) & 1u);                                            // round to nearest even
  return (uint16_t)(u >> 16);
}
uint16_t f32_to_f16(float f) { _Float16 h = (_Float16)f; uint16_t u; memcpy(&u, &h, 2); return u; }

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

struct effocr_mnv3 {
  int img = 224, prec = PREC_FP16, D = 0, chunk = 0;
  int stem_c = 16;
  std::vector<Param> params;
  std::map<std::string, int> index;
  std::vector<Block> blocks;
  ConvOff stem, head;
  size_t wbytes = 0;
  const char* wdev = nullptr;
};

namespace effocr {
namespace {

void add_param(effocr_mnv3* e, const std::string& name, int64_t numel) {
  e->index[name] = (int)e->params.size();
  e->params.push_back(Param{name, numel, {}, false});
}
void add_bn(effocr_mnv3* e, const std::string& p, int c) {
  add_param(e, p + ".weight", c); add_param(e, p + ".bias", c);
  add_param(e, p + ".running_mean", c); add_param(e, p + ".running_var", c);
}
void add_se(effocr_mnv3* e, const std::string& p, int c, int r) {
  add_param(e, p + ".se.conv_reduce.weight", (int64_t)r * c); add_param(e, p + ".se.conv_reduce.bias", r);
  add_param(e, p + ".se.conv_expand.weight", (int64_t)c * r); add_param(e, p + ".se.conv_expand.bias", c);
}
const std::vector<float>& P(const effocr_mnv3* e, const std::string& n) { return e->params[e->index.at(n)].data; }

size_t pw_bytes(const effocr_mnv3* e, int N, int K) {
  if (e->prec == PREC_FP32) return (size_t)N * K * 4;
  return (size_t)align_up(N, 16) * align_up(K, 16) * 2;       // zero-padded to whole 16 x 16 MFMA tiles
}

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

  add_param(e, "conv_stem.weight", (int64_t)e->stem_c * 27);
  add_bn(e, "bn1", e->stem_c);
  for (const Block& b : e->blocks) {
    const std::string& p = b.key;
    if (b.type == BLK_DS) {
      add_param(e, p + ".conv_dw.weight", (int64_t)b.cin * b.k * b.k); add_bn(e, p + ".bn1", b.cin);
      if (b.se) add_se(e, p, b.cin, b.se);
      add_param(e, p + ".conv_pw.weight", (int64_t)b.cout * b.cin); add_bn(e, p + ".bn2", b.cout);
    } else if (b.type == BLK_IR) {
      add_param(e, p + ".conv_pw.weight", (int64_t)b.mid * b.cin); add_bn(e, p + ".bn1", b.mid);
      add_param(e, p + ".conv_dw.weight", (int64_t)b.mid * b.k * b.k); add_bn(e, p + ".bn2", b.mid);
      if (b.se) add_se(e, p, b.mid, b.se);
      add_param(e, p + ".conv_pwl.weight", (int64_t)b.cout * b.mid); add_bn(e, p + ".bn3", b.cout);
    } else {
      add_param(e, p + ".conv.weight", (int64_t)b.cout * b.cin); add_bn(e, p + ".bn1", b.cout);
    }
  }
  add_param(e, "conv_head.weight", (int64_t)e->D * cin);
  add_param(e, "conv_head.bias", e->D);

  Alloc a;
  e->stem.w = a.take((size_t)27 * e->stem_c * 4); e->stem.b = a.take((size_t)e->stem_c * 4);
  for (Block& b : e->blocks) {
    if (b.type == BLK_IR) { b.pw.w = a.take(pw_bytes(e, b.mid, b.cin)); b.pw.b = a.take((size_t)b.mid * 4); }
    if (b.type != BLK_CN) { b.dw.w = a.take((size_t)b.k * b.k * b.mid * 4); b.dw.b = a.take((size_t)b.mid * 4); }
    if (b.se) {
      b.ser.w = a.take((size_t)b.se * b.mid * 4); b.ser.b = a.take((size_t)b.se * 4);
      b.see.w = a.take((size_t)b.mid * b.se * 4); b.see.b = a.take((size_t)b.mid * 4);
    }
    const int K = b.type == BLK_CN ? b.cin : b.mid;
    b.pwl.w = a.take(pw_bytes(e, b.cout, K)); b.pwl.b = a.take((size_t)b.cout * 4);
  }
  e->head.w = a.take(pw_bytes(e, e->D, cin)); e->head.b = a.take((size_t)e->D * 4);
  e->wbytes = a.off;
}

// pointwise weight [N][K] fp32 -> the blob: fp32 as it is, else rounded once to the operand type inside a zeroed [N16][K16] frame
void put_pw(const effocr_mnv3* e, std::vector<char>& blob, size_t off, const float* w, int N, int K) {
  if (e->prec == PREC_FP32) { memcpy(blob.data() + off, w, (size_t)N * K * 4); return; }
  const int Kp = (int)align_up(K, 16);
  uint16_t* d = reinterpret_cast<uint16_t*>(blob.data() + off);   // (the blob starts zeroed)
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) d[(size_t)n * Kp + k] = e->prec == PREC_BF16 ? f32_to_bf16(w[(size_t)n * K + k]) : f32_to_f16(w[(size_t)n * K + k]);
}
void put_f32(std::vector<char>& blob, size_t off, const float* v, size_t n) { memcpy(blob.data() + off, v, n * 4); }

// Every BatchNorm (eval, eps 1e-5) folded into the conv in front of it in fp32, as libeffocr_hip.so does for mobilenetv3_small_050:
// w' = w g / sqrt(v + eps), b' = beta - m g / sqrt(v + eps).  Depthwise and stem weights tap-major; SE convs fp32 as they are.
void pack_mnv3(const effocr_mnv3* e, std::vector<char>& blob) {
  std::vector<float> wf, bf;
  auto fold = [&](const std::string& w, const std::string& bn) {
    const auto& W = P(e, w);
    const auto& g = P(e, bn + ".weight"); const auto& be = P(e, bn + ".bias");
    const auto& m = P(e, bn + ".running_mean"); const auto& v = P(e, bn + ".running_var");
    const size_t C = g.size(), per = W.size() / C;
    wf.resize(W.size()); bf.resize(C);
    for (size_t c = 0; c < C; ++c) {
      const float sc = g[c] / sqrtf(v[c] + 1e-5f);
      for (size_t k = 0; k < per; ++k) wf[c * per + k] = W[c * per + k] * sc;
      bf[c] = be[c] - m[c] * sc;
    }
  };
  auto pw = [&](const ConvOff& c, const std::string& w, const std::string& bn, int N, int K) {
    fold(w, bn); put_pw(e, blob, c.w, wf.data(), N, K); put_f32(blob, c.b, bf.data(), bf.size());
  };
  auto tapmajor = [&](const ConvOff& c, const std::string& w, const std::string& bn, int C, int taps) {
    fold(w, bn);
    float* d = reinterpret_cast<float*>(blob.data() + c.w);
    for (int ch = 0; ch < C; ++ch)
      for (int t = 0; t < taps; ++t) d[(size_t)t * C + ch] = wf[(size_t)ch * taps + t];
    put_f32(blob, c.b, bf.data(), bf.size());
  };
  auto plain = [&](const ConvOff& c, const std::string& p) {
    const auto& w = P(e, p + ".weight"); const auto& b = P(e, p + ".bias");
    put_f32(blob, c.w, w.data(), w.size()); put_f32(blob, c.b, b.data(), b.size());
  };
  tapmajor(e->stem, "conv_stem.weight", "bn1", e->stem_c, 27);           // [ci][ky][kx] taps
  for (const Block& b : e->blocks) {
    const std::string& p = b.key;
    if (b.type == BLK_DS) {
      tapmajor(b.dw, p + ".conv_dw.weight", p + ".bn1", b.cin, b.k * b.k);
      pw(b.pwl, p + ".conv_pw.weight", p + ".bn2", b.cout, b.cin);
    } else if (b.type == BLK_IR) {
      pw(b.pw, p + ".conv_pw.weight", p + ".bn1", b.mid, b.cin);
      tapmajor(b.dw, p + ".conv_dw.weight", p + ".bn2", b.mid, b.k * b.k);
      pw(b.pwl, p + ".conv_pwl.weight", p + ".bn3", b.cout, b.mid);
    } else {
      pw(b.pwl, p + ".conv.weight", p + ".bn1", b.cout, b.cin);
    }
    if (b.se) { plain(b.ser, p + ".se.conv_reduce"); plain(b.see, p + ".se.conv_expand"); }
  }
  const Block& last = e->blocks.back();
  put_pw(e, blob, e->head.w, P(e, "conv_head.weight").data(), e->D, last.cout);
  put_f32(blob, e->head.b, P(e, "conv_head.bias").data(), e->D);
}

int out_size(int H, int stride) { return (H - 1) / stride + 1; }           // k x k, pad k / 2

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
  int c = e->chunk;
  if (c <= 0) c = (int)std::min<size_t>(MG_MAX_CHUNK, std::max<size_t>(1, MG_WS_BUDGET / mnv3_ws(e, 1).total));
  return c < batch ? c : batch;
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

hipStream_t S(void* s) { return static_cast<hipStream_t>(s); }

}  // namespace
}  // namespace effocr

MNV3_API int effocr_mnv3_abi_version(void) { return EFFOCR_MNV3_ABI_VERSION; }
MNV3_API const char* effocr_mnv3_last_error(void) { return effocr::g_mnv3_err.c_str(); }

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
MNV3_API const char* effocr_mnv3_param_name(const effocr_mnv3_t* enc, int i) {
  if (!enc || i < 0 || i >= (int)enc->params.size()) return nullptr;
  return enc->params[i].name.c_str();
}
MNV3_API int64_t effocr_mnv3_param_numel(const effocr_mnv3_t* enc, int i) {
  if (!enc || i < 0 || i >= (int)enc->params.size()) return -1;
  return enc->params[i].numel;
}

MNV3_API int effocr_mnv3_set_param(effocr_mnv3_t* enc, const char* name, const float* host, int64_t numel) {
  if (!enc || !name || !host) return fail(EFFOCR_MNV3_EINVAL, "mnv3_set_param: NULL argument");
  auto it = enc->index.find(name);
  if (it == enc->index.end()) return fail(EFFOCR_MNV3_EINVAL, std::string("mnv3_set_param: unknown parameter '") + name + "'");
  Param& p = enc->params[it->second];
  if (p.numel != numel)
    return fail(EFFOCR_MNV3_EINVAL, std::string("mnv3_set_param: '") + name + "' expects " + std::to_string(p.numel) + " elements, got " +
                                        std::to_string(numel));
  p.data.assign(host, host + numel);
  p.set = true;
  return EFFOCR_MNV3_OK;
}

MNV3_API size_t effocr_mnv3_weights_bytes(const effocr_mnv3_t* enc) { return enc ? enc->wbytes : 0; }

MNV3_API int effocr_mnv3_upload(effocr_mnv3_t* enc, void* weights_dev, size_t bytes) {
  if (!enc || !weights_dev) return fail(EFFOCR_MNV3_EINVAL, "mnv3_upload: NULL argument");
  if (bytes < enc->wbytes) return fail(EFFOCR_MNV3_EWORKSPACE, "mnv3_upload: weight buffer too small");
  for (const Param& p : enc->params)
    if (!p.set) return fail(EFFOCR_MNV3_ESTATE, "mnv3_upload: parameter '" + p.name + "' was never set");
  std::vector<char> blob(enc->wbytes, 0);
  pack_mnv3(enc, blob);
  const hipError_t er = hipMemcpy(weights_dev, blob.data(), enc->wbytes, hipMemcpyHostToDevice);
  if (er != hipSuccess) return fail(EFFOCR_MNV3_EHIP, std::string("mnv3_upload: hipMemcpy: ") + hipGetErrorString(er));
  enc->wdev = static_cast<const char*>(weights_dev);
  return EFFOCR_MNV3_OK;
}

MNV3_API size_t effocr_mnv3_workspace_bytes(const effocr_mnv3_t* enc, int batch) {
  if (!enc || batch <= 0) return 0;
  return mnv3_ws(enc, mnv3_chunk(enc, batch)).total;
}

MNV3_API int effocr_mnv3_set_chunk(effocr_mnv3_t* enc, int crops_per_chunk) {
  if (!enc || crops_per_chunk < 0) return fail(EFFOCR_MNV3_EINVAL, "mnv3_set_chunk: bad argument");
  enc->chunk = crops_per_chunk;
  return EFFOCR_MNV3_OK;
}

MNV3_API int effocr_mnv3_forward(effocr_mnv3_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize, void* workspace_dev,
                                 size_t workspace_bytes, void* stream) {
  if (!enc) return fail(EFFOCR_MNV3_EINVAL, "mnv3_forward: NULL encoder");
  if (batch < 0) return fail(EFFOCR_MNV3_EINVAL, "mnv3_forward: negative batch");
  if (batch == 0) return EFFOCR_MNV3_OK;
  if (!x_dev || !emb_dev || !workspace_dev) return fail(EFFOCR_MNV3_EINVAL, "mnv3_forward: NULL device pointer");
  if (!enc->wdev) return fail(EFFOCR_MNV3_ESTATE, "mnv3_forward: weights were not uploaded");
  if (workspace_bytes < effocr_mnv3_workspace_bytes(enc, batch)) return fail(EFFOCR_MNV3_EWORKSPACE, "mnv3_forward: workspace too small");
  const int chunk = mnv3_chunk(enc, batch);
  char* ws = static_cast<char*>(workspace_dev);
  const size_t img_elems = (size_t)3 * enc->img * enc->img;
  // every kernel computes a crop from that crop's data alone: the embeddings are bit-identical for every chunk setting
  for (int b0 = 0; b0 < batch; b0 += chunk) {
    const int cb = std::min(chunk, batch - b0);
    const int rc = mnv3_forward(enc, x_dev + (size_t)b0 * img_elems, cb, emb_dev + (size_t)b0 * enc->D, l2_normalize, ws, S(stream));
    if (rc) return rc;
  }
  return EFFOCR_MNV3_OK;
}

MNV3_API int effocr_mnv3_check_status(const effocr_mnv3_t* enc, const void* workspace_dev, void* stream) {
  if (!enc || !workspace_dev) return fail(EFFOCR_MNV3_EINVAL, "mnv3_check_status: NULL argument");
  int st = 0;
  hipError_t er = hipMemcpyAsync(&st, workspace_dev, sizeof(int), hipMemcpyDeviceToHost, S(stream));   // MgWs::status = offset 0
  if (er == hipSuccess) er = hipStreamSynchronize(S(stream));
  if (er == hipSuccess && st != 0) er = hipMemsetAsync(const_cast<void*>(workspace_dev), 0, sizeof(int), S(stream));   // read-and-clear
  if (er != hipSuccess) return fail(EFFOCR_MNV3_EHIP, std::string("mnv3_check_status: ") + hipGetErrorString(er));
  if (st != 0)
    return fail(EFFOCR_MNV3_EOVERFLOW, enc->prec == PREC_FP16
                    ? "forward: non-finite embedding — an f16 operand overflowed (an activation beyond 65504) or the input was not finite; use "
                      "precision bf16 or fp32 for this checkpoint"
                    : "forward: non-finite embedding — the input crops or the weights hold inf / nan");
  return EFFOCR_MNV3_OK;
}
