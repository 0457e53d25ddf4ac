// C ABI of libeffocr_effnet.so (include/effocr_effnet.h): the EfficientNet-B0 encoder handle (block list derived from the architecture
// name, parameter table in timm's state-dict order, host-side BN folding and packing, sub-batched forward orchestration) and the library's
// own error state.  The kernels are effnet.hip's (stem, depthwise + tile sums, squeeze-excite gate) and mnv3g.hip's (pointwise GEMM, pool,
// normalise).  All device memory is caller-owned; this file allocates host memory only.
#include "../../include/effocr_effnet.h"
#include "mbconv_pack.hpp"
#include "mnv3g.hpp"
#include "effnet.hpp"

#include <memory>

#define EFFNET_API extern "C" __attribute__((visibility("default")))

namespace effocr {
namespace {

// sub-batches: as many crops as keep the workspace within EF_WS_BUDGET, at most EF_MAX_CHUNK
constexpr size_t EF_WS_BUDGET = (size_t)512 << 20;
constexpr int EF_MAX_CHUNK = 256;
constexpr int EF_CHUNK_LIMIT = 65535;                       // crops are the grid's z dimension in ef_dw
constexpr int EF_D = 1280;

enum { BLK_DS = 0, BLK_IR = 1 };
// one block of the table: geometry and blob offsets (pw = expand, dw = depthwise, ser / see = squeeze-excite reduce / expand, pwl = project
// — for the ds block its conv_pw)
struct Block { std::string key; int type, cin, mid, cout, k, stride, se, res; ConvOff pw, dw, ser, see, pwl; };

// timm's arch definition (_gen_efficientnet), one row per stage: type, repeats, kernel, stride of the first repeat, expansion, channels.
// Every block has squeeze-excite at ratio 0.25 of its INPUT channels; at multipliers 1.0 / 1.0 no count is rounded.
struct DefRow { int type, r, k, s, e, c; };
const DefRow DEF_B0[] = {
    {BLK_DS, 1, 3, 1, 1, 16}, {BLK_IR, 2, 3, 2, 6, 24}, {BLK_IR, 2, 5, 2, 6, 40}, {BLK_IR, 3, 3, 2, 6, 80},
    {BLK_IR, 3, 5, 1, 6, 112}, {BLK_IR, 4, 5, 2, 6, 192}, {BLK_IR, 1, 3, 1, 6, 320},
};

}  // namespace
}  // namespace effocr

using namespace effocr;

struct effocr_effnet : EncoderCore {
  bool tf = false;                     // TensorFlow SAME padding and BN eps 1e-3
  std::vector<Block> blocks;
  ConvOff stem, head;
};

namespace effocr {
namespace {

// The block list the way timm's _efficientnet_builder derives it, the parameter table in timm's state-dict order (a module's own
// parameters, then its children's) and the blob layout.
void build_effnet(effocr_effnet* e) {
  int cin = EF_STEM_C, stage = 0;
  for (const DefRow& r : DEF_B0) {
    for (int rep = 0; rep < r.r; ++rep) {
      Block b;
      b.key = "blocks." + std::to_string(stage) + "." + std::to_string(rep);
      b.type = r.type; b.cin = cin; b.k = r.k; b.cout = r.c;
      b.stride = rep == 0 ? r.s : 1;
      b.mid = cin * r.e;
      b.se = (int)nearbyint(cin * 0.25);                      // round(in_chs x se_ratio), no make_divisible (8, 4, 6, 10, 20, 28, 48)
      b.res = b.stride == 1 && cin == b.cout;
      e->blocks.push_back(b);
      cin = b.cout;
    }
    ++stage;
  }
  e->add_param("conv_stem.weight", (int64_t)EF_STEM_C * 27);
  e->add_bn("bn1", EF_STEM_C);
  for (const Block& b : e->blocks) {
    const std::string& p = b.key;
    if (b.type == BLK_DS) {
      e->add_param(p + ".conv_dw.weight", (int64_t)b.cin * b.k * b.k); e->add_bn(p + ".bn1", b.cin);
      add_se(e, p, b.cin, b.se);
      e->add_param(p + ".conv_pw.weight", (int64_t)b.cout * b.cin); e->add_bn(p + ".bn2", b.cout);
    } else {
      e->add_param(p + ".conv_pw.weight", (int64_t)b.mid * b.cin); e->add_bn(p + ".bn1", b.mid);
      e->add_param(p + ".conv_dw.weight", (int64_t)b.mid * b.k * b.k); e->add_bn(p + ".bn2", b.mid);
      add_se(e, p, b.mid, b.se);
      e->add_param(p + ".conv_pwl.weight", (int64_t)b.cout * b.mid); e->add_bn(p + ".bn3", b.cout);
    }
  }
  e->add_param("conv_head.weight", (int64_t)EF_D * cin);
  e->add_bn("bn2", EF_D);

  Alloc a;
  e->stem.w = a.take((size_t)27 * EF_STEM_C * 4); e->stem.b = a.take((size_t)EF_STEM_C * 4);
  for (Block& b : e->blocks) {
    if (b.type == BLK_IR) { b.pw.w = a.take(pw_bytes(e->prec, b.mid, b.cin)); b.pw.b = a.take((size_t)b.mid * 4); }
    b.dw.w = a.take((size_t)b.k * b.k * b.mid * 4); b.dw.b = a.take((size_t)b.mid * 4);
    b.ser.w = a.take((size_t)b.se * b.mid * 4); b.ser.b = a.take((size_t)b.se * 4);
    b.see.w = a.take((size_t)b.mid * b.se * 4); b.see.b = a.take((size_t)b.mid * 4);
    b.pwl.w = a.take(pw_bytes(e->prec, b.cout, b.mid)); b.pwl.b = a.take((size_t)b.cout * 4);
  }
  e->head.w = a.take(pw_bytes(e->prec, EF_D, cin)); e->head.b = a.take((size_t)EF_D * 4);
  e->wbytes = a.off;
}

// Every BatchNorm (eval; eps 1e-5, tf_: 1e-3) folded into the conv in front of it in fp32: w' = w g / sqrt(v + eps),
// b' = beta - m g / sqrt(v + eps).  Depthwise and stem weights tap-major; SE reduce as it is, SE expand transposed to [R][C].
void pack_effnet(const effocr_effnet* e, std::vector<char>& blob) {
  BnFolder f{e, blob, e->tf ? 1e-3f : 1e-5f};
  f.tapmajor(e->stem, "conv_stem.weight", "bn1", EF_STEM_C, 27);           // [ci][ky][kx] taps
  for (const Block& b : e->blocks) {
    const std::string& p = b.key;
    if (b.type == BLK_DS) {
      f.tapmajor(b.dw, p + ".conv_dw.weight", p + ".bn1", b.cin, b.k * b.k);
      f.pw(b.pwl, p + ".conv_pw.weight", p + ".bn2", b.cout, b.cin);
    } else {
      f.pw(b.pw, p + ".conv_pw.weight", p + ".bn1", b.mid, b.cin);
      f.tapmajor(b.dw, p + ".conv_dw.weight", p + ".bn2", b.mid, b.k * b.k);
      f.pw(b.pwl, p + ".conv_pwl.weight", p + ".bn3", b.cout, b.mid);
    }
    const auto& rw = e->P(p + ".se.conv_reduce.weight"); const auto& rb = e->P(p + ".se.conv_reduce.bias");
    const auto& ew = e->P(p + ".se.conv_expand.weight"); const auto& eb = e->P(p + ".se.conv_expand.bias");
    put_f32(blob, b.ser.w, rw.data(), rw.size()); put_f32(blob, b.ser.b, rb.data(), rb.size());
    float* d = reinterpret_cast<float*>(blob.data() + b.see.w);
    for (int c = 0; c < b.mid; ++c)
      for (int j = 0; j < b.se; ++j) d[(size_t)j * b.mid + c] = ew[(size_t)c * b.se + j];
    put_f32(blob, b.see.b, eb.data(), eb.size());
  }
  f.pw(e->head, "conv_head.weight", "bn2", EF_D, e->blocks.back().cout);
}

// Workspace of one sub-batch of B crops: the status word; two block input / output maps (ping-pong); the expansion (at the block's input
// resolution; conv_head's output too); the depthwise output; its tile sums; the squeeze-excite gates.  All fp32.
struct EfWs { size_t status, io[2], exp, dw, part, gate, total; };
EfWs effnet_ws(const effocr_effnet* e, int B) {
  size_t io = 0, ex = 0, dw = 0, part = 0, gate = 0;
  int H = e->img / 2;
  io = (size_t)H * H * EF_STEM_C;
  for (const Block& b : e->blocks) {
    const int Ho = out_size(H, b.stride);
    if (b.type == BLK_IR) ex = std::max(ex, (size_t)H * H * b.mid);
    dw = std::max(dw, (size_t)Ho * Ho * b.mid);
    part = std::max(part, (size_t)ef_tiles(Ho) * b.mid);
    io = std::max(io, (size_t)Ho * Ho * b.cout);
    gate = std::max(gate, (size_t)b.mid);
    H = Ho;
  }
  ex = std::max(ex, (size_t)H * H * EF_D);
  Alloc a; EfWs w;
  w.status = a.take(256);                   // int32 status word at workspace offset 0 (effocr_effnet_check_status)
  w.io[0] = a.take(B * io * 4); w.io[1] = a.take(B * io * 4);
  w.exp = a.take(B * ex * 4);
  w.dw = a.take(B * dw * 4);
  w.part = a.take(B * part * 4);
  w.gate = a.take(B * gate * 4);
  w.total = a.off;
  return w;
}

int effnet_chunk(const effocr_effnet* e, int batch) {
  return enc_default_chunk(e, batch, EF_WS_BUDGET, EF_MAX_CHUNK, [e](int B) { return effnet_ws(e, B).total; });
}

// One sub-batch: stem -> 16 blocks -> conv_head (+ bn2 + SiLU) -> global average pool -> F.normalize / status.
//   ds block: depthwise (+ tile sums) -> SE gate -> 1x1                                        3 launches
//   ir block: 1x1 expand -> depthwise (+ tile sums) -> SE gate -> 1x1 project (+ residual)     4 launches
// 1 + 3 + 15 x 4 + 3 = 67 launches.
int effnet_forward(const effocr_effnet* e, const float* x, int B, float* emb, int l2, char* ws, hipStream_t s) {
  const EfWs w = effnet_ws(e, B);
  const char* wb = e->wdev;
  auto F = [&](size_t off) { return reinterpret_cast<const float*>(wb + off); };
  float* io[2] = {reinterpret_cast<float*>(ws + w.io[0]), reinterpret_cast<float*>(ws + w.io[1])};
  float* ex = reinterpret_cast<float*>(ws + w.exp);
  float* dw = reinterpret_cast<float*>(ws + w.dw);
  float* part = reinterpret_cast<float*>(ws + w.part);
  float* gate = reinterpret_cast<float*>(ws + w.gate);
  int* status = reinterpret_cast<int*>(ws + w.status);
  int rc;
  int H = e->img / 2, cur = 0;
  if ((rc = ef_stem(x, B, e->img, e->tf ? 0 : 1, F(e->stem.w), F(e->stem.b), io[0], s))) return rc;
  for (const Block& b : e->blocks) {
    const int Ho = out_size(H, b.stride);
    const float* dwin = io[cur];
    if (b.type == BLK_IR) {
      if ((rc = mg_pw(e->prec, io[cur], (int64_t)B * H * H, b.cin, wb + b.pw.w, b.mid, F(b.pw.b), nullptr, 1, MG_ACT_SILU, nullptr, ex, s))) return rc;
      dwin = ex;
    }
    const int padb = (e->tf && b.stride == 2) ? b.k / 2 - 1 : b.k / 2;    // SAME on an even map at stride 2: one less before than after
    if ((rc = ef_dw(dwin, B, H, b.mid, b.k, b.stride, padb, F(b.dw.w), F(b.dw.b), dw, Ho, part, s))) return rc;
    if ((rc = ef_se_gate(part, B, ef_tiles(Ho), Ho * Ho, b.mid, b.se, F(b.ser.w), F(b.ser.b), F(b.see.w), F(b.see.b), gate, s))) return rc;
    if ((rc = mg_pw(e->prec, dw, (int64_t)B * Ho * Ho, b.mid, wb + b.pwl.w, b.cout, F(b.pwl.b), gate, Ho * Ho, MG_ACT_NONE,
                    b.res ? io[cur] : nullptr, io[cur ^ 1], s))) return rc;
    cur ^= 1;
    H = Ho;
  }
  if ((rc = mg_pw(e->prec, io[cur], (int64_t)B * H * H, e->blocks.back().cout, wb + e->head.w, EF_D, F(e->head.b), nullptr, 1, MG_ACT_SILU,
                  nullptr, ex, s))) return rc;
  if ((rc = mg_pool(ex, B, H * H, EF_D, emb, s))) return rc;
  return mg_finish(emb, B, EF_D, l2, status, s);
}

}  // namespace
}  // namespace effocr

EFFNET_API int effocr_effnet_abi_version(void) { return EFFOCR_EFFNET_ABI_VERSION; }
EFFNET_API const char* effocr_effnet_last_error(void) { return g_err.c_str(); }

EFFNET_API int effocr_effnet_create(const char* arch, int img_size, int precision, effocr_effnet_t** out) {
  if (!arch || !out) return fail(EFFOCR_EFFNET_EINVAL, "effnet_create: NULL argument");
  if (precision < 0 || precision > 2) return fail(EFFOCR_EFFNET_EINVAL, "effnet_create: unknown precision");
  const std::string a = arch;
  bool tf = false;
  if (a == "efficientnet_b0") tf = false;
  else if (a == "tf_efficientnet_b0") tf = true;
  else
    return fail(EFFOCR_EFFNET_EUNSUPPORTED, "effnet_create: unsupported architecture '" + a + "' (efficientnet_b0, tf_efficientnet_b0)");
  if (img_size < 32 || img_size > 224 || img_size % 32) return fail(EFFOCR_EFFNET_EINVAL, "effnet_create: img_size must be a multiple of 32 in [32, 224]");
  std::unique_ptr<effocr_effnet> e(new effocr_effnet());
  e->img = img_size; e->prec = precision; e->D = EF_D; e->tf = tf;
  build_effnet(e.get());
  *out = e.release();
  return EFFOCR_EFFNET_OK;
}

EFFNET_API void effocr_effnet_destroy(effocr_effnet_t* enc) { delete enc; }
EFFNET_API int effocr_effnet_embed_dim(const effocr_effnet_t* enc) { return enc ? EF_D : 0; }
EFFNET_API int effocr_effnet_num_params(const effocr_effnet_t* enc) { return enc ? (int)enc->params.size() : 0; }
EFFNET_API const char* effocr_effnet_param_name(const effocr_effnet_t* enc, int i) { return enc_param_name(enc, i); }
EFFNET_API int64_t effocr_effnet_param_numel(const effocr_effnet_t* enc, int i) { return enc_param_numel(enc, i); }

EFFNET_API int effocr_effnet_set_param(effocr_effnet_t* enc, const char* name, const float* host, int64_t numel) {
  return enc_set_param("effnet", enc, name, host, numel);
}

EFFNET_API size_t effocr_effnet_weights_bytes(const effocr_effnet_t* enc) { return enc ? enc->wbytes : 0; }

EFFNET_API int effocr_effnet_upload(effocr_effnet_t* enc, void* weights_dev, size_t bytes) {
  return enc_upload("effnet", enc, weights_dev, bytes, pack_effnet);
}

EFFNET_API size_t effocr_effnet_workspace_bytes(const effocr_effnet_t* enc, int batch) {
  if (!enc || batch <= 0) return 0;
  return effnet_ws(enc, effnet_chunk(enc, batch)).total;
}

EFFNET_API int effocr_effnet_set_chunk(effocr_effnet_t* enc, int crops_per_chunk) {
  if (enc && crops_per_chunk > EF_CHUNK_LIMIT) return fail(EFFOCR_EFFNET_EINVAL, "effnet_set_chunk: at most 65535 crops per sub-batch");
  return enc_set_chunk("effnet", enc, crops_per_chunk);
}

EFFNET_API int effocr_effnet_forward(effocr_effnet_t* enc, const void* x_dev, int x_dtype, int batch, float* emb_dev, int l2_normalize,
                                     void* workspace_dev, size_t workspace_bytes, void* stream) {
  // the crop type is checked before an empty batch returns, behind the two checks that come before it in every family
  if (!enc) return fail(EFFOCR_EFFNET_EINVAL, "effnet_forward: NULL encoder");
  if (batch < 0) return fail(EFFOCR_EFFNET_EINVAL, "effnet_forward: negative batch");
  if (x_dtype < 0 || x_dtype > 2) return fail(EFFOCR_EFFNET_EINVAL, "effnet_forward: unknown crop type");
  if (x_dtype != PREC_FP32) return fail(EFFOCR_EFFNET_EUNSUPPORTED, "effnet_forward: 16-bit crops are not supported (the stem is an fp32 convolution)");
  const int rc = enc_forward_args("effnet", enc, x_dev, batch, emb_dev, workspace_dev, workspace_bytes, effocr_effnet_workspace_bytes(enc, batch));
  if (rc || batch == 0) return rc;
  return enc_forward_chunks(enc, static_cast<const float*>(x_dev), batch, effnet_chunk(enc, batch), emb_dev, [&](const float* x, int crops, float* emb) {
    return effnet_forward(enc, x, crops, emb, l2_normalize, static_cast<char*>(workspace_dev), S(stream));
  });
}

EFFNET_API int effocr_effnet_check_status(const effocr_effnet_t* enc, const void* workspace_dev, void* stream) {   // EfWs::status = offset 0
  return enc_check_status("effnet", enc, workspace_dev, stream, MBCONV_FP16_OVERFLOW);
}

EFFNET_API int effocr_effnet_reset_status(const effocr_effnet_t* enc, void* workspace_dev, void* stream) {
  return enc_reset_status("effnet", enc, workspace_dev, stream);
}

EFFNET_API int effocr_effnet_op_stem(const float* x_dev, int batch, int img_size, int pad_before, const float* w_dev, const float* b_dev,
                                     float* out_dev, void* stream) {
  if (!x_dev || !w_dev || !b_dev || !out_dev) return fail(EFFOCR_EFFNET_EINVAL, "effnet_op_stem: NULL argument");
  if (batch <= 0 || img_size <= 0) return fail(EFFOCR_EFFNET_EINVAL, "effnet_op_stem: bad geometry");
  return ef_stem(x_dev, batch, img_size, pad_before, w_dev, b_dev, out_dev, S(stream));
}

EFFNET_API int effocr_effnet_op_tiles(int out_size) { return out_size > 0 ? ef_tiles(out_size) : 0; }

EFFNET_API int effocr_effnet_op_dw_se(const float* in_dev, int batch, int in_size, int channels, int kernel, int stride, int pad_before,
                                      const float* dw_w_dev, const float* dw_b_dev, int se_width, const float* se_reduce_w_dev,
                                      const float* se_reduce_b_dev, const float* se_expand_wt_dev, const float* se_expand_b_dev,
                                      float* dw_out_dev, float* part_dev, float* gate_dev, void* stream) {
  if (!in_dev || !dw_w_dev || !dw_b_dev || !se_reduce_w_dev || !se_reduce_b_dev || !se_expand_wt_dev || !se_expand_b_dev || !dw_out_dev ||
      !part_dev || !gate_dev)
    return fail(EFFOCR_EFFNET_EINVAL, "effnet_op_dw_se: NULL argument");
  if (batch <= 0 || in_size <= 0 || (stride != 1 && stride != 2)) return fail(EFFOCR_EFFNET_EINVAL, "effnet_op_dw_se: bad geometry");
  const int Ho = out_size(in_size, stride);
  int rc;
  if ((rc = ef_dw(in_dev, batch, in_size, channels, kernel, stride, pad_before, dw_w_dev, dw_b_dev, dw_out_dev, Ho, part_dev, S(stream)))) return rc;
  return ef_se_gate(part_dev, batch, ef_tiles(Ho), Ho * Ho, channels, se_width, se_reduce_w_dev, se_reduce_b_dev, se_expand_wt_dev,
                    se_expand_b_dev, gate_dev, S(stream));
}
