// C ABI of libeffocr_resnet.so (include/effocr_resnet.h): the ResNet-34 / ResNet-50 encoder handle (parameter table, host-side BN folding
// and packing, sub-batched forward orchestration) and the library's own error state.  The 16-bit modes run resnet16.hip's kernels; the
// fp32 mode runs the exact-fp32 convolution pipeline of resnet.hip, which this library compiles a second time with hidden visibility, with
// its split-K turned off.  All device memory is caller-owned; this file allocates host memory only.
#include "../../include/effocr_resnet.h"
#include "resnet_core.hpp"

#include <math.h>
#include <memory>

#define RESNET_API extern "C" __attribute__((visibility("default")))

namespace effocr {
namespace {

// sub-batches: as many crops as keep the workspace under RN_WS_BUDGET (1 GB < 1 GiB), at most RN_MAX_CHUNK
constexpr size_t RN_WS_BUDGET = (size_t)1000 << 20;
constexpr int RN_MAX_CHUNK = 256;

// one convolution + its BatchNorm: geometry, timm key prefixes and the blob offset of the bias [cout] fp32
struct Conv : ConvGeom { std::string w, bn; size_t b_off; };
// one residual block: convs[c0 ..] = conv1, conv2 (, conv3) (, downsample)
struct Block { int c0, nconv, stride; bool down; };

}  // namespace
}  // namespace effocr

using namespace effocr;

struct effocr_resnet : EncoderCore {
  bool bottleneck = false;
  std::vector<Conv> convs;          // conv1 (stem), then the blocks' convolutions in forward order
  std::vector<Block> blocks;
};

namespace effocr {
namespace {

void add_conv(effocr_resnet* e, const std::string& w, const std::string& bn, int cin, int cout, int k, int stride, int pad) {
  e->add_param(w, (int64_t)cout * cin * k * k);
  e->add_bn(bn, cout);
  e->convs.push_back(Conv{{cin, cout, k, stride, pad, k * k * cin, 0}, w, bn, 0});
}

// timm resnet34 (BasicBlock) / resnet50 (Bottleneck): depths 3-4-6-3, widths 64-128-256-512 (x4 expansion for the bottleneck),
// 7x7/2 stem + 3x3/2 max pool, the stride on the 3x3 conv (the bottleneck's conv2), a 1x1 stride-s conv + BN shortcut, BN eps 1e-5.
void build_resnet(effocr_resnet* e) {
  static const int depths[4] = {3, 4, 6, 3}, widths[4] = {64, 128, 256, 512};
  const int exp = e->bottleneck ? 4 : 1;
  add_conv(e, "conv1.weight", "bn1", 3, 64, 7, 2, 3);
  e->convs[0].kpad = e->prec == PREC_FP32 ? RES_STEM_K32 : RN_STEM_K16;
  int cin = 64;
  for (int li = 0; li < 4; ++li) {
    const int w = widths[li], cout = w * exp;
    for (int bi = 0; bi < depths[li]; ++bi) {
      const std::string p = "layer" + std::to_string(li + 1) + "." + std::to_string(bi) + ".";
      const int stride = (bi == 0 && li > 0) ? 2 : 1;
      Block b{(int)e->convs.size(), 0, stride, bi == 0 && (stride != 1 || cin != cout)};
      if (e->bottleneck) {
        add_conv(e, p + "conv1.weight", p + "bn1", cin, w, 1, 1, 0);
        add_conv(e, p + "conv2.weight", p + "bn2", w, w, 3, stride, 1);
        add_conv(e, p + "conv3.weight", p + "bn3", w, cout, 1, 1, 0);
      } else {
        add_conv(e, p + "conv1.weight", p + "bn1", cin, w, 3, stride, 1);
        add_conv(e, p + "conv2.weight", p + "bn2", w, w, 3, 1, 1);
      }
      if (b.down) add_conv(e, p + "downsample.0.weight", p + "downsample.1", cin, cout, 1, stride, 0);
      b.nconv = (int)e->convs.size() - b.c0;
      e->blocks.push_back(b);
      cin = cout;
    }
  }
  e->D = cin;
  const size_t es = prec_esize(e->prec);
  Alloc a;
  for (Conv& c : e->convs) {
    c.w_off = a.take((size_t)c.cout * c.kpad * es);
    c.b_off = a.take((size_t)c.cout * 4);
  }
  e->wbytes = a.off;
}

// BatchNorm (eval, eps 1e-5) folded into the conv in double: w' = w * g/sqrt(v+eps), b' = beta - mean*g/sqrt(v+eps); the weight re-laid-out
// from torch [Cout,Cin,KH,KW] to [Cout][KH][KW][Cin] (Cin fastest), zero-padded to kpad columns, then rounded once to the operand type.
void pack_resnet(const effocr_resnet* e, std::vector<char>& blob) {
  for (const Conv& c : e->convs) {
    const auto& w = e->P(c.w);
    const auto& g = e->P(c.bn + ".weight"); const auto& bt = e->P(c.bn + ".bias");
    const auto& mu = e->P(c.bn + ".running_mean"); const auto& var = e->P(c.bn + ".running_var");
    std::vector<double> sc(c.cout);
    float* bd = reinterpret_cast<float*>(blob.data() + c.b_off);
    for (int co = 0; co < c.cout; ++co) {
      sc[co] = (double)g[co] / sqrt((double)var[co] + 1e-5);
      bd[co] = (float)((double)bt[co] - (double)mu[co] * sc[co]);
    }
    const std::vector<float> wd = relayout_ohwi(w, c, std::vector<double>(c.cout, 0.0), sc);   // w - 0.0 is exact
    put_op(blob, c.w_off, wd.data(), wd.size(), e->prec);
  }
}

// workspace of one sub-batch of B crops: resnet_core.hpp's four buffers, nothing of its own
ResWs resnet_ws(const effocr_resnet* e, int B) { return res_ws(B, e->img, e->convs[0].kpad, prec_esize(e->prec), 0); }

int resnet_chunk(const effocr_resnet* e, int batch) {
  return enc_default_chunk(e, batch, RN_WS_BUDGET, RN_MAX_CHUNK, [e](int B) { return resnet_ws(e, B).total; });
}

const float* bias_of(const effocr_resnet* e, const Conv& c) { return reinterpret_cast<const float*>(e->wdev + c.b_off); }

// one convolution (+ folded BN) with the epilogue: + residual, ReLU
int conv(const effocr_resnet* e, const Conv& c, const void* in, int B, int H, int W, int OH, int OW, const void* resid, int relu, void* out,
         hipStream_t s) {
  return launch_conv(e->prec, e->wdev, c, bias_of(e, c), in, B, H, W, OH, OW, resid, relu, out, s);
}

// One sub-batch: stem (im2col + 1x1 GEMM, bn1, ReLU) -> max pool -> 16 residual blocks -> global average pool (+ F.normalize).
int resnet_forward(const effocr_resnet* e, const float* x, int B, float* emb, int l2, char* ws, hipStream_t s) {
  const ResWs w = resnet_ws(e, B);
  const bool f32 = e->prec == PREC_FP32;
  void* buf[4];
  for (int i = 0; i < 4; ++i) buf[i] = ws + w.buf[i];
  int* status = reinterpret_cast<int*>(ws + w.status);
  int rc;
  if ((rc = stem_as_1x1(e->prec, e->wdev, e->convs[0], bias_of(e, e->convs[0]), x, buf[1], B, e->img, 1, buf[0], s))) return rc;
  int H = e->img / 2, OH = (H - 1) / 2 + 1;
  if ((rc = f32 ? maxpool3x3s2_nhwc(static_cast<float*>(buf[0]), static_cast<float*>(buf[1]), B, H, H, 64, OH, OH, s)
                : rn_maxpool16(e->prec, buf[0], buf[1], B, H, H, 64, OH, OH, s))) return rc;
  H = OH;
  int cur = 1;                                          // buf[cur] holds the block input
  for (const Block& b : e->blocks) {
    int t[3];
    free_bufs(cur, t);
    const int Ho = (H - 1) / b.stride + 1;
    const Conv* cv = e->convs.data() + b.c0;
    const void* idt = buf[cur];
    if (b.down) {                                       // shortcut: 1x1 stride-s conv + BN into t[2]
      if ((rc = conv(e, cv[b.nconv - 1], buf[cur], B, H, H, Ho, Ho, nullptr, 0, buf[t[2]], s))) return rc;
      idt = buf[t[2]];
    }
    int out;
    if (e->bottleneck) {                                // 1x1 -> t0, 3x3/s -> t1, 1x1 + identity -> t0
      if ((rc = conv(e, cv[0], buf[cur], B, H, H, H, H, nullptr, 1, buf[t[0]], s))) return rc;
      if ((rc = conv(e, cv[1], buf[t[0]], B, H, H, Ho, Ho, nullptr, 1, buf[t[1]], s))) return rc;
      if ((rc = conv(e, cv[2], buf[t[1]], B, Ho, Ho, Ho, Ho, idt, 1, buf[t[0]], s))) return rc;
      out = t[0];
    } else {                                            // 3x3/s -> t0, 3x3 + identity -> t1
      if ((rc = conv(e, cv[0], buf[cur], B, H, H, Ho, Ho, nullptr, 1, buf[t[0]], s))) return rc;
      if ((rc = conv(e, cv[1], buf[t[0]], B, Ho, Ho, Ho, Ho, idt, 1, buf[t[1]], s))) return rc;
      out = t[1];
    }
    cur = out;
    H = Ho;
  }
  return rn_avgpool(e->prec, buf[cur], emb, B, H * H, e->D, l2, status, s);
}

}  // namespace
}  // namespace effocr

RESNET_API int effocr_resnet_abi_version(void) { return EFFOCR_RESNET_ABI_VERSION; }
RESNET_API const char* effocr_resnet_last_error(void) { return g_err.c_str(); }

RESNET_API int effocr_resnet_create(const char* arch, int img_size, int precision, effocr_resnet_t** out) {
  if (!arch || !out) return fail(EFFOCR_RESNET_EINVAL, "resnet_create: NULL argument");
  if (precision < 0 || precision > 2) return fail(EFFOCR_RESNET_EINVAL, "resnet_create: unknown precision");
  const std::string a = arch;
  if (a != "resnet34" && a != "resnet50")
    return fail(EFFOCR_RESNET_EUNSUPPORTED, "resnet_create: unsupported architecture '" + a + "' (resnet34, resnet50)");
  if (img_size < 32 || img_size % 32) return fail(EFFOCR_RESNET_EINVAL, "resnet_create: img_size must be a positive multiple of 32");
  std::unique_ptr<effocr_resnet> e(new effocr_resnet());
  e->img = img_size; e->prec = precision; e->bottleneck = a == "resnet50";
  build_resnet(e.get());
  *out = e.release();
  return EFFOCR_RESNET_OK;
}

RESNET_API void effocr_resnet_destroy(effocr_resnet_t* enc) { delete enc; }
RESNET_API int effocr_resnet_embed_dim(const effocr_resnet_t* enc) { return enc ? enc->D : 0; }
RESNET_API int effocr_resnet_num_params(const effocr_resnet_t* enc) { return enc ? (int)enc->params.size() : 0; }
RESNET_API const char* effocr_resnet_param_name(const effocr_resnet_t* enc, int i) { return enc_param_name(enc, i); }
RESNET_API int64_t effocr_resnet_param_numel(const effocr_resnet_t* enc, int i) { return enc_param_numel(enc, i); }

RESNET_API int effocr_resnet_set_param(effocr_resnet_t* enc, const char* name, const float* host, int64_t numel) {
  return enc_set_param("resnet", enc, name, host, numel);
}

RESNET_API size_t effocr_resnet_weights_bytes(const effocr_resnet_t* enc) { return enc ? enc->wbytes : 0; }

RESNET_API int effocr_resnet_upload(effocr_resnet_t* enc, void* weights_dev, size_t bytes) {
  return enc_upload("resnet", enc, weights_dev, bytes, pack_resnet);
}

RESNET_API size_t effocr_resnet_workspace_bytes(const effocr_resnet_t* enc, int batch) {
  if (!enc || batch <= 0) return 0;
  return resnet_ws(enc, resnet_chunk(enc, batch)).total;
}

RESNET_API int effocr_resnet_set_chunk(effocr_resnet_t* enc, int crops_per_chunk) { return enc_set_chunk("resnet", enc, crops_per_chunk); }

RESNET_API int effocr_resnet_forward(effocr_resnet_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize,
                                     void* workspace_dev, size_t workspace_bytes, void* stream) {
  const int rc = enc_forward_args("resnet", enc, x_dev, batch, emb_dev, workspace_dev, workspace_bytes, effocr_resnet_workspace_bytes(enc, batch));
  if (rc || batch == 0) return rc;
  const int chunk = resnet_chunk(enc, batch);
  if (!res_index_ok(chunk, enc->img, enc->convs[0].kpad))
    return fail(EFFOCR_RESNET_EUNSUPPORTED, "resnet_forward: chunk too large for 32-bit activation indices (effocr_resnet_set_chunk)");
  return enc_forward_chunks(enc, x_dev, batch, chunk, emb_dev, [&](const float* x, int crops, float* emb) {
    return resnet_forward(enc, x, crops, emb, l2_normalize, static_cast<char*>(workspace_dev), S(stream));
  });
}

RESNET_API int effocr_resnet_check_status(const effocr_resnet_t* enc, const void* workspace_dev, void* stream) {   // RnWs::status = offset 0
  return enc_check_status("resnet", enc, workspace_dev, stream, ENC_F16_ACTIVATION_OVERFLOW);
}
