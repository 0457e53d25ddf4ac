// C ABI of libeffocr_bit.so (include/effocr_bit.h): the BiT ResNetV2 encoder handle (parameter table, host-side weight standardisation
// and packing, sub-batched forward orchestration), the library's own error state and the test entry points of bit.hip's operators.  The
// convolutions are the ResNet paths' own, compiled into this library once more with hidden visibility: resnet16.hip's kernel in the 16-bit
// modes, resnet.hip's exact-fp32 pipeline with its split-K turned off in the fp32 mode — both with an all-zero bias vector, no ReLU, and
// the residual on conv3.  All device memory is caller-owned; this file allocates host memory only.
#include "../../include/effocr_bit.h"
#include "resnet_core.hpp"
#include "bit.hpp"

#include <math.h>
#include <memory>

#define BIT_API extern "C" __attribute__((visibility("default")))

namespace effocr {
namespace {

// sub-batches: as many crops as keep the workspace under BIT_WS_BUDGET (1 GB < 1 GiB), at most BIT_MAX_CHUNK
constexpr size_t BIT_WS_BUDGET = (size_t)1000 << 20;
constexpr int BIT_MAX_CHUNK = 256;
constexpr int BIT_WIDTH = 2048;     // the widest layer: length of the shared zero bias

// one weight-standardised convolution: geometry and timm key
struct Conv : ConvGeom { std::string w; };
// one GroupNorm: timm key prefix, channels and blob offsets (gamma, beta [C] fp32)
struct Norm { std::string p; int C; size_t g_off, b_off; };
// one pre-activation bottleneck: convs[c0 ..] = (downsample,) conv1, conv2, conv3; norms[n0 ..] = norm1, norm2, norm3
struct Block { int c0, n0, stride; bool down; };

}  // namespace
}  // namespace effocr

using namespace effocr;

struct effocr_bit : EncoderCore {
  std::vector<Conv> convs;          // the stem, then the blocks' convolutions in state-dict order
  std::vector<Norm> norms;          // the blocks' norms, then the final norm
  std::vector<Block> blocks;
  size_t zero_off = 0;              // BIT_WIDTH fp32 zeros: the bias of every convolution
  int gn_tiles = 0;                 // most GroupNorm tiles a crop has in any layer
};

namespace effocr {
namespace {

void add_conv(effocr_bit* e, const std::string& w, int cin, int cout, int k, int stride, int pad) {
  e->add_param(w, (int64_t)cout * cin * k * k);
  e->convs.push_back(Conv{{cin, cout, k, stride, pad, k * k * cin, 0}, w});
}
void add_norm(effocr_bit* e, const std::string& p, int C, int HW) {
  e->add_param(p + ".weight", C); e->add_param(p + ".bias", C);
  e->norms.push_back(Norm{p, C, 0, 0});
  e->gn_tiles = std::max(e->gn_tiles, bit_gn_tiles(HW, C));
}

// timm resnetv2 (PreActBottleneck, width factor 1): mid widths 64-128-256-512, x4 out, the stride on conv2 and on the shortcut of a
// stage's first block, GroupNorm(32, eps 1e-5) + ReLU before every convolution, a final norm.
void build_bit(effocr_bit* e, int depth2) {
  const int depths[4] = {3, 4, depth2, 3}, widths[4] = {64, 128, 256, 512};
  add_conv(e, "stem.conv.weight", 3, 64, 7, 2, 3);
  e->convs[0].kpad = e->prec == PREC_FP32 ? RES_STEM_K32 : RN_STEM_K16;
  int cin = 64, H = e->img / 4;
  for (int si = 0; si < 4; ++si) {
    const int mid = widths[si], cout = 4 * mid;
    for (int bi = 0; bi < depths[si]; ++bi) {
      const std::string p = "stages." + std::to_string(si) + ".blocks." + std::to_string(bi) + ".";
      const int stride = (bi == 0 && si > 0) ? 2 : 1, Ho = (H - 1) / stride + 1;
      Block b{(int)e->convs.size(), (int)e->norms.size(), stride, bi == 0};
      if (b.down) add_conv(e, p + "downsample.conv.weight", cin, cout, 1, stride, 0);
      add_norm(e, p + "norm1", cin, H * H);
      add_conv(e, p + "conv1.weight", cin, mid, 1, 1, 0);
      add_norm(e, p + "norm2", mid, H * H);
      add_conv(e, p + "conv2.weight", mid, mid, 3, stride, 1);
      add_norm(e, p + "norm3", mid, Ho * Ho);
      add_conv(e, p + "conv3.weight", mid, cout, 1, 1, 0);
      e->blocks.push_back(b);
      cin = cout; H = Ho;
    }
  }
  add_norm(e, "norm", cin, H * H);
  e->D = cin;
  const size_t es = prec_esize(e->prec);
  Alloc a;
  e->zero_off = a.take((size_t)BIT_WIDTH * 4);
  for (Conv& c : e->convs) c.w_off = a.take((size_t)c.cout * c.kpad * es);
  for (Norm& n : e->norms) { n.g_off = a.take((size_t)n.C * 4); n.b_off = a.take((size_t)n.C * 4); }
  e->wbytes = a.off;
}

// Weight standardisation (timm StdConv2d, eps 1e-8) in double, per output channel over its Cin x KH x KW values: w' = (w - mean) /
// sqrt(biased var + eps); the weight re-laid-out from torch [Cout,Cin,KH,KW] to [Cout][KH][KW][Cin] (Cin fastest), zero-padded to kpad
// columns, then rounded once to the operand type.  The zero bias stays as the zeroed blob has it.
void pack_bit(const effocr_bit* e, std::vector<char>& blob) {
  for (const Conv& c : e->convs) {
    const auto& w = e->P(c.w);
    const size_t fan = (size_t)c.cin * c.k * c.k;
    std::vector<double> mean(c.cout), sc(c.cout);
    for (int co = 0; co < c.cout; ++co) {
      const float* wc = w.data() + (size_t)co * fan;
      double m = 0.0, var = 0.0;
      for (size_t i = 0; i < fan; ++i) m += (double)wc[i];
      m /= (double)fan;
      for (size_t i = 0; i < fan; ++i) { const double d = (double)wc[i] - m; var += d * d; }
      mean[co] = m; sc[co] = 1.0 / sqrt(var / (double)fan + 1e-8);
    }
    const std::vector<float> wd = relayout_ohwi(w, c, mean, sc);
    put_op(blob, c.w_off, wd.data(), wd.size(), e->prec);
  }
  for (const Norm& n : e->norms) {
    put_f32(blob, n.g_off, e->P(n.p + ".weight").data(), n.C);
    put_f32(blob, n.b_off, e->P(n.p + ".bias").data(), n.C);
  }
}

// workspace of one sub-batch of B crops: resnet_core.hpp's four buffers, with the GroupNorm tile statistics as the block of its own
ResWs bit_ws(const effocr_bit* e, int B) {
  return res_ws(B, e->img, e->convs[0].kpad, prec_esize(e->prec), (size_t)B * e->gn_tiles * BIT_GROUPS * BIT_GN_REC * sizeof(float));
}

int bit_chunk(const effocr_bit* e, int batch) {
  return enc_default_chunk(e, batch, BIT_WS_BUDGET, BIT_MAX_CHUNK, [e](int B) { return bit_ws(e, B).total; });
}

const float* zero_bias(const effocr_bit* e) { return reinterpret_cast<const float*>(e->wdev + e->zero_off); }

// one weight-standardised convolution, no bias (the shared zeros), no ReLU, + residual
int conv(const effocr_bit* e, const Conv& c, const void* in, int B, int H, int W, int OH, int OW, const void* resid, void* out, hipStream_t s) {
  return launch_conv(e->prec, e->wdev, c, zero_bias(e), in, B, H, W, OH, OW, resid, 0, out, s);
}

int gn(const effocr_bit* e, const Norm& n, const void* in, void* out, int B, int HW, float* partial, hipStream_t s) {
  const char* wb = e->wdev;
  return bit_groupnorm_relu(e->prec, in, out, B, HW, n.C, reinterpret_cast<const float*>(wb + n.g_off), reinterpret_cast<const float*>(wb + n.b_off),
                            partial, s);
}

// One sub-batch: stem (im2col + 1x1 GEMM, nothing after it) -> zero pad + max pool -> the pre-activation bottlenecks -> head.
// A block with input x in buf[cur]: p = gn1(x) -> t0; shortcut = downsample(p) -> t2 (first block of a stage) or x; conv1(p) -> t1, gn2 in
// place; conv2 -> t0, gn3 in place; conv3 + shortcut -> t1, the next block's input.
int bit_forward(const effocr_bit* e, const float* x, int B, float* emb, int l2, char* ws, hipStream_t s) {
  const ResWs w = bit_ws(e, B);
  void* buf[4];
  for (int i = 0; i < 4; ++i) buf[i] = ws + w.buf[i];
  int* status = reinterpret_cast<int*>(ws + w.status);
  float* part = reinterpret_cast<float*>(ws + w.extra);
  int rc;
  if ((rc = stem_as_1x1(e->prec, e->wdev, e->convs[0], zero_bias(e), x, buf[1], B, e->img, 0, buf[0], s))) return rc;
  int H = e->img / 2, OH = (H - 1) / 2 + 1;
  if ((rc = bit_stem_pool(e->prec, buf[0], buf[1], B, H, H, 64, OH, OH, s))) return rc;
  H = OH;
  int cur = 1;                                          // buf[cur] holds the block input
  for (const Block& b : e->blocks) {
    int t[3];
    free_bufs(cur, t);
    const int Ho = (H - 1) / b.stride + 1;
    const Conv* cv = e->convs.data() + b.c0 + (b.down ? 1 : 0);
    const Norm* nm = e->norms.data() + b.n0;
    if ((rc = gn(e, nm[0], buf[cur], buf[t[0]], B, H * H, part, s))) return rc;
    const void* idt = buf[cur];
    if (b.down) {
      if ((rc = conv(e, e->convs[b.c0], buf[t[0]], B, H, H, Ho, Ho, nullptr, buf[t[2]], s))) return rc;
      idt = buf[t[2]];
    }
    if ((rc = conv(e, cv[0], buf[t[0]], B, H, H, H, H, nullptr, buf[t[1]], s))) return rc;
    if ((rc = gn(e, nm[1], buf[t[1]], buf[t[1]], B, H * H, part, s))) return rc;
    if ((rc = conv(e, cv[1], buf[t[1]], B, H, H, Ho, Ho, nullptr, buf[t[0]], s))) return rc;
    if ((rc = gn(e, nm[2], buf[t[0]], buf[t[0]], B, Ho * Ho, part, s))) return rc;
    if ((rc = conv(e, cv[2], buf[t[0]], B, Ho, Ho, Ho, Ho, idt, buf[t[1]], s))) return rc;
    cur = t[1];
    H = Ho;
  }
  const Norm& fin = e->norms.back();
  return bit_head(e->prec, buf[cur], emb, B, H * H, e->D, reinterpret_cast<const float*>(e->wdev + fin.g_off),
                  reinterpret_cast<const float*>(e->wdev + fin.b_off), l2, status, s);
}

}  // namespace
}  // namespace effocr

BIT_API int effocr_bit_abi_version(void) { return EFFOCR_BIT_ABI_VERSION; }
BIT_API const char* effocr_bit_last_error(void) { return g_err.c_str(); }

BIT_API int effocr_bit_create(const char* arch, int img_size, int precision, effocr_bit_t** out) {
  if (!arch || !out) return fail(EFFOCR_BIT_EINVAL, "bit_create: NULL argument");
  if (precision < 0 || precision > 2) return fail(EFFOCR_BIT_EINVAL, "bit_create: unknown precision");
  const std::string a = arch;
  int depth2;
  if (a == "resnetv2_50x1_bitm" || a == "resnetv2_50x1_bit") depth2 = 6;
  else if (a == "resnetv2_101x1_bitm" || a == "resnetv2_101x1_bit") depth2 = 23;
  else return fail(EFFOCR_BIT_EUNSUPPORTED, "bit_create: unsupported architecture '" + a + "' (resnetv2_50x1_bitm, resnetv2_101x1_bitm)");
  if (img_size < 32 || img_size % 32) return fail(EFFOCR_BIT_EINVAL, "bit_create: img_size must be a positive multiple of 32");
  std::unique_ptr<effocr_bit> e(new effocr_bit());
  e->img = img_size; e->prec = precision;
  build_bit(e.get(), depth2);
  *out = e.release();
  return EFFOCR_BIT_OK;
}

BIT_API void effocr_bit_destroy(effocr_bit_t* enc) { delete enc; }
BIT_API int effocr_bit_embed_dim(const effocr_bit_t* enc) { return enc ? enc->D : 0; }
BIT_API int effocr_bit_num_params(const effocr_bit_t* enc) { return enc ? (int)enc->params.size() : 0; }
BIT_API const char* effocr_bit_param_name(const effocr_bit_t* enc, int i) { return enc_param_name(enc, i); }
BIT_API int64_t effocr_bit_param_numel(const effocr_bit_t* enc, int i) { return enc_param_numel(enc, i); }

BIT_API int effocr_bit_set_param(effocr_bit_t* enc, const char* name, const float* host, int64_t numel) {
  return enc_set_param("bit", enc, name, host, numel);
}

BIT_API size_t effocr_bit_weights_bytes(const effocr_bit_t* enc) { return enc ? enc->wbytes : 0; }

BIT_API int effocr_bit_upload(effocr_bit_t* enc, void* weights_dev, size_t bytes) { return enc_upload("bit", enc, weights_dev, bytes, pack_bit); }

BIT_API size_t effocr_bit_workspace_bytes(const effocr_bit_t* enc, int batch) {
  if (!enc || batch <= 0) return 0;
  return bit_ws(enc, bit_chunk(enc, batch)).total;
}

BIT_API int effocr_bit_set_chunk(effocr_bit_t* enc, int crops_per_chunk) { return enc_set_chunk("bit", enc, crops_per_chunk); }

BIT_API int effocr_bit_forward(effocr_bit_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize, void* workspace_dev,
                               size_t workspace_bytes, void* stream) {
  const int rc = enc_forward_args("bit", enc, x_dev, batch, emb_dev, workspace_dev, workspace_bytes, effocr_bit_workspace_bytes(enc, batch));
  if (rc || batch == 0) return rc;
  const int chunk = bit_chunk(enc, batch);
  if (!res_index_ok(chunk, enc->img, enc->convs[0].kpad) || chunk > 65535)
    return fail(EFFOCR_BIT_EUNSUPPORTED, "bit_forward: chunk too large for 32-bit activation indices (effocr_bit_set_chunk)");
  return enc_forward_chunks(enc, x_dev, batch, chunk, emb_dev, [&](const float* x, int crops, float* emb) {
    return bit_forward(enc, x, crops, emb, l2_normalize, static_cast<char*>(workspace_dev), S(stream));
  });
}

BIT_API int effocr_bit_check_status(const effocr_bit_t* enc, const void* workspace_dev, void* stream) {   // BitWs::status = offset 0
  return enc_check_status("bit", enc, workspace_dev, stream,
                          "forward: non-finite embedding — an f16 activation overflowed (beyond 65504) or the input or the weights were "
                          "not finite; use precision bf16 or fp32 for this checkpoint");
}

BIT_API int effocr_bit_reset_status(const effocr_bit_t* enc, void* workspace_dev, void* stream) {
  return enc_reset_status("bit", enc, workspace_dev, stream);
}

// ---------------------------------------------------------------- test entry points (one operator per call)
BIT_API int effocr_bit_op_groupnorm_relu(int dtype, const void* x_dev, int batch, int hw, int channels, const float* gamma_dev,
                                         const float* beta_dev, void* out_dev, void* scratch_dev, size_t scratch_bytes, void* stream) {
  if (!x_dev || !gamma_dev || !beta_dev || !out_dev || !scratch_dev) return fail(EFFOCR_BIT_EINVAL, "bit_op_groupnorm_relu: NULL argument");
  if (dtype < 0 || dtype > 2) return fail(EFFOCR_BIT_EINVAL, "bit_op_groupnorm_relu: unknown dtype");
  if (batch <= 0 || hw <= 0 || channels <= 0) return fail(EFFOCR_BIT_EINVAL, "bit_op_groupnorm_relu: bad geometry");
  if (channels < 64 || channels > 2048 || (channels & (channels - 1)))
    return fail(EFFOCR_BIT_EUNSUPPORTED, "bit_op_groupnorm_relu: channels must be a power of two from 64 to 2048");
  if (scratch_bytes < bit_gn_scratch_bytes(batch, hw, channels)) return fail(EFFOCR_BIT_EWORKSPACE, "bit_op_groupnorm_relu: scratch too small");
  return bit_groupnorm_relu(dtype, x_dev, out_dev, batch, hw, channels, gamma_dev, beta_dev, static_cast<float*>(scratch_dev), S(stream));
}

BIT_API int effocr_bit_op_stem_pool(int dtype, const void* x_dev, int batch, int h, int w, int channels, void* out_dev, void* stream) {
  if (!x_dev || !out_dev) return fail(EFFOCR_BIT_EINVAL, "bit_op_stem_pool: NULL argument");
  if (dtype < 0 || dtype > 2) return fail(EFFOCR_BIT_EINVAL, "bit_op_stem_pool: unknown dtype");
  if (batch <= 0 || h <= 0 || w <= 0 || channels <= 0) return fail(EFFOCR_BIT_EINVAL, "bit_op_stem_pool: bad geometry");
  return bit_stem_pool(dtype, x_dev, out_dev, batch, h, w, channels, (h - 1) / 2 + 1, (w - 1) / 2 + 1, S(stream));
}

BIT_API int effocr_bit_op_head(int dtype, const void* x_dev, int batch, int hw, int channels, const float* gamma_dev, const float* beta_dev,
                               int l2_normalize, float* emb_dev, int* status_dev, void* stream) {
  if (!x_dev || !gamma_dev || !beta_dev || !emb_dev) return fail(EFFOCR_BIT_EINVAL, "bit_op_head: NULL argument");
  if (dtype < 0 || dtype > 2) return fail(EFFOCR_BIT_EINVAL, "bit_op_head: unknown dtype");
  if (batch <= 0 || hw <= 0 || channels <= 0) return fail(EFFOCR_BIT_EINVAL, "bit_op_head: bad geometry");
  return bit_head(dtype, x_dev, emb_dev, batch, hw, channels, gamma_dev, beta_dev, l2_normalize, status_dev, S(stream));
}
