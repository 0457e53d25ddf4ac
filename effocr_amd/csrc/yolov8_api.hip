// C ABI of libeffocr_yolov8.so (include/effocr_yolov8.h): the ultralytics YOLOv8 detection networks n / s / m / l / x as localizers.
// No ultralytics install was at hand: the builder follows yolov8.yaml, nn/modules and parse_model as published, checked by the five
// published parameter counts (tests/test_yolov8_host.py) — UNVERIFIED against a real checkpoint (DESIGN.md section 3 "YOLOv8").
//   Conv        = Conv2d(bias=False) + BatchNorm2d(eps 1e-3) + SiLU        -> BN folded on the host, SiLU in the epilogue
//   Bottleneck  = x + cv2(cv1(x)) (shortcut) | cv2(cv1(x))                  both convolutions 3x3, e = 1.0 inside C2f
//   C2f         = cv2(cat(y0, y1, m0(y1), m1(m0(y1)), ...))  [y0 | y1] = cv1(x)   -> ONE buffer of 2 + n slices, cv1 writes two of them
//   SPPF        = YOLOv5's
//   Detect      = per level: box branch Conv3x3, Conv3x3, 1x1 (bias) -> 4 x 16 logits; class branch Conv3x3, Conv3x3, 1x1 (bias) -> nc
//                 logits; decode (yolov8.hip) -> rows (cx, cy, w, h, 1, scores): the YOLOv5 row layout, so the product library's NMS applies
// The machinery (parameter table, buffers, channel-slice views, ops, BN folding, weight packing, zero-padded storage of widths that are
// no multiple of 32, the op loop) is localizer_core.hpp's, shared with the YOLOv5 engine; the convolutions are resnet.hip's implicit GEMM
// and the upsample / pool / im2col kernels yolo.hip's, both compiled into this library a second time with hidden visibility.
#include "../../include/effocr_yolov8.h"
#include "enc_core.hpp"
#include "localizer_core.hpp"

#define YOLOV8_API extern "C" __attribute__((visibility("default")))

using namespace effocr;

struct effocr_yolov8 : LocNet {};

namespace effocr {
namespace {

int pad_of(int c) { return pad32(c) == c ? 0 : pad32(c); }   // View::S of a tensor of c channels

struct V8Builder : Builder {
  // C2f(c1 -> c2, n bottlenecks, shortcut): one concat buffer of 2 + n slices of c = c2 / 2 channels.  cv1 (ONE Conv block of 2c output
  // channels) writes slices 0 and 1 in one launch; bottleneck i reads slice 1 + i and its second convolution writes slice 2 + i, its
  // residual read from slice 1 + i; cv2 reads the whole buffer.  A c that is not a multiple of 32 (model.2 of n / m / x) is stored as
  // cp = c padded to 32 in every slice: cv1's weight rows and cv2's weight columns skip every pad (LConv::ocut / icut).
  void c2f(const std::string& name, View in, View out, int n, bool shortcut) {
    const int c = out.C / 2, cp = pad32(c), H = e->bufs[in.buf].H, W = e->bufs[in.buf].W;
    const int cat = new_buf(H, W, (2 + n) * cp);
    auto slice = [&](int i) { return View{cat, i * cp, c, pad_of(c)}; };
    conv(name + ".cv1", in, View{cat, 0, 2 * c, cp == c ? 0 : 2 * cp}, 1, 1);
    e->convs.back().ocut = c; e->convs.back().oshift = cp - c;
    const View t = {new_buf(H, W, cp), 0, c, pad_of(c)};   // the bottlenecks run one after the other: one temporary serves them all
    for (int i = 0; i < n; ++i) {
      const std::string m = name + ".m." + std::to_string(i);
      conv(m + ".cv1", slice(1 + i), t, 3, 1);
      conv(m + ".cv2", t, slice(2 + i), 3, 1, 1, shortcut ? slice(1 + i) : View{-1, 0, 0});
    }
    conv(name + ".cv2", View{cat, 0, (2 + n) * c, cp == c ? 0 : (2 + n) * cp}, out, 1, 1);
    e->convs.back().icut = c; e->convs.back().ishift = cp - c;
  }
};

struct Scale { const char* name; double depth, width; int max_channels; };
const Scale SCALES[5] = {{"yolov8n", 0.33, 0.25, 1024}, {"yolov8s", 0.33, 0.50, 1024}, {"yolov8m", 0.67, 0.75, 768}, {"yolov8l", 1.00, 1.00, 512},
                         {"yolov8x", 1.00, 1.25, 512}};

// parse_model over the yolov8.yaml rows at (depth, width, max_channels): channels ceil(min(c, max_channels) * width / 8) * 8, repeats
// max(round(n * depth), 1) for n > 1.  The neck concatenations are slices of one buffer each, written by their producers.
int build_yolov8(effocr_yolov8* e, const Scale& sc) {
  V8Builder b{{e}};
  auto ch = [&](int c) { return (int)ceil(std::min(c, sc.max_channels) * sc.width / 8) * 8; };
  auto rp = [&](int n) { return n > 1 ? std::max((int)lround(n * sc.depth), 1) : n; };
  const int c64 = ch(64), c128 = ch(128), c256 = ch(256), c512 = ch(512), c1024 = ch(1024);
  // the concat slices, the SPPF slices and the pooled / upsampled tensors are addressed unpadded
  if (c128 % 32 || c256 % 32 || c512 % 32 || c1024 % 64) return fail(EFFOCR_EUNSUPPORTED, "yolov8_create: a scale whose layer widths are no multiples of 32");
  const int H = e->in_h, W = e->in_w;
  const int H1 = down(H), W1 = down(W), H2 = down(H1), W2 = down(W1), H3 = down(H2), W3 = down(W2), H4 = down(H3), W4 = down(W3),
            H5 = down(H4), W5 = down(W4);
  // 0: Conv(3, c64, 3, 2) — stem: stem3x3s2_nchw, or (direct_stem = 0) im2col rows [.., 32] (27 taps + zeros) then a 1x1 implicit GEMM
  const View v0 = {b.new_buf(H1, W1, pad32(c64)), 0, c64, pad_of(c64)};
  b.stem("model.0", v0, 3, 1, 32, H1, W1);
  const int l1 = b.new_buf(H2, W2, c128);  b.conv("model.1", v0, b.whole(l1), 3, 2);
  const int l2 = b.new_buf(H2, W2, c128);  b.c2f("model.2", b.whole(l1), b.whole(l2), rp(3), true);
  const int l3 = b.new_buf(H3, W3, c256);  b.conv("model.3", b.whole(l2), b.whole(l3), 3, 2);
  const int cat14 = b.new_buf(H3, W3, c512 + c256);         // [up(l12) | l4]
  const View l4 = {cat14, c512, c256};
  b.c2f("model.4", b.whole(l3), l4, rp(6), true);
  const int l5 = b.new_buf(H4, W4, c512);  b.conv("model.5", l4, b.whole(l5), 3, 2);
  const int cat11 = b.new_buf(H4, W4, c1024 + c512);        // [up(l9) | l6]
  const View l6 = {cat11, c1024, c512};
  b.c2f("model.6", b.whole(l5), l6, rp(6), true);
  const int l7 = b.new_buf(H5, W5, c1024); b.conv("model.7", l6, b.whole(l7), 3, 2);
  const int l8 = b.new_buf(H5, W5, c1024); b.c2f("model.8", b.whole(l7), b.whole(l8), rp(3), true);
  // 9: SPPF(c1024, c1024, 5), its output straight into the last concat
  const int cs = c1024 / 2;
  const int spp = b.new_buf(H5, W5, 4 * cs);
  b.conv("model.9.cv1", b.whole(l8), {spp, 0, cs}, 1, 1);
  for (int i = 0; i < 3; ++i) e->ops.push_back({OP_POOL, {spp, cs * i, cs}, {spp, cs * (i + 1), cs}, {-1, 0, 0}, -1, 0});
  const int cat20 = b.new_buf(H5, W5, c512 + c1024);        // [l19 | l9]
  const View l9 = {cat20, c512, c1024};
  b.conv("model.9.cv2", b.whole(spp), l9, 1, 1);
  // head
  e->ops.push_back({OP_UP, l9, {cat11, 0, c1024}, {-1, 0, 0}, -1, 0});                                // 10, 11
  const int cat17 = b.new_buf(H4, W4, c256 + c512);         // [l16 | l12]
  const View l12 = {cat17, c256, c512};
  b.c2f("model.12", b.whole(cat11), l12, rp(3), false);
  e->ops.push_back({OP_UP, l12, {cat14, 0, c512}, {-1, 0, 0}, -1, 0});                                // 13, 14
  const int l15 = b.new_buf(H3, W3, c256); b.c2f("model.15", b.whole(cat14), b.whole(l15), rp(3), false);
  b.conv("model.16", b.whole(l15), {cat17, 0, c256}, 3, 2);                                          // 16, 17
  const int l18 = b.new_buf(H4, W4, c512); b.c2f("model.18", b.whole(cat17), b.whole(l18), rp(3), false);
  b.conv("model.19", b.whole(l18), {cat20, 0, c512}, 3, 2);                                          // 19, 20
  const int l21 = b.new_buf(H5, W5, c1024); b.c2f("model.21", b.whole(cat20), b.whole(l21), rp(3), false);
  // 22: Detect.  The first convolutions of the two branches read the same input: ONE launch into [box c2 | class c3]; the last 1x1
  // convolutions have a bias, no BN and no activation (fp32 operands in both modes); class logits padded to a multiple of 4 channels
  const int feats[3] = {l15, l18, l21};
  const int c2 = std::max(std::max(16, c256 / 4), 64), c3 = std::max(c256, std::min(e->nc, 100));
  const int c2p = pad32(c2), c3p = pad32(c3), npad = (e->nc + 3) / 4 * 4;
  e->npred = 0;
  for (int l = 0; l < 3; ++l) {
    const Buf f = e->bufs[feats[l]];
    const std::string box = "model.22.cv2." + std::to_string(l), cls = "model.22.cv3." + std::to_string(l);
    const int pair = b.new_buf(f.H, f.W, c2p + c3p);
    b.conv_pair(box + ".0", cls + ".0", b.whole(feats[l]), View{pair, 0, c2 + c3, c2p + c3p == c2 + c3 ? 0 : c2p + c3p}, c2, 3, 1, c2p);
    const View tb = {b.new_buf(f.H, f.W, c2p), 0, c2, pad_of(c2)}, tc = {b.new_buf(f.H, f.W, c3p), 0, c3, pad_of(c3)};
    b.conv(box + ".1", View{pair, 0, c2, pad_of(c2)}, tb, 3, 1);
    b.conv(cls + ".1", View{pair, c2p, c3, pad_of(c3)}, tc, 3, 1);
    const View rawb = {b.new_buf(f.H, f.W, 64), 0, 64}, rawc = {b.new_buf(f.H, f.W, npad), 0, npad};
    b.conv_bias(box + ".2", tb, rawb, 64);
    b.conv_bias(cls + ".2", tc, rawc, e->nc);
    e->ops.push_back({OP_DETECT, rawb, rawc, {-1, 0, 0}, -1, l});                                     // in: box logits, out: class logits
    e->npred += (int64_t)f.H * f.W;
  }
  ladd(e, "model.22.dfl.conv.weight", {1, 16, 1, 1});      // the constant 0 .. 15 (checked at upload): the decode kernel has it built in
  layout_weights(e);
  return EFFOCR_OK;
}

int pack_yolov8(effocr_yolov8* e, std::vector<char>& blob) {
  const auto& dfl = LP(e, "model.22.dfl.conv.weight");
  for (int k = 0; k < 16; ++k)
    if (dfl[k] != (float)k) return fail(EFFOCR_EINVAL, "yolov8_upload: model.22.dfl.conv.weight is not the constant 0 .. 15 (bin " + std::to_string(k) + " = " + std::to_string(dfl[k]) + ")");
  pack_convs(e, blob);
  return EFFOCR_OK;
}

}  // namespace
}  // namespace effocr

YOLOV8_API int effocr_yolov8_abi_version(void) { return EFFOCR_YOLOV8_ABI_VERSION; }
YOLOV8_API const char* effocr_yolov8_last_error(void) { return g_err.c_str(); }

YOLOV8_API int effocr_yolov8_create(const char* arch, int num_classes, int in_h, int in_w, effocr_yolov8_t** out) {
  if (!arch || !out) return fail(EFFOCR_EINVAL, "yolov8_create: NULL argument");
  int si = -1;
  for (int i = 0; i < 5; ++i) if (std::string(arch) == SCALES[i].name) si = i;
  if (si < 0) return fail(EFFOCR_EUNSUPPORTED, std::string("yolov8_create: unsupported architecture '") + arch + "' (yolov8n / s / m / l / x)");
  if (num_classes < 1 || num_classes > 80) return fail(EFFOCR_EINVAL, "yolov8_create: num_classes must be in 1..80");
  if (in_h < 32 || in_w < 32 || in_h % 32 || in_w % 32) return fail(EFFOCR_EINVAL, "yolov8_create: input size must be a positive multiple of 32 (stride)");
  std::unique_ptr<effocr_yolov8> e(new effocr_yolov8());
  e->nc = num_classes; e->no = num_classes + 5; e->in_h = in_h; e->in_w = in_w;
  if (const int rc = build_yolov8(e.get(), SCALES[si])) return rc;
  *out = e.release();
  return EFFOCR_OK;
}
YOLOV8_API void effocr_yolov8_destroy(effocr_yolov8_t* loc) { delete loc; }
YOLOV8_API int effocr_yolov8_num_params(const effocr_yolov8_t* loc) { return loc ? (int)loc->params.size() : 0; }
YOLOV8_API const char* effocr_yolov8_param_name(const effocr_yolov8_t* loc, int i) { return loc_param_name(loc, i); }
YOLOV8_API int64_t effocr_yolov8_param_numel(const effocr_yolov8_t* loc, int i) { return loc_param_numel(loc, i); }
YOLOV8_API int effocr_yolov8_set_param(effocr_yolov8_t* loc, const char* name, const float* host, int64_t numel) {
  return loc_set_param("yolov8", loc, name, host, numel);
}
YOLOV8_API size_t effocr_yolov8_weights_bytes(const effocr_yolov8_t* loc) { return loc ? loc->wbytes : 0; }
YOLOV8_API int effocr_yolov8_upload(effocr_yolov8_t* loc, void* weights_dev, size_t bytes) {
  return loc_upload("yolov8", loc, weights_dev, bytes, pack_yolov8);
}
YOLOV8_API int effocr_yolov8_set_option(effocr_yolov8_t* loc, const char* name, int value) { return loc_set_option("yolov8", loc, name, value); }
YOLOV8_API int64_t effocr_yolov8_num_predictions(const effocr_yolov8_t* loc) { return loc ? loc->npred : 0; }
YOLOV8_API int effocr_yolov8_num_outputs(const effocr_yolov8_t* loc) { return loc ? loc->no : 0; }
YOLOV8_API size_t effocr_yolov8_workspace_bytes(const effocr_yolov8_t* loc, int batch) {
  if (!loc || batch <= 0) return 0;
  return localizer_ws(loc, batch).total;
}

YOLOV8_API int effocr_yolov8_forward(effocr_yolov8_t* loc, const float* x_dev, int batch, float* pred_dev, void* workspace_dev, size_t workspace_bytes,
                                     void* stream) {
  hipStream_t s = LS(stream);
  // the 27-tap stem straight from NCHW (fp32 in both precision modes, as YOLOv5's: VALU work, the operand rounding starts at layer 1)
  auto stem = [&](const LConv& c, const View& out, float* out_dev) {
    if (!(c.k == 3 && c.stride == 2 && c.pad == 1 && c.cin == 3 && c.act)) return 0;
    const Buf o = loc->bufs[out.buf];
    const int rc = stem3x3s2_nchw(x_dev, reinterpret_cast<const float*>(loc->wdev + c.wt_off), c.cout_pad, reinterpret_cast<const float*>(loc->wdev + c.b_off),
                                  out_dev, batch, loc->in_h, loc->in_w, o.H, o.W, o.C, out.off, c.cout, c.cout_pad, s);
    return rc ? rc : 1;
  };
  auto detect = [&](const Op& op, auto& P) {
    const Buf bb = loc->bufs[op.in.buf], bc = loc->bufs[op.out.buf];
    const float strides[3] = {8.f, 16.f, 32.f};
    int64_t row0 = 0;
    for (const Op& o : loc->ops)
      if (o.type == OP_DETECT && o.level < op.level) row0 += (int64_t)loc->bufs[o.in.buf].H * loc->bufs[o.in.buf].W;
    return yolov8_decode(P(op.in.buf), bb.C, P(op.out.buf), bc.C, pred_dev, batch, bb.H, bb.W, loc->nc, strides[op.level], loc->npred, row0, s);
  };
  return loc_run_ops("yolov8", loc, x_dev, batch, pred_dev, workspace_dev, workspace_bytes, s, stem, detect);
}

// ---------------------------------------------------------------- test entry points: one kernel each, caller-made tensors
// yolov8.hip yolov8_decode: box [B * ny * nx][box_ld] (64 logits: 4 sides x 16 bins), cls [B * ny * nx][cls_ld] (nc logits) -> rows row0 ..
// row0 + ny * nx of pred [B][total][5 + nc]
YOLOV8_API int effocr_yolov8_op_decode(const float* box_dev, int box_ld, const float* cls_dev, int cls_ld, float* pred_dev, int batch, int ny, int nx, int nc,
                                       float stride, int64_t total, int64_t row0, void* stream) {
  if (!box_dev || !cls_dev || !pred_dev) return fail(EFFOCR_EINVAL, "yolov8_op_decode: NULL argument");
  if (batch < 0 || ny < 1 || nx < 1 || nc < 1 || box_ld < 64 || cls_ld < nc || total < 1 || row0 < 0) return fail(EFFOCR_EINVAL, "yolov8_op_decode: bad shape");
  return yolov8_decode(box_dev, box_ld, cls_dev, cls_ld, pred_dev, batch, ny, nx, nc, stride, total, row0, LS(stream));
}
// yolov8.hip stem3x3s2_nchw: x [B][3][H][W], wt [27 taps (ky, kx, c)][wt_ld], bias [cout_st] (zero from cout on) -> channels out_off ..
// out_off + cout_st of out [B * OH * OW][out_ld], the channels from cout on 0
YOLOV8_API int effocr_yolov8_op_stem(const float* x_dev, const float* wt_dev, int wt_ld, const float* bias_dev, float* out_dev, int batch, int H, int W, int OH,
                                     int OW, int out_ld, int out_off, int cout, int cout_st, void* stream) {
  if (!x_dev || !wt_dev || !bias_dev || !out_dev) return fail(EFFOCR_EINVAL, "yolov8_op_stem: NULL argument");
  if (batch < 0 || H < 1 || W < 1 || OH < 1 || OW < 1 || wt_ld < 1 || wt_ld % 4 || out_ld < 1 || out_off < 0 || cout < 1 || cout_st < 1)
    return fail(EFFOCR_EINVAL, "yolov8_op_stem: bad shape");
  return stem3x3s2_nchw(x_dev, wt_dev, wt_ld, bias_dev, out_dev, batch, H, W, OH, OW, out_ld, out_off, cout, cout_st, LS(stream));
}
