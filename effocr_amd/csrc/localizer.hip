// C ABI of the YOLOv5 localizer engine (include/effocr_hip.h, "localizer" section): the network the reference runs
// through ONNXRuntime in onnx_engines/localizer_engine.py:14-66 (EffLocalizer, model_backend == 'yolo'), restated as a
// fixed sequence of gfx950 kernels.  The architecture is ultralytics YOLOv5 v6 at any of its five scales n / s / m / l / x
// (models/yolov5{n,s,m,l,x}.yaml: one layer table at depth 0.33 / 0.33 / 0.67 / 1.00 / 1.33, width 0.25 / 0.50 / 0.75 / 1.00 / 1.25):
// the reference ships no model definition (it loads an exported .onnx), so the builder below follows the published yaml /
// common.py / parse_model; parameter names are the ultralytics state-dict keys (model.<i>....).
//   Conv        = Conv2d(bias=False) + BatchNorm2d(eps 1e-3) + SiLU        -> BN folded on the host, SiLU in the epilogue
//   Bottleneck  = x + cv2(cv1(x)) (shortcut) | cv2(cv1(x))                  cv1 1x1, cv2 3x3, e = 1.0 inside C3
//   C3          = cv3(cat(m(cv1(x)), cv2(x)))                              -> both branches write slices of ONE buffer
//   SPPF        = cv2(cat(x', m(x'), m(m(x')), m(m(m(x')))))  x' = cv1(x)  -> the pool chain walks the slices of one buffer
//   Detect      = per level 1x1 conv (bias) -> sigmoid -> grid / anchor decode -> (bs, sum na*ny*nx, 5 + nc)
// The handle's pieces (parameter table, buffers, channel-slice views, ops), the BN folding / weight packing, the zero-padded storage of
// widths that are no multiple of 32 (n: 16, m: 48, x: 80 — the stem and model.2's inner C3 tensors) and the op loop of a forward are
// localizer_core.hpp's, shared with the YOLOv8 engine (yolov8_api.hip).
#include "../../include/effocr_hip.h"
#include "localizer_core.hpp"

using namespace effocr;

struct effocr_localizer : LocNet {
  int det_raw[3] = {-1, -1, -1};
  float anchors[3][6];
};

namespace effocr {
namespace {

struct V5Builder : Builder {
  // C3(c1 -> c2, n bottlenecks, shortcut): returns nothing, writes `out`.  cv1 and cv2 (two 1x1 Conv blocks on the same input) run as ONE
  // convolution of 2 c_ output channels straight into the concat buffer [m(cv1(x)) | cv2(x)] (round 4: the input is read once, half the
  // launches / prologues, a wider channel tile); the bottleneck chain starts from slice 0 and its last block writes slice 0 back — in
  // place when n = 1: its 3x3 convolution reads the temporary t, and the residual element is read by the lane that overwrites it.
  // A c_ that is not a multiple of 32 (model.2 of n / m / x) is stored as cp = c_ padded to 32 everywhere inside: the concat buffer is
  // [c_ | pad | c_ | pad], and cv3's weight columns skip the first pad.
  void c3(const std::string& name, View in, View out, int n, bool shortcut) {
    const int c_ = out.C / 2, cp = pad32(c_), H = e->bufs[in.buf].H, W = e->bufs[in.buf].W;
    const View tv = {0, 0, c_, cp == c_ ? 0 : cp};          // buffer / offset filled in below
    const int cat = new_buf(H, W, 2 * cp);
    conv_pair(name + ".cv1", name + ".cv2", in, View{cat, 0, 2 * c_, cp == c_ ? 0 : 2 * cp}, c_, 1, 1);
    View cur = tv; cur.buf = cat;
    for (int i = 0; i < n; ++i) {
      const std::string m = name + ".m." + std::to_string(i);
      View t = tv; t.buf = new_buf(H, W, cp);
      conv(m + ".cv1", cur, t, 1, 1);
      View nxt = tv; nxt.buf = (i == n - 1) ? cat : new_buf(H, W, cp);
      conv(m + ".cv2", t, nxt, 3, 1, 1, shortcut ? cur : View{-1, 0, 0});
      cur = nxt;
    }
    conv(name + ".cv3", View{cat, 0, 2 * c_, cp == c_ ? 0 : 2 * cp}, out, 1, 1);
    e->convs.back().icut = c_; e->convs.back().ishift = cp - c_;
  }
};

// parse_model over the v6 yaml rows at (depth, width): channels make_divisible(c * width, 8), repeats max(round(n * depth), 1) for n > 1.
// At (0.33, 0.50) this is exactly the yolov5s sequence of ops, buffers and convolutions.
void build_yolov5(effocr_localizer* e, double depth, double width) {
  V5Builder b{{e}};
  auto ch = [&](int c) { return (int)ceil(c * width / 8) * 8; };
  auto rp = [&](int n) { return n > 1 ? std::max((int)lround(n * depth), 1) : n; };
  const int c64 = ch(64), c128 = ch(128), c256 = ch(256), c512 = ch(512), c1024 = ch(1024);
  const int H = e->in_h, W = e->in_w;
  const int H1 = down(H), W1 = down(W), H2 = down(H1), W2 = down(W1), H3 = down(H2), W3 = down(W2), H4 = down(H3), W4 = down(W3),
            H5 = down(H4), W5 = down(W4);
  // 0: Conv(3, c64, 6, 2, 2) — stem: the direct kernels, or (A/B) im2col rows [.., 128] (108 taps + zeros) then a 1x1 implicit GEMM
  const View v0 = {b.new_buf(H1, W1, pad32(c64)), 0, c64, pad32(c64) == c64 ? 0 : pad32(c64)};
  b.stem("model.0", v0, 6, 2, 128, H1, W1);
  const int l1 = b.new_buf(H2, W2, c128);  b.conv("model.1", v0, b.whole(l1), 3, 2);
  const int l2 = b.new_buf(H2, W2, c128);  b.c3("model.2", b.whole(l1), b.whole(l2), rp(3), true);
  const int l3 = b.new_buf(H3, W3, c256);  b.conv("model.3", b.whole(l2), b.whole(l3), 3, 2);
  const int cat16 = b.new_buf(H3, W3, 2 * c256);            // [up(l14) | l4]
  b.c3("model.4", b.whole(l3), {cat16, c256, c256}, rp(6), true);
  const int l5 = b.new_buf(H4, W4, c512);  b.conv("model.5", {cat16, c256, c256}, b.whole(l5), 3, 2);
  const int cat12 = b.new_buf(H4, W4, 2 * c512);            // [up(l10) | l6]
  b.c3("model.6", b.whole(l5), {cat12, c512, c512}, rp(9), true);
  const int l7 = b.new_buf(H5, W5, c1024); b.conv("model.7", {cat12, c512, c512}, b.whole(l7), 3, 2);
  const int l8 = b.new_buf(H5, W5, c1024); b.c3("model.8", b.whole(l7), b.whole(l8), rp(3), true);
  // 9: SPPF(c1024, c1024, 5)
  const int cs = c1024 / 2;
  const int spp = b.new_buf(H5, W5, 4 * cs);
  b.conv("model.9.cv1", b.whole(l8), {spp, 0, cs}, 1, 1);
  for (int i = 0; i < 3; ++i) e->ops.push_back({OP_POOL, {spp, cs * i, cs}, {spp, cs * (i + 1), cs}, {-1, 0, 0}, -1, 0});
  const int l9 = b.new_buf(H5, W5, c1024); b.conv("model.9.cv2", b.whole(spp), b.whole(l9), 1, 1);
  // head
  const int cat22 = b.new_buf(H5, W5, 2 * c512);            // [l21 | l10]
  b.conv("model.10", b.whole(l9), {cat22, c512, c512}, 1, 1);
  e->ops.push_back({OP_UP, {cat22, c512, c512}, {cat12, 0, c512}, {-1, 0, 0}, -1, 0});                // 11, 12
  const int l13 = b.new_buf(H4, W4, c512); b.c3("model.13", b.whole(cat12), b.whole(l13), rp(3), false);
  const int cat19 = b.new_buf(H4, W4, 2 * c256);            // [l18 | l14]
  b.conv("model.14", b.whole(l13), {cat19, c256, c256}, 1, 1);
  e->ops.push_back({OP_UP, {cat19, c256, c256}, {cat16, 0, c256}, {-1, 0, 0}, -1, 0});                // 15, 16
  const int l17 = b.new_buf(H3, W3, c256); b.c3("model.17", b.whole(cat16), b.whole(l17), rp(3), false);
  b.conv("model.18", b.whole(l17), {cat19, 0, c256}, 3, 2);                                          // 18, 19
  const int l20 = b.new_buf(H4, W4, c512); b.c3("model.20", b.whole(cat19), b.whole(l20), rp(3), false);
  b.conv("model.21", b.whole(l20), {cat22, 0, c512}, 3, 2);                                          // 21, 22
  const int l23 = b.new_buf(H5, W5, c1024); b.c3("model.23", b.whole(cat22), b.whole(l23), rp(3), false);
  // 24: Detect — 1x1 conv with bias (no BN, no activation); output channels padded to a multiple of 4
  const int feats[3] = {l17, l20, l23};
  const int nout = 3 * e->no, npad = (nout + 3) / 4 * 4;
  e->npred = 0;
  for (int l = 0; l < 3; ++l) {
    const Buf f = e->bufs[feats[l]];
    e->det_raw[l] = b.new_buf(f.H, f.W, npad);
    b.conv_bias("model.24.m." + std::to_string(l), b.whole(feats[l]), {e->det_raw[l], 0, npad}, nout);
    e->ops.push_back({OP_DETECT, {e->det_raw[l], 0, npad}, {-1, 0, 0}, {-1, 0, 0}, -1, l});
    e->npred += (int64_t)3 * f.H * f.W;
  }
  ladd(e, "model.24.anchors", {3, 3, 2});                 // in units of the level's stride (ultralytics buffer)
  layout_weights(e);
}

int pack_localizer(effocr_localizer* e, std::vector<char>& blob) {
  pack_convs(e, blob);
  const auto& an = LP(e, "model.24.anchors");
  const float strides[3] = {8.f, 16.f, 32.f};
  for (int l = 0; l < 3; ++l)
    for (int j = 0; j < 6; ++j) e->anchors[l][j] = an[l * 6 + j] * strides[l];      // anchor_grid = anchors * stride (pixels)
  return EFFOCR_OK;
}

}  // namespace
}  // namespace effocr

extern "C" {

// arch: "yolov5n" | "yolov5s" | "yolov5m" | "yolov5l" | "yolov5x" (ultralytics v6, the depth / width multiples below); anything else
// EFFOCR_EUNSUPPORTED.  The builder lays out parameters, buffers, weights and workspace from the scale's own table.
int effocr_localizer_create(const char* arch, int num_classes, int in_h, int in_w, effocr_localizer_t** out) {
  if (!arch || !out) return fail(EFFOCR_EINVAL, "localizer_create: NULL argument");
  static const struct { const char* name; double depth, width; } scales[] = {
      {"yolov5n", 0.33, 0.25}, {"yolov5s", 0.33, 0.50}, {"yolov5m", 0.67, 0.75}, {"yolov5l", 1.00, 1.00}, {"yolov5x", 1.33, 1.25}};
  int si = -1;
  for (int i = 0; i < 5; ++i) if (std::string(arch) == scales[i].name) si = i;
  if (si < 0) return fail(EFFOCR_EUNSUPPORTED, std::string("localizer_create: unsupported architecture '") + arch + "' (yolov5n / s / m / l / x)");
  if (num_classes < 1 || num_classes > 80) return fail(EFFOCR_EINVAL, "localizer_create: num_classes must be in 1..80");
  if (in_h < 32 || in_w < 32 || in_h % 32 || in_w % 32) return fail(EFFOCR_EINVAL, "localizer_create: input size must be a positive multiple of 32 (stride)");
  std::unique_ptr<effocr_localizer> e(new effocr_localizer());
  e->nc = num_classes; e->no = num_classes + 5; e->in_h = in_h; e->in_w = in_w;
  build_yolov5(e.get(), scales[si].depth, scales[si].width);
  *out = e.release();
  return EFFOCR_OK;
}
void effocr_localizer_destroy(effocr_localizer_t* loc) { delete loc; }
int effocr_localizer_num_params(const effocr_localizer_t* loc) { return loc ? (int)loc->params.size() : 0; }
const char* effocr_localizer_param_name(const effocr_localizer_t* loc, int i) { return loc_param_name(loc, i); }
int64_t effocr_localizer_param_numel(const effocr_localizer_t* loc, int i) { return loc_param_numel(loc, i); }
int effocr_localizer_set_param(effocr_localizer_t* loc, const char* name, const float* host, int64_t numel) {
  return loc_set_param("localizer", loc, name, host, numel);
}
size_t effocr_localizer_weights_bytes(const effocr_localizer_t* loc) { return loc ? loc->wbytes : 0; }
int effocr_localizer_upload(effocr_localizer_t* loc, void* weights_dev, size_t bytes) {
  return loc_upload("localizer", loc, weights_dev, bytes, pack_localizer);
}
int effocr_localizer_set_option(effocr_localizer_t* loc, const char* name, int value) { return loc_set_option("localizer", loc, name, value); }
int64_t effocr_localizer_num_predictions(const effocr_localizer_t* loc) { return loc ? loc->npred : 0; }
int effocr_localizer_num_outputs(const effocr_localizer_t* loc) { return loc ? loc->no : 0; }
size_t effocr_localizer_workspace_bytes(const effocr_localizer_t* loc, int batch) {
  if (!loc || batch <= 0) return 0;
  return localizer_ws(loc, batch).total;
}

int effocr_localizer_forward(effocr_localizer_t* loc, const float* x_dev, int batch, float* pred_dev, void* workspace_dev, size_t workspace_bytes,
                             void* stream) {
  hipStream_t s = LS(stream);
  // the 6x6 stem straight from NCHW (fp32 in both precision modes: 108 taps per pixel are VALU work, the operand rounding of the bf16
  // mode starts at layer 1): the 32-channel kernel of yolov5s, 16-channel groups for the other widths
  auto stem = [&](const LConv& c, const View& out, float* out_dev) {
    const Buf o = loc->bufs[out.buf];
    const float* wt = reinterpret_cast<const float*>(loc->wdev + c.wt_off);
    const float* bias = reinterpret_cast<const float*>(loc->wdev + c.b_off);
    if (!(c.k == 6 && c.stride == 2 && c.pad == 2 && c.cin == 3 && c.kpad >= 108)) return 0;
    int rc;
    if (c.cout == 32 && c.cout_pad == 32)
      rc = stem6x6s2_nchw(x_dev, reinterpret_cast<const float*>(loc->wdev + c.w_off), c.kpad, wt, bias, out_dev, batch, loc->in_h, loc->in_w, o.H, o.W,
                          o.C, out.off, c.act, s);
    else if (c.act)
      rc = stem6x6s2_g16_nchw(x_dev, wt, c.cout_pad, bias, out_dev, batch, loc->in_h, loc->in_w, o.H, o.W, o.C, out.off, c.cout, c.cout_pad, s);
    else
      return 0;
    return rc ? rc : 1;
  };
  auto detect = [&](const Op& op, auto& P) {
    const Buf r = loc->bufs[op.in.buf];
    const float strides[3] = {8.f, 16.f, 32.f};
    int64_t row0 = 0;
    for (int l = 0; l < op.level; ++l) row0 += (int64_t)3 * loc->bufs[loc->det_raw[l]].H * loc->bufs[loc->det_raw[l]].W;
    return yolo_decode(P(op.in.buf), r.C, pred_dev, batch, r.H, r.W, 3, loc->no, strides[op.level], loc->anchors[op.level], loc->npred, row0, s);
  };
  return loc_run_ops("localizer", loc, x_dev, batch, pred_dev, workspace_dev, workspace_bytes, s, stem, detect);
}

int effocr_letterbox(const uint8_t* image_dev, int height, int width, int64_t row_stride, int bgr, int out_h, int out_w, int new_h, int new_w,
                     int top, int left, float* out_dev, void* stream) {
  if (!image_dev || !out_dev) return fail(EFFOCR_EINVAL, "letterbox: NULL device pointer");
  if (row_stride < (int64_t)3 * width) return fail(EFFOCR_EINVAL, "letterbox: row stride smaller than 3 * width");
  return letterbox_u8(image_dev, height, width, row_stride, bgr, out_h, out_w, new_h, new_w, top, left, 114.0f, out_dev, LS(stream));
}

size_t effocr_nms_workspace_bytes(int n, int max_nms) { return nms_workspace_bytes(n, max_nms); }
size_t effocr_nms_batch_workspace_bytes(int n, int max_det, int max_nms) { return nms_greedy_applies(n, max_det, max_nms) ? 0 : nms_workspace_bytes(n, max_nms); }

int effocr_nms(const float* pred_dev, int n, int num_classes, float conf_thres, float iou_thres, int max_det, int max_nms, float max_wh, int agnostic,
               float* out_dev, int* count_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (n > 0 && (!pred_dev || !workspace_dev)) return fail(EFFOCR_EINVAL, "nms: NULL device pointer");
  if (!out_dev || !count_dev) return fail(EFFOCR_EINVAL, "nms: NULL output pointer");
  return nms_yolo(pred_dev, n, num_classes, conf_thres, iou_thres, max_det, max_nms, max_wh, agnostic, out_dev, count_dev, workspace_dev, workspace_bytes,
                  LS(stream));
}

int effocr_nms_batch(const float* pred_dev, int batch, int n, int num_classes, float conf_thres, float iou_thres, int max_det, int max_nms, float max_wh,
                     int agnostic, float* out_dev, int* count_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (batch > 0 && n > 0 && !pred_dev) return fail(EFFOCR_EINVAL, "nms: NULL device pointer");
  if (batch > 0 && (!out_dev || !count_dev)) return fail(EFFOCR_EINVAL, "nms: NULL output pointer");
  if (batch > 0 && n > 0 && !nms_greedy_applies(n, max_det, max_nms) && !workspace_dev) return fail(EFFOCR_EINVAL, "nms: NULL workspace");
  return nms_yolo_batch(pred_dev, batch, n, num_classes, conf_thres, iou_thres, max_det, max_nms, max_wh, agnostic, out_dev, count_dev, workspace_dev,
                        workspace_bytes, LS(stream));
}

}  // extern "C"
