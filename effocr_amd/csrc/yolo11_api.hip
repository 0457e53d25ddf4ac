// C ABI of libeffocr_yolo11.so (include/effocr_yolo11.h): the ultralytics YOLO11 detection networks n / s / m / l / x as localizers.
// No ultralytics install was at hand: the builder follows yolo11.yaml, nn/modules and parse_model as published, checked by the five
// published parameter counts (tests/test_yolo11_host.py) — UNVERIFIED against a real checkpoint (DESIGN.md section 3 "YOLO11").
//   Conv        = Conv2d(bias=False) + BatchNorm2d(eps 1e-3) + SiLU (none with act=False)   -> BN folded on the host, SiLU in the epilogue
//   Bottleneck  = x + cv2(cv1(x)), both 3x3; hidden width c / 2 (e = 0.5) directly inside C3k2, c (e = 1.0) inside C3k
//   C3k         = cv3(cat(m1(m0(cv1(x))), cv2(x)))                           -> cv1 | cv2 in one launch, as YOLOv5's C3
//   C3k2        = cv2(cat(y0, y1, m0(y1), ...))  [y0 | y1] = cv1(x), m = Bottleneck or C3k  -> ONE buffer of 2 + n slices, as YOLOv8's C2f
//   C2PSA       = cv2(cat(a, b'))  [a | b] = cv1(x), b' = n PSABlocks on b:  b += proj(attention(qkv(b)) + pe(v));  b += ffn.1(ffn.0(b))
//                 attention and the depthwise pe are yolo11.hip's kernels; pe reads v out of the qkv tensor in place and adds the attention output
//   Detect      = box branch as YOLOv8's; class branch DWConv3x3, Conv1x1, DWConv3x3, Conv1x1, 1x1 (bias); decode = yolov8_decode
// The machinery (parameter table, buffers, channel-slice views, ops, BN folding, weight packing, zero-padded storage of widths that are
// no multiple of 32, the op loop) is localizer_core.hpp's, shared with the YOLOv5 and YOLOv8 engines; resnet.hip, yolo.hip and yolov8.hip
// are compiled into this library once more with hidden visibility.
#include "../../include/effocr_yolo11.h"
#include "enc_core.hpp"
#include "localizer_core.hpp"

#define YOLO11_API extern "C" __attribute__((visibility("default")))

using namespace effocr;

struct effocr_yolo11 : LocNet {};

namespace effocr {
namespace {

int pad_of(int c) { return pad32(c) == c ? 0 : pad32(c); }   // View::S of a tensor of c channels

struct V11Builder : Builder {
  View temp(int H, int W, int c) { return View{new_buf(H, W, pad32(c)), 0, c, pad_of(c)}; }
  // C3k(c -> c, 2 bottlenecks of e = 1.0): the concat buffer [m(cv1(x)) | cv2(x)] of two slices of c_ = c / 2 channels (stored padded
  // to 32 each: x's model.2 has c_ = 48), cv1 | cv2 in one launch, the second bottleneck writes slice 0 back
  void c3k(const std::string& name, View in, View out) {
    const int c_ = out.C / 2, cp = pad32(c_), H = e->bufs[in.buf].H, W = e->bufs[in.buf].W;
    const int cat = new_buf(H, W, 2 * cp);
    const View both = {cat, 0, 2 * c_, cp == c_ ? 0 : 2 * cp};
    conv_pair(name + ".cv1", name + ".cv2", in, both, c_, 1, 1);
    View cur = {cat, 0, c_, pad_of(c_)};
    for (int i = 0; i < 2; ++i) {
      const std::string m = name + ".m." + std::to_string(i);
      const View t = temp(H, W, c_);
      conv(m + ".cv1", cur, t, 3, 1);
      const View nxt = i == 1 ? View{cat, 0, c_, pad_of(c_)} : temp(H, W, c_);
      conv(m + ".cv2", t, nxt, 3, 1, 1, cur);
      cur = nxt;
    }
    conv(name + ".cv3", both, out, 1, 1);
    e->convs.back().icut = c_; e->convs.back().ishift = cp - c_;
  }
  // C3k2(c1 -> c2, n blocks, c3k, e): YOLOv8's C2f layout with c = int(c2 * e); block i reads slice 1 + i and writes slice 2 + i.  The
  // plain block is the DEFAULT Bottleneck (hidden width c / 2), with its shortcut in the backbone and in the head alike.
  void c3k2(const std::string& name, View in, View out, int n, bool c3k_, double ex) {
    const int c = (int)(out.C * ex), cp = pad32(c), H = e->bufs[in.buf].H, W = e->bufs[in.buf].W;
    const int cat = new_buf(H, W, (2 + n) * cp);
    auto slice = [&](int i) { return View{cat, i * cp, c, pad_of(c)}; };
    conv(name + ".cv1", in, View{cat, 0, 2 * c, cp == c ? 0 : 2 * cp}, 1, 1);
    e->convs.back().ocut = c; e->convs.back().oshift = cp - c;
    for (int i = 0; i < n; ++i) {
      const std::string m = name + ".m." + std::to_string(i);
      if (c3k_) { c3k(m, slice(1 + i), slice(2 + i)); continue; }
      const View t = temp(H, W, c / 2);
      conv(m + ".cv1", slice(1 + i), t, 3, 1);
      conv(m + ".cv2", t, slice(2 + i), 3, 1, 1, slice(1 + i));
    }
    conv(name + ".cv2", View{cat, 0, (2 + n) * c, cp == c ? 0 : (2 + n) * cp}, out, 1, 1);
    e->convs.back().icut = c; e->convs.back().ishift = cp - c;
  }
  // C2PSA(c1 -> c1, n PSABlocks), c = c1 / 2 (a multiple of 64: heads = c / 64).  [a | b] is one buffer; a block takes b through
  // b2 = b + proj(att + pe(v)) and back into b = b2 + ffn.1(ffn.0(b2)), so no convolution writes the tensor its residual comes from.
  // The convolutions without an activation (qkv, proj, ffn.1) still take bf16-rounded operands in that mode (LConv::q16).
  void c2psa(const std::string& name, View in, View out, int n) {
    const int c = in.C / 2, heads = c / 64, H = e->bufs[in.buf].H, W = e->bufs[in.buf].W;
    const int ab = new_buf(H, W, 2 * c), qkv = new_buf(H, W, 2 * c), att = new_buf(H, W, c), sum = new_buf(H, W, c), b2 = new_buf(H, W, c),
              hid = new_buf(H, W, 2 * c);
    const View b = {ab, c, c};
    conv(name + ".cv1", in, whole(ab), 1, 1);
    for (int j = 0; j < n; ++j) {
      const std::string p = name + ".m." + std::to_string(j);
      conv(p + ".attn.qkv", b, whole(qkv), 1, 1, 0); e->convs.back().q16 = 1;
      attention(whole(qkv), whole(att), heads);
      // pe on v rearranged head-major: its channel h * 64 + d is qkv channel h * 128 + 64 + d, read where it lies
      dwconv(p + ".attn.pe", View{qkv, 64, c}, whole(sum), 0, whole(att), 64, 128);
      conv(p + ".attn.proj", whole(sum), whole(b2), 1, 1, 0, b); e->convs.back().q16 = 1;
      conv(p + ".ffn.0", whole(b2), whole(hid), 1, 1);
      conv(p + ".ffn.1", whole(hid), b, 1, 1, 0, whole(b2)); e->convs.back().q16 = 1;
    }
    conv(name + ".cv2", whole(ab), out, 1, 1);
  }
};

struct Scale { const char* name; double depth, width; int max_channels; bool c3k; };
const Scale SCALES[5] = {{"yolo11n", 0.50, 0.25, 1024, false}, {"yolo11s", 0.50, 0.50, 1024, false}, {"yolo11m", 0.50, 1.00, 512, true},
                         {"yolo11l", 1.00, 1.00, 512, true}, {"yolo11x", 1.00, 1.50, 512, true}};

// parse_model over the yolo11.yaml rows at (depth, width, max_channels): channels ceil(min(c, max_channels) * width / 8) * 8, repeats
// max(round(n * depth), 1); m / l / x force c3k = True in every C3k2.  The neck concatenations are slices of one buffer each.
int build_yolo11(effocr_yolo11* e, const Scale& sc) {
  V11Builder b{{e}};
  auto ch = [&](int c) { return (int)ceil(std::min(c, sc.max_channels) * sc.width / 8) * 8; };
  const int n2 = std::max((int)lround(2 * sc.depth), 1);
  const int c64 = ch(64), c128 = ch(128), c256 = ch(256), c512 = ch(512), c1024 = ch(1024);
  if (c128 % 32 || c256 % 32 || c512 % 32 || c1024 % 128) return fail(EFFOCR_EUNSUPPORTED, "yolo11_create: a scale whose layer widths are no multiples of 32");
  const int H = e->in_h, W = e->in_w;
  const int H1 = down(H), W1 = down(W), H2 = down(H1), W2 = down(W1), H3 = down(H2), W3 = down(W2), H4 = down(H3), W4 = down(W3),
            H5 = down(H4), W5 = down(W4);
  if ((int64_t)H5 * W5 > Y11_MAX_TOKENS)
    return fail(EFFOCR_EUNSUPPORTED, "yolo11_create: " + std::to_string((int64_t)H5 * W5) + " tokens on the stride-32 map, the attention kernel is tested up to " +
                                         std::to_string(Y11_MAX_TOKENS) + " (1280 x 1280)");
  const View v0 = {b.new_buf(H1, W1, pad32(c64)), 0, c64, pad_of(c64)};
  b.stem("model.0", v0, 3, 1, 32, H1, W1);
  const int l1 = b.new_buf(H2, W2, c128);  b.conv("model.1", v0, b.whole(l1), 3, 2);
  const int l2 = b.new_buf(H2, W2, c256);  b.c3k2("model.2", b.whole(l1), b.whole(l2), n2, sc.c3k, 0.25);
  const int l3 = b.new_buf(H3, W3, c256);  b.conv("model.3", b.whole(l2), b.whole(l3), 3, 2);
  const int cat15 = b.new_buf(H3, W3, c512 + c512);         // [up(l13) | l4]
  const View l4 = {cat15, c512, c512};
  b.c3k2("model.4", b.whole(l3), l4, n2, sc.c3k, 0.25);
  const int l5 = b.new_buf(H4, W4, c512);  b.conv("model.5", l4, b.whole(l5), 3, 2);
  const int cat12 = b.new_buf(H4, W4, c1024 + c512);        // [up(l10) | l6]
  const View l6 = {cat12, c1024, c512};
  b.c3k2("model.6", b.whole(l5), l6, n2, true, 0.5);
  const int l7 = b.new_buf(H5, W5, c1024); b.conv("model.7", l6, b.whole(l7), 3, 2);
  const int l8 = b.new_buf(H5, W5, c1024); b.c3k2("model.8", b.whole(l7), b.whole(l8), n2, true, 0.5);
  // 9: SPPF(c1024, c1024, 5)
  const int cs = c1024 / 2;
  const int spp = b.new_buf(H5, W5, 4 * cs);
  b.conv("model.9.cv1", b.whole(l8), {spp, 0, cs}, 1, 1);
  for (int i = 0; i < 3; ++i) e->ops.push_back({OP_POOL, {spp, cs * i, cs}, {spp, cs * (i + 1), cs}, {-1, 0, 0}, -1, 0});
  const int l9 = b.new_buf(H5, W5, c1024); b.conv("model.9.cv2", b.whole(spp), b.whole(l9), 1, 1);
  // 10: C2PSA(c1024), its output straight into the last concat
  const int cat21 = b.new_buf(H5, W5, c512 + c1024);        // [l20 | l10]
  const View l10 = {cat21, c512, c1024};
  b.c2psa("model.10", b.whole(l9), l10, n2);
  // head: C3k2 with the shortcut ON (unlike YOLOv8's head)
  e->ops.push_back({OP_UP, l10, {cat12, 0, c1024}, {-1, 0, 0}, -1, 0});                               // 11, 12
  const int cat18 = b.new_buf(H4, W4, c256 + c512);         // [l17 | l13]
  const View l13 = {cat18, c256, c512};
  b.c3k2("model.13", b.whole(cat12), l13, n2, sc.c3k, 0.5);
  e->ops.push_back({OP_UP, l13, {cat15, 0, c512}, {-1, 0, 0}, -1, 0});                                // 14, 15
  const int l16 = b.new_buf(H3, W3, c256); b.c3k2("model.16", b.whole(cat15), b.whole(l16), n2, sc.c3k, 0.5);
  b.conv("model.17", b.whole(l16), {cat18, 0, c256}, 3, 2);                                          // 17, 18
  const int l19 = b.new_buf(H4, W4, c512); b.c3k2("model.19", b.whole(cat18), b.whole(l19), n2, sc.c3k, 0.5);
  b.conv("model.20", b.whole(l19), {cat21, 0, c512}, 3, 2);                                          // 20, 21
  const int l22 = b.new_buf(H5, W5, c1024); b.c3k2("model.22", b.whole(cat21), b.whole(l22), n2, true, 0.5);
  // 23: Detect.  The last 1x1 convolutions have a bias, no BN and no activation (fp32 operands in both modes); class logits padded to a
  // multiple of 4 channels.  c3 = max(c256, min(nc, 100)) is no multiple of 32 for yolo11n above 64 classes: stored padded, the depthwise
  // kernel runs over the stored channels (zero weights and bias there)
  const int feats[3] = {l16, l19, l22};
  const int c2 = std::max(std::max(16, c256 / 4), 64), c3 = std::max(c256, std::min(e->nc, 100));
  const int npad = (e->nc + 3) / 4 * 4;
  e->npred = 0;
  for (int l = 0; l < 3; ++l) {
    const Buf f = e->bufs[feats[l]];
    const std::string box = "model.23.cv2." + std::to_string(l), cls = "model.23.cv3." + std::to_string(l);
    const View tb0 = b.temp(f.H, f.W, c2), tb1 = b.temp(f.H, f.W, c2);
    b.conv(box + ".0", b.whole(feats[l]), tb0, 3, 1);
    b.conv(box + ".1", tb0, tb1, 3, 1);
    const View rawb = {b.new_buf(f.H, f.W, 64), 0, 64}, rawc = {b.new_buf(f.H, f.W, npad), 0, npad};
    b.conv_bias(box + ".2", tb1, rawb, 64);
    const View d0 = b.temp(f.H, f.W, f.C), e0 = b.temp(f.H, f.W, c3), d1 = b.temp(f.H, f.W, c3), e1 = b.temp(f.H, f.W, c3);
    b.dwconv(cls + ".0.0", b.whole(feats[l]), d0, 1);
    b.conv(cls + ".0.1", d0, e0, 1, 1);
    b.dwconv(cls + ".1.0", e0, d1, 1);
    b.conv(cls + ".1.1", d1, e1, 1, 1);
    b.conv_bias(cls + ".2", e1, rawc, e->nc);
    e->ops.push_back({OP_DETECT, rawb, rawc, {-1, 0, 0}, -1, l});                                     // in: box logits, out: class logits
    e->npred += (int64_t)f.H * f.W;
  }
  ladd(e, "model.23.dfl.conv.weight", {1, 16, 1, 1});      // the constant 0 .. 15 (checked at upload): the decode kernel has it built in
  layout_weights(e);
  return EFFOCR_OK;
}

int pack_yolo11(effocr_yolo11* e, std::vector<char>& blob) {
  const auto& dfl = LP(e, "model.23.dfl.conv.weight");
  for (int k = 0; k < 16; ++k)
    if (dfl[k] != (float)k) return fail(EFFOCR_EINVAL, "yolo11_upload: model.23.dfl.conv.weight is not the constant 0 .. 15 (bin " + std::to_string(k) + " = " + std::to_string(dfl[k]) + ")");
  pack_convs(e, blob);
  pack_dws(e, blob);
  return EFFOCR_OK;
}

}  // namespace
}  // namespace effocr

YOLO11_API int effocr_yolo11_abi_version(void) { return EFFOCR_YOLO11_ABI_VERSION; }
YOLO11_API const char* effocr_yolo11_last_error(void) { return g_err.c_str(); }

YOLO11_API int effocr_yolo11_create(const char* arch, int num_classes, int in_h, int in_w, effocr_yolo11_t** out) {
  if (!arch || !out) return fail(EFFOCR_EINVAL, "yolo11_create: NULL argument");
  int si = -1;
  for (int i = 0; i < 5; ++i) if (std::string(arch) == SCALES[i].name) si = i;
  if (si < 0) return fail(EFFOCR_EUNSUPPORTED, std::string("yolo11_create: unsupported architecture '") + arch + "' (yolo11n / s / m / l / x)");
  if (num_classes < 1 || num_classes > 80) return fail(EFFOCR_EINVAL, "yolo11_create: num_classes must be in 1..80");
  if (in_h < 32 || in_w < 32 || in_h % 32 || in_w % 32) return fail(EFFOCR_EINVAL, "yolo11_create: input size must be a positive multiple of 32 (stride)");
  std::unique_ptr<effocr_yolo11> e(new effocr_yolo11());
  e->nc = num_classes; e->no = num_classes + 5; e->in_h = in_h; e->in_w = in_w;
  if (const int rc = build_yolo11(e.get(), SCALES[si])) return rc;
  *out = e.release();
  return EFFOCR_OK;
}
YOLO11_API void effocr_yolo11_destroy(effocr_yolo11_t* loc) { delete loc; }
YOLO11_API int effocr_yolo11_num_params(const effocr_yolo11_t* loc) { return loc ? (int)loc->params.size() : 0; }
YOLO11_API const char* effocr_yolo11_param_name(const effocr_yolo11_t* loc, int i) { return loc_param_name(loc, i); }
YOLO11_API int64_t effocr_yolo11_param_numel(const effocr_yolo11_t* loc, int i) { return loc_param_numel(loc, i); }
YOLO11_API int effocr_yolo11_set_param(effocr_yolo11_t* loc, const char* name, const float* host, int64_t numel) {
  return loc_set_param("yolo11", loc, name, host, numel);
}
YOLO11_API size_t effocr_yolo11_weights_bytes(const effocr_yolo11_t* loc) { return loc ? loc->wbytes : 0; }
YOLO11_API int effocr_yolo11_upload(effocr_yolo11_t* loc, void* weights_dev, size_t bytes) {
  return loc_upload("yolo11", loc, weights_dev, bytes, pack_yolo11);
}
YOLO11_API int effocr_yolo11_set_option(effocr_yolo11_t* loc, const char* name, int value) { return loc_set_option("yolo11", loc, name, value); }
YOLO11_API int64_t effocr_yolo11_num_predictions(const effocr_yolo11_t* loc) { return loc ? loc->npred : 0; }
YOLO11_API int effocr_yolo11_num_outputs(const effocr_yolo11_t* loc) { return loc ? loc->no : 0; }
YOLO11_API size_t effocr_yolo11_workspace_bytes(const effocr_yolo11_t* loc, int batch) {
  if (!loc || batch <= 0) return 0;
  return localizer_ws(loc, batch).total;
}

YOLO11_API int effocr_yolo11_forward(effocr_yolo11_t* loc, const float* x_dev, int batch, float* pred_dev, void* workspace_dev, size_t workspace_bytes,
                                     void* stream) {
  hipStream_t s = LS(stream);
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
  auto extra = [&](const Op& op, auto& P) {
    const Buf i = loc->bufs[op.in.buf], o = loc->bufs[op.out.buf];
    if (op.type == OP_ATTN) return attention_nhwc(P(op.in.buf), i.C, op.in.off, P(op.out.buf), o.C, op.out.off, batch, i.H * i.W, op.level, s);
    if (op.type != OP_DW) return fail(EFFOCR_EINVAL, "yolo11_forward: unknown op kind");
    const LDw& d = loc->dws[op.conv];
    const float* add = op.res.buf >= 0 ? P(op.res.buf) : nullptr;
    return dwconv3x3_nhwc(P(op.in.buf), i.C, op.in.off, d.icut, d.istride, reinterpret_cast<const float*>(loc->wdev + d.w_off),
                          reinterpret_cast<const float*>(loc->wdev + d.b_off), d.act, add, add ? loc->bufs[op.res.buf].C : 0, add ? op.res.off : 0, P(op.out.buf), o.C,
                          op.out.off, batch, i.H, i.W, d.cst, s);
  };
  return loc_run_ops("yolo11", loc, x_dev, batch, pred_dev, workspace_dev, workspace_bytes, s, stem, detect, extra);
}

// ---------------------------------------------------------------- test entry points: one kernel each, dense tensors
YOLO11_API int effocr_yolo11_op_attention(const float* qkv_dev, int batch, int H, int W, int heads, float* out_dev, void* stream) {
  if (batch < 0 || H < 1 || W < 1 || heads < 1) return fail(EFFOCR_EINVAL, "yolo11_op_attention: bad shape");
  if ((int64_t)H * W > Y11_MAX_TOKENS) return fail(EFFOCR_EUNSUPPORTED, "yolo11_op_attention: more than " + std::to_string(Y11_MAX_TOKENS) + " tokens");
  return attention_nhwc(qkv_dev, heads * 128, 0, out_dev, heads * 64, 0, batch, H * W, heads, LS(stream));
}
YOLO11_API int effocr_yolo11_op_dwconv3x3(const float* x_dev, int batch, int H, int W, int C, int ld_in, const float* w_dev, const float* bias_dev, int silu,
                                          float* out_dev, int ld_out, void* stream) {
  if (batch < 0) return fail(EFFOCR_EINVAL, "yolo11_op_dwconv3x3: negative batch");
  return dwconv3x3_nhwc(x_dev, ld_in, 0, 0, 0, w_dev, bias_dev, silu, nullptr, 0, 0, out_dev, ld_out, 0, batch, H, W, C, LS(stream));
}
