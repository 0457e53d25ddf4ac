// Host-side core of the YOLO localizer engines: localizer.hip (YOLOv5, in libeffocr_hip.so), yolov8_api.hip (YOLOv8, in
// libeffocr_yolov8.so) and yolo11_api.hip (YOLO11, in libeffocr_yolo11.so) describe their networks with the same pieces — a table of named parameters, NHWC activation buffers, channel-slice
// views of them and a flat list of ops — and share the weight layout, the BN folding / packing and the op loop of a forward.  What
// differs between the two families stays in their own files: the layer table, the stem kernel and the Detect decode (the two hooks of
// loc_run_ops).  No kernel and no device memory here.  Include it from ONE translation unit per shared library.
//
// Activations NHWC fp32; convolutions = resnet.hip's implicit GEMM on exact fp32 MFMA.  That GEMM takes input channels in steps of 32:
// a tensor of another width is STORED with its channel count padded to 32; its producer writes the padding as zeros (zero weight rows,
// zero bias, SiLU(0) = 0) and its consumers' weights have zero columns there, so the products add exact zeros.
#pragma once
#include "common.hpp"
#include "kernels.hpp"

#include <math.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace effocr {
namespace {

struct LParam { std::string name; std::vector<int64_t> shape; int64_t numel; std::vector<float> data; bool set; };
struct Buf { int H, W, C; };                             // NHWC activation buffer (per image)
struct View { int buf, off, C, S = 0; };                 // channel slice of a buffer: C channels, S (0: = C) stored channels (C padded to 32)
int stored(const View& v) { return v.S ? v.S : v.C; }
enum { OP_STEM = 0, OP_CONV = 1, OP_UP = 2, OP_POOL = 3, OP_DETECT = 4,
       OP_ATTN = 5,                                      // multi-head self-attention over the map's pixels (YOLO11's C2PSA): in = the qkv tensor, level = heads
       OP_DW = 6 };                                      // depthwise 3x3, stride 1 (+ res: a tensor added behind the activation): conv = index into dws
struct Op {
  int type;
  View in, out, res;                                     // res.buf < 0: no residual
  int conv;                                              // index into convs
  int level;                                             // OP_DETECT
};
struct LConv { std::string w, bn, bias; int cin, cout, cout_pad, k, stride, pad, act; size_t w_off, b_off; int kpad; size_t w16_off; size_t wt_off;
               std::string w2, bn2; int cout1 = 0;
               int cin_st = 0, icut = 0, ishift = 0;    // weight columns: cin_st stored input channels per tap; the input is segments of icut channels, each stored ishift channels wider: channel ci sits at ci + (ci / icut) * ishift
               int row2 = 0, cout2 = 0;                 // pair: the second block's cout2 rows start at weight row row2 (= cout1 unless padded)   // w2 / bn2: a second Conv block stacked behind the first cout1 output channels (C3's cv1 | cv2 in one launch)   // w16: the bf16 copy, rows padded to 64 k
               int q16 = 0;                             // 1: bf16-rounded operands in the bf16_operands mode although the block has no activation (YOLO11's qkv / proj / ffn.1)
               int ocut = 0, oshift = 0; };             // one block whose output is segments of ocut channels, each stored oshift channels wider (0: one segment, padded at its end)

// a depthwise 3x3 Conv block (Conv2d(groups = C, bias = False) + BN + optional SiLU): weights [cst][9] (tap ky * 3 + kx), BN folded; its
// input channel ci is read at in.off + (ci / icut) * istride + ci % icut (icut = 0: at in.off + ci)
struct LDw { std::string w, bn; int c, cst, act, icut, istride; size_t w_off, b_off; };

// what both localizer handles are: the C handle structs derive from it
struct LocNet {
  int nc = 2, no = 7, in_h = 640, in_w = 640;
  std::vector<LParam> params;
  std::map<std::string, int> index;
  std::vector<Buf> bufs;
  std::vector<Op> ops;
  std::vector<LConv> convs;
  std::vector<LDw> dws;
  int stem_col = -1;                                     // buffer of the stem's im2col rows
  size_t wbytes = 0;
  const char* wdev = nullptr;
  int64_t npred = 0;
  int direct_stem = 1;                                   // 0: the stem through im2col + the 1x1 implicit GEMM (A/B)
  int call_size_invariant = 0;                           // 1: no convolution splits K (the split count follows the call's tile count): a row of predictions is a function of its image alone
  int bf16 = 0;                                          // 1: bf16-operand MFMAs for every convolution with an activation (Detect's 1x1 heads stay fp32)
};

void ladd(LocNet* e, const std::string& name, std::vector<int64_t> shape) {
  LParam p; p.name = name; p.shape = shape; p.numel = 1; for (auto v : shape) p.numel *= v; p.set = false;
  e->index[name] = (int)e->params.size();
  e->params.push_back(std::move(p));
}

int pad32(int c) { return (c + 31) / 32 * 32; }
int down(int v) { return (v - 1) / 2 + 1; }              // conv k, stride 2, pad k/2: ceil(v / 2)

struct Builder {
  LocNet* e;
  int new_buf(int H, int W, int C) { e->bufs.push_back({H, W, C}); return (int)e->bufs.size() - 1; }
  View whole(int b) { return {b, 0, e->bufs[b].C}; }
  void add_bn_conv_params(const std::string& n, int co, int ci, int k) {
    ladd(e, n + ".conv.weight", {co, ci, k, k});
    ladd(e, n + ".bn.weight", {co}); ladd(e, n + ".bn.bias", {co}); ladd(e, n + ".bn.running_mean", {co}); ladd(e, n + ".bn.running_var", {co});
  }
  // ultralytics Conv block `name` (= "<name>.conv" + "<name>.bn"): in -> out slice
  void conv(const std::string& name, View in, View out, int k, int s, int act = 1, View res = {-1, 0, 0}) {
    LConv c; c.w = name + ".conv.weight"; c.bn = name + ".bn"; c.bias = "";
    c.cin = in.C; c.cout = out.C; c.cout_pad = stored(out); c.k = k; c.stride = s; c.pad = k / 2; c.act = act; c.kpad = 0;
    c.cin_st = stored(in); c.icut = in.C;
    add_bn_conv_params(name, out.C, in.C, k);
    e->convs.push_back(c);
    e->ops.push_back({OP_CONV, in, out, res, (int)e->convs.size() - 1, 0});
  }
  // a convolution with a bias and neither BN nor activation (the Detect heads' last 1x1): weight `name`.weight, bias `name`.bias
  void conv_bias(const std::string& name, View in, View out, int cout) {
    LConv c; c.w = name + ".weight"; c.bn = ""; c.bias = name + ".bias";
    c.cin = in.C; c.cout = cout; c.cout_pad = stored(out); c.k = 1; c.stride = 1; c.pad = 0; c.act = 0; c.kpad = 0; c.cin_st = stored(in); c.icut = in.C;
    ladd(e, c.w, {cout, in.C, 1, 1}); ladd(e, c.bias, {cout});
    e->convs.push_back(c);
    e->ops.push_back({OP_CONV, in, out, {-1, 0, 0}, (int)e->convs.size() - 1, 0});
  }
  // two Conv blocks of the same geometry on the same input in ONE launch: output channels [0, c1) = block `n1`, [c1, out.C) = block `n2`
  // (out stored as two halves of stored(out) / 2 channels each when padded; row2 >= 0: the second block's first stored channel instead)
  void conv_pair(const std::string& n1, const std::string& n2, View in, View out, int c1, int k, int s, int row2 = -1) {
    LConv c; c.w = n1 + ".conv.weight"; c.bn = n1 + ".bn"; c.bias = ""; c.w2 = n2 + ".conv.weight"; c.bn2 = n2 + ".bn"; c.cout1 = c1;
    c.cin = in.C; c.cout = out.C; c.cout_pad = stored(out); c.k = k; c.stride = s; c.pad = k / 2; c.act = 1; c.kpad = 0;
    c.cin_st = stored(in); c.icut = in.C; c.row2 = row2 >= 0 ? row2 : out.S ? stored(out) / 2 : c1; c.cout2 = out.C - c1;
    add_bn_conv_params(n1, c1, in.C, k);
    add_bn_conv_params(n2, out.C - c1, in.C, k);
    e->convs.push_back(c);
    e->ops.push_back({OP_CONV, in, out, {-1, 0, 0}, (int)e->convs.size() - 1, 0});
  }
  // ultralytics Conv / DWConv block `name` with k = 3, groups = channels: in -> out (+ res behind the activation).  icut / istride: LDw
  void dwconv(const std::string& name, View in, View out, int act, View res = {-1, 0, 0}, int icut = 0, int istride = 0) {
    LDw d; d.w = name + ".conv.weight"; d.bn = name + ".bn"; d.c = out.C; d.cst = stored(out); d.act = act; d.icut = icut; d.istride = istride; d.w_off = d.b_off = 0;
    ladd(e, d.w, {out.C, 1, 3, 3});
    ladd(e, name + ".bn.weight", {out.C}); ladd(e, name + ".bn.bias", {out.C}); ladd(e, name + ".bn.running_mean", {out.C}); ladd(e, name + ".bn.running_var", {out.C});
    e->dws.push_back(d);
    e->ops.push_back({OP_DW, in, out, res, (int)e->dws.size() - 1, 0});
  }
  // softmax(scale q k^T) v per head over the pixels of `in` = [heads x (q 32 | k 32 | v 64)] channels -> out = heads x 64 channels
  void attention(View in, View out, int heads) { e->ops.push_back({OP_ATTN, in, out, {-1, 0, 0}, -1, heads}); }
  // the stem Conv(3, c, k, 2, pad): OP_STEM, its im2col rows (kpad wide) only on the direct_stem = 0 path
  void stem(const std::string& name, View out, int k, int pad, int kpad, int H1, int W1) {
    e->stem_col = new_buf(H1, W1, kpad);
    LConv c; c.w = name + ".conv.weight"; c.bn = name + ".bn"; c.bias = ""; c.cin = 3; c.cout = out.C; c.cout_pad = stored(out); c.k = k; c.stride = 2;
    c.pad = pad; c.act = 1; c.kpad = kpad; c.cin_st = 3; c.icut = 3;
    add_bn_conv_params(name, out.C, 3, k);
    e->convs.push_back(c);
    e->ops.push_back({OP_STEM, {-1, 0, 3}, out, {-1, 0, 0}, (int)e->convs.size() - 1, 0});
  }
};

// blob offsets of every convolution: fp32 weights, bias, the bf16 copy and (stem) the [tap][channel] transpose
void layout_weights(LocNet* e) {
  size_t off = 0;
  for (auto& c : e->convs) {
    const size_t K = c.kpad ? (size_t)c.kpad : (size_t)c.k * c.k * c.cin_st;
    c.w_off = off; off = align_up(off + (size_t)c.cout_pad * K * 4, 256);
    c.b_off = off; off = align_up(off + (size_t)c.cout_pad * 4, 256);
    c.w16_off = off; off = align_up(off + (size_t)c.cout_pad * ((K + 63) / 64 * 64) * 2, 256);
    c.wt_off = 0;
    if (c.kpad) { c.wt_off = off; off = align_up(off + (size_t)c.k * c.k * c.cin_st * c.cout_pad * 4, 256); }   // stem: [tap][channel] transpose (scalar-weight kernel)
  }
  for (auto& d : e->dws) {
    d.w_off = off; off = align_up(off + (size_t)d.cst * 9 * 4, 256);
    d.b_off = off; off = align_up(off + (size_t)d.cst * 4, 256);
  }
  e->wbytes = off;
}

const std::vector<float>& LP(const LocNet* e, const std::string& n) { return e->params[e->index.at(n)].data; }

void pack_convs(const LocNet* e, std::vector<char>& blob) {
  for (const LConv& c : e->convs) {
    const int K = c.k * c.k * c.cin_st, Kp = c.kpad ? c.kpad : K;
    float* wd = reinterpret_cast<float*>(blob.data() + c.w_off);
    float* bd = reinterpret_cast<float*>(blob.data() + c.b_off);
    for (int co = 0; co < c.cout_pad; ++co) {
      for (int kk = 0; kk < Kp; ++kk) wd[(size_t)co * Kp + kk] = 0.f;
      bd[co] = 0.f;
      const bool second = !c.w2.empty() && co >= c.row2;    // stacked pair: rows [row2, row2 + cout2) come from the second block
      int cs = second ? co - c.row2 : co;                   // the row inside its own block
      if (c.ocut) {                                         // segmented output: stored row -> (segment, channel) or a segment's padding
        const int seg = co / (c.ocut + c.oshift), within = co % (c.ocut + c.oshift);
        cs = within < c.ocut ? seg * c.ocut + within : c.cout;
      }
      if (cs >= (second ? c.cout2 : c.w2.empty() ? c.cout : c.cout1)) continue;   // channel padding: zero row, zero bias
      const auto& w = LP(e, second ? c.w2 : c.w);
      const std::string& bn = second ? c.bn2 : c.bn;
      double sc = 1.0;
      if (!bn.empty()) {                                 // BatchNorm2d(eps = 1e-3: ultralytics initialize_weights) folded in
        const double g = LP(e, bn + ".weight")[cs], bt = LP(e, bn + ".bias")[cs], mu = LP(e, bn + ".running_mean")[cs],
                     var = LP(e, bn + ".running_var")[cs];
        sc = g / sqrt(var + 1e-3);
        bd[co] = (float)(bt - mu * sc);
      } else {
        bd[co] = LP(e, c.bias)[cs];
      }
      for (int ky = 0; ky < c.k; ++ky)
        for (int kx = 0; kx < c.k; ++kx)
          for (int ci = 0; ci < c.cin; ++ci)
            wd[(size_t)co * Kp + (ky * c.k + kx) * c.cin_st + ci + ci / c.icut * c.ishift] =
                (float)((double)w[(((size_t)cs * c.cin + ci) * c.k + ky) * c.k + kx] * sc);
    }
    if (c.kpad) {
      float* wt = reinterpret_cast<float*>(blob.data() + c.wt_off);
      for (int kk = 0; kk < K; ++kk)
        for (int co = 0; co < c.cout_pad; ++co) wt[(size_t)kk * c.cout_pad + co] = wd[(size_t)co * Kp + kk];
    }
    // bf16 copy of the folded weights (round to nearest even), rows zero-padded to a multiple of 64 k
    const int Kp64 = (Kp + 63) / 64 * 64;
    uint16_t* w16 = reinterpret_cast<uint16_t*>(blob.data() + c.w16_off);
    for (int co = 0; co < c.cout_pad; ++co)
      for (int kk = 0; kk < Kp64; ++kk) {
        uint32_t u = 0;
        if (kk < Kp) {
          const float f = wd[(size_t)co * Kp + kk];
          memcpy(&u, &f, 4);
          u = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;    // finite values only (folded weights)
        }
        w16[(size_t)co * Kp64 + kk] = (uint16_t)u;
      }
  }
}

// depthwise blocks: BN folded as above, fp32 only; stored channels past c are zero rows with a zero bias (SiLU(0) = 0)
void pack_dws(const LocNet* e, std::vector<char>& blob) {
  for (const LDw& d : e->dws) {
    float* wd = reinterpret_cast<float*>(blob.data() + d.w_off);
    float* bd = reinterpret_cast<float*>(blob.data() + d.b_off);
    const auto& w = LP(e, d.w);
    for (int ch = 0; ch < d.cst; ++ch) {
      bd[ch] = 0.f;
      for (int t = 0; t < 9; ++t) wd[(size_t)ch * 9 + t] = 0.f;
      if (ch >= d.c) continue;
      const double g = LP(e, d.bn + ".weight")[ch], bt = LP(e, d.bn + ".bias")[ch], mu = LP(e, d.bn + ".running_mean")[ch],
                   var = LP(e, d.bn + ".running_var")[ch];
      const double sc = g / sqrt(var + 1e-3);
      bd[ch] = (float)(bt - mu * sc);
      for (int t = 0; t < 9; ++t) wd[(size_t)ch * 9 + t] = (float)((double)w[(size_t)ch * 9 + t] * sc);
    }
  }
}

constexpr size_t LOC_SPLIT_BYTES = (size_t)16 << 20;   // split-K scratch of conv2d_nhwc (the deep layers at small batches: few tiles, long K)
struct LWs { std::vector<size_t> off; size_t split, total; };
LWs localizer_ws(const LocNet* e, int B) {
  LWs w; size_t off = 0;
  for (size_t i = 0; i < e->bufs.size(); ++i) {
    const Buf& b = e->bufs[i];
    w.off.push_back(off);
    if ((int)i == e->stem_col && e->direct_stem) continue;   // the im2col rows of the stem (840 MB at 16 x 640 x 640 for YOLOv5's) exist only on the A/B path
    off = align_up(off + (size_t)B * b.H * b.W * b.C * 4, 256);
  }
  w.split = off; off += LOC_SPLIT_BYTES;
  w.total = off;
  return w;
}

hipStream_t LS(void* s) { return static_cast<hipStream_t>(s); }

// ---------------------------------------------------------------- bodies of the entry points both handles share (`what`: the message prefix)
const char* loc_param_name(const LocNet* loc, int i) {
  if (!loc || i < 0 || i >= (int)loc->params.size()) return nullptr;
  return loc->params[i].name.c_str();
}
int64_t loc_param_numel(const LocNet* loc, int i) {
  if (!loc || i < 0 || i >= (int)loc->params.size()) return -1;
  return loc->params[i].numel;
}
int loc_set_param(const std::string& what, LocNet* loc, const char* name, const float* host, int64_t numel) {
  if (!loc || !name || !host) return fail(EFFOCR_EINVAL, what + "_set_param: NULL argument");
  auto it = loc->index.find(name);
  if (it == loc->index.end()) return fail(EFFOCR_EINVAL, what + "_set_param: unknown parameter '" + name + "'");
  LParam& p = loc->params[it->second];
  if (p.numel != numel) return fail(EFFOCR_EINVAL, what + "_set_param: '" + name + "' expects " + std::to_string(p.numel) + " elements, got " + std::to_string(numel));
  p.data.assign(host, host + numel);
  p.set = true;
  return EFFOCR_OK;
}
// pack(loc, blob): pack_convs + whatever else the family keeps from its parameters; a non-zero return refuses the upload
template <typename Net, typename Pack>
int loc_upload(const std::string& what, Net* loc, void* weights_dev, size_t bytes, Pack pack) {
  if (!loc || !weights_dev) return fail(EFFOCR_EINVAL, what + "_upload: NULL argument");
  if (bytes < loc->wbytes) return fail(EFFOCR_EWORKSPACE, what + "_upload: weight buffer too small");
  for (const LParam& p : loc->params)
    if (!p.set) return fail(EFFOCR_ESTATE, what + "_upload: parameter '" + p.name + "' was never set");
  std::vector<char> blob(loc->wbytes, 0);
  if (const int rc = pack(loc, blob)) return rc;
  const hipError_t er = hipMemcpy(weights_dev, blob.data(), loc->wbytes, hipMemcpyHostToDevice);
  if (er != hipSuccess) return fail(EFFOCR_EHIP, what + "_upload: hipMemcpy: " + hipGetErrorString(er));
  loc->wdev = static_cast<const char*>(weights_dev);
  return EFFOCR_OK;
}
int loc_set_option(const std::string& what, LocNet* loc, const char* name, int value) {
  if (!loc || !name) return fail(EFFOCR_EINVAL, what + "_set_option: NULL argument");
  if (std::string(name) == "bf16_operands") { loc->bf16 = value != 0; return EFFOCR_OK; }
  if (std::string(name) == "direct_stem") { loc->direct_stem = value != 0; return EFFOCR_OK; }
  if (std::string(name) == "call_size_invariant") {
    if (value != 0 && value != 1) return fail(EFFOCR_EINVAL, what + "_set_option: call_size_invariant must be 0 or 1");
    loc->call_size_invariant = value; return EFFOCR_OK;
  }
  return fail(EFFOCR_EINVAL, what + "_set_option: unknown option '" + name + "'");
}

// One forward: the ops in order.  direct_stem(conv, out view, out pointer) runs the family's own stem kernel and returns 1 when it did, 0
// when the shape is not its (then, as with direct_stem = 0, im2col + the 1x1 implicit GEMM), < 0 on an error; detect(op, P) decodes a level;
// extra(op, P) runs the op kinds whose kernels only some libraries have (OP_ATTN, OP_DW).
template <typename Stem, typename Detect, typename Extra>
int loc_run_ops(const std::string& what, const LocNet* loc, const float* x_dev, int batch, float* pred_dev, void* workspace_dev, size_t workspace_bytes,
                hipStream_t s, Stem direct_stem, Detect detect, Extra extra) {
  if (!loc) return fail(EFFOCR_EINVAL, what + "_forward: NULL localizer");
  if (batch < 0) return fail(EFFOCR_EINVAL, what + "_forward: negative batch");
  if (batch == 0) return EFFOCR_OK;
  if (!x_dev || !pred_dev || !workspace_dev) return fail(EFFOCR_EINVAL, what + "_forward: NULL device pointer");
  if (!loc->wdev) return fail(EFFOCR_ESTATE, what + "_forward: weights were not uploaded");
  const LWs w = localizer_ws(loc, batch);
  if (workspace_bytes < w.total) return fail(EFFOCR_EWORKSPACE, what + "_forward: workspace too small");
  char* ws = static_cast<char*>(workspace_dev);
  auto P = [&](int b) { return reinterpret_cast<float*>(ws + w.off[b]); };
  int rc;
  for (const Op& op : loc->ops) {
    switch (op.type) {
      case OP_STEM: {
        const LConv& c = loc->convs[op.conv];
        const Buf o = loc->bufs[op.out.buf];
        if (loc->direct_stem) {
          if ((rc = direct_stem(c, op.out, P(op.out.buf))) < 0) return rc;
          if (rc > 0) break;
        }
        if ((rc = im2col_nchw(x_dev, P(loc->stem_col), batch, 3, loc->in_h, loc->in_w, c.k, c.k, c.stride, c.pad, o.H, o.W, c.kpad, s))) return rc;
        ConvArgs a{};
        a.in = P(loc->stem_col); a.w = reinterpret_cast<const float*>(loc->wdev + c.w_off); a.bias = reinterpret_cast<const float*>(loc->wdev + c.b_off);
        a.out = P(op.out.buf); a.B = batch * o.H * o.W; a.H = 1; a.W = 1; a.Cin = c.kpad; a.Cout = c.cout_pad; a.KH = 1; a.KW = 1; a.stride = 1; a.pad = 0;
        a.OH = 1; a.OW = 1; a.silu = c.act; a.out_ld = o.C; a.out_off = op.out.off;
        if (loc->bf16 && c.act) a.w16 = loc->wdev + c.w16_off;
        a.partial = loc->call_size_invariant ? nullptr : reinterpret_cast<float*>(ws + w.split); a.partial_bytes = LOC_SPLIT_BYTES;
        if ((rc = conv2d_nhwc(a, s))) return rc;
        break;
      }
      case OP_CONV: {
        const LConv& c = loc->convs[op.conv];
        const Buf i = loc->bufs[op.in.buf], o = loc->bufs[op.out.buf];
        ConvArgs a{};
        a.in = P(op.in.buf); a.in_ld = i.C; a.in_off = op.in.off;
        a.w = reinterpret_cast<const float*>(loc->wdev + c.w_off); a.bias = reinterpret_cast<const float*>(loc->wdev + c.b_off);
        a.out = P(op.out.buf); a.out_ld = o.C; a.out_off = op.out.off;
        if (op.res.buf >= 0) { a.resid = P(op.res.buf); a.res_ld = loc->bufs[op.res.buf].C; a.res_off = op.res.off; }
        a.B = batch; a.H = i.H; a.W = i.W; a.Cin = c.cin_st; a.Cout = c.cout_pad; a.KH = c.k; a.KW = c.k; a.stride = c.stride; a.pad = c.pad;
        a.OH = o.H; a.OW = o.W; a.silu = c.act;
        if (loc->bf16 && (c.act || c.q16)) a.w16 = loc->wdev + c.w16_off;
        a.partial = loc->call_size_invariant ? nullptr : reinterpret_cast<float*>(ws + w.split); a.partial_bytes = LOC_SPLIT_BYTES;
        if ((rc = conv2d_nhwc(a, s))) return rc;
        break;
      }
      case OP_UP: {
        const Buf i = loc->bufs[op.in.buf], o = loc->bufs[op.out.buf];
        if ((rc = upsample2x_nhwc(P(op.in.buf), i.C, op.in.off, P(op.out.buf), o.C, op.out.off, batch, i.H, i.W, op.in.C, s))) return rc;
        break;
      }
      case OP_POOL: {
        const Buf i = loc->bufs[op.in.buf];
        if ((rc = maxpool5_nhwc(P(op.in.buf), i.C, op.in.off, P(op.out.buf), i.C, op.out.off, batch, i.H, i.W, op.in.C, s))) return rc;
        break;
      }
      case OP_DETECT: {
        if ((rc = detect(op, P))) return rc;
        break;
      }
      default: {
        if ((rc = extra(op, P))) return rc;
        break;
      }
    }
  }
  return EFFOCR_OK;
}
// the networks made of the five op kinds above alone (YOLOv5, YOLOv8)
template <typename Stem, typename Detect>
int loc_run_ops(const std::string& what, const LocNet* loc, const float* x_dev, int batch, float* pred_dev, void* workspace_dev, size_t workspace_bytes,
                hipStream_t s, Stem direct_stem, Detect detect) {
  auto none = [&](const Op&, auto&) { return fail(EFFOCR_EINVAL, what + "_forward: an op kind this library has no kernel for"); };
  return loc_run_ops(what, loc, x_dev, batch, pred_dev, workspace_dev, workspace_bytes, s, direct_stem, detect, none);
}

}  // namespace
}  // namespace effocr
