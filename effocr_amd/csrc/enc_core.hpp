// Host-side core of the C-ABI libraries: the error plumbing common.hpp declares, the small packing helpers and — for every
// encoder-family library (each <family>_api.hip whose handle derives from EncoderCore) — the handle's shared fields, the default
// sub-batch size and the bodies of the entry points that do not depend on the family.  token_core.hpp (Swin, BEiT, patch-8 ViT) and
// resnet_core.hpp (ResNet-34/50, BiT) build on it.  No kernel and no device memory: everything here runs once per handle or once per call.
//
// Include it from exactly ONE translation unit per shared library (its *_api.hip).  The error plumbing below is that library's
// definition of set_error / fail / check_launch / device_cus for every kernel file linked into it, and g_err is that library's own
// thread-local message: last_error is per shared object.
#pragma once
#include "common.hpp"
#include "kernels.hpp"

#include <string.h>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace effocr {

// ---------------------------------------------------------------- error plumbing (one definition per library, not inline)
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int fail(int code, const std::string& msg) { g_err = msg; return code; }
int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EFFOCR_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  return EFFOCR_OK;
}
int device_cus() {
  static int cache[64] = {0};                            // benign race: every thread computes the same value
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cache[dev] == 0) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    cache[dev] = v;
  }
  return cache[dev];
}

// ---------------------------------------------------------------- small helpers
// offsets into a blob or a workspace, every buffer aligned to 256 bytes
struct Alloc {
  size_t off = 0;
  size_t take(size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; }
};

static inline uint16_t f32_to_bf16(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN
  u += 0x7fffu + ((u >> 16) & 1u);                                            // round to nearest even
  return (uint16_t)(u >> 16);
}
static inline uint16_t f32_to_f16(float f) { _Float16 h = (_Float16)f; uint16_t u; memcpy(&u, &h, 2); return u; }

// n fp32 values into the blob: as they are / rounded once to the operand type of `prec`
static inline void put_f32(std::vector<char>& blob, size_t off, const float* src, size_t n) { memcpy(blob.data() + off, src, n * 4); }
static inline void put_op(std::vector<char>& blob, size_t off, const float* src, size_t n, int prec) {
  if (prec == PREC_FP32) { memcpy(blob.data() + off, src, n * 4); return; }
  uint16_t* d = reinterpret_cast<uint16_t*>(blob.data() + off);
  if (prec == PREC_BF16) for (size_t i = 0; i < n; ++i) d[i] = f32_to_bf16(src[i]);
  else for (size_t i = 0; i < n; ++i) d[i] = f32_to_f16(src[i]);
}

static inline hipStream_t S(void* s) { return static_cast<hipStream_t>(s); }

// ---------------------------------------------------------------- the encoder-family handle
// What every family handle holds; `struct effocr_<family>` derives from it and adds its tables and blob offsets.
struct EncoderCore {
  struct Param { std::string name; int64_t numel; std::vector<float> data; bool set; };
  int img = 224, prec = PREC_FP16, D = 0, chunk = 0;    // chunk: crops per sub-batch, 0 = the family's default
  std::vector<Param> params;                             // in timm's state-dict order
  std::map<std::string, int> index;
  size_t wbytes = 0;
  const char* wdev = nullptr;                            // device blob after upload

  void add_param(const std::string& name, int64_t numel) {
    index[name] = (int)params.size();
    params.push_back(Param{name, numel, {}, false});
  }
  void add_bn(const std::string& p, int c) {
    add_param(p + ".weight", c); add_param(p + ".bias", c);
    add_param(p + ".running_mean", c); add_param(p + ".running_var", c);
  }
  const std::vector<float>& P(const std::string& n) const { return params[index.at(n)].data; }
};

// The bodies of effocr_<family>_*: `fam` is the family's short name, the prefix of every message.
static inline const char* enc_param_name(const EncoderCore* e, int i) {
  if (!e || i < 0 || i >= (int)e->params.size()) return nullptr;
  return e->params[i].name.c_str();
}
static inline int64_t enc_param_numel(const EncoderCore* e, int i) {
  if (!e || i < 0 || i >= (int)e->params.size()) return -1;
  return e->params[i].numel;
}

static inline int enc_set_param(const char* fam, EncoderCore* e, const char* name, const float* host, int64_t numel) {
  if (!e || !name || !host) return fail(EFFOCR_EINVAL, std::string(fam) + "_set_param: NULL argument");
  auto it = e->index.find(name);
  if (it == e->index.end()) return fail(EFFOCR_EINVAL, std::string(fam) + "_set_param: unknown parameter '" + name + "'");
  EncoderCore::Param& p = e->params[it->second];
  if (p.numel != numel)
    return fail(EFFOCR_EINVAL, std::string(fam) + "_set_param: '" + name + "' expects " + std::to_string(p.numel) + " elements, got " + std::to_string(numel));
  p.data.assign(host, host + numel);
  p.set = true;
  return EFFOCR_OK;
}

// pack(e, blob): the family's host-side packing of the parameter table into the zeroed blob
template <typename H>
int enc_upload(const char* fam, H* e, void* weights_dev, size_t bytes, void (*pack)(const H*, std::vector<char>&)) {
  if (!e || !weights_dev) return fail(EFFOCR_EINVAL, std::string(fam) + "_upload: NULL argument");
  if (bytes < e->wbytes) return fail(EFFOCR_EWORKSPACE, std::string(fam) + "_upload: weight buffer too small");
  for (const EncoderCore::Param& p : e->params)
    if (!p.set) return fail(EFFOCR_ESTATE, std::string(fam) + "_upload: parameter '" + p.name + "' was never set");
  std::vector<char> blob(e->wbytes, 0);
  pack(e, blob);
  const hipError_t er = hipMemcpy(weights_dev, blob.data(), e->wbytes, hipMemcpyHostToDevice);
  if (er != hipSuccess) return fail(EFFOCR_EHIP, std::string(fam) + "_upload: hipMemcpy: " + hipGetErrorString(er));
  e->wdev = static_cast<const char*>(weights_dev);
  return EFFOCR_OK;
}

static inline int enc_set_chunk(const char* fam, EncoderCore* e, int crops_per_chunk) {
  if (!e || crops_per_chunk < 0) return fail(EFFOCR_EINVAL, std::string(fam) + "_set_chunk: bad argument");
  e->chunk = crops_per_chunk;
  return EFFOCR_OK;
}

// crops per sub-batch: the handle's own setting, else as many as keep ws_total(crops) — the family's workspace size — within `budget`, at
// most max_chunk; never more than the batch.  The shrink loop matters only where the per-buffer alignment makes ws_total grow faster than
// the crop count (EfficientNet); where every buffer is linear in the crop count it ends at once.
template <typename WsTotal>
int enc_default_chunk(const EncoderCore* e, int batch, size_t budget, int max_chunk, WsTotal ws_total) {
  int c = e->chunk;
  if (c <= 0) {
    c = (int)std::min<size_t>(max_chunk, std::max<size_t>(1, budget / ws_total(1)));
    while (c > 1 && ws_total(c) > budget) --c;
  }
  return c < batch ? c : batch;
}

// The argument checks of effocr_<family>_forward; `need` is the family's workspace_bytes(batch) (0 for a NULL handle).  A batch of 0
// passes them: the caller returns before it touches a pointer.
static inline int enc_forward_args(const char* fam, const EncoderCore* e, const void* x_dev, int batch, const float* emb_dev,
                                   const void* workspace_dev, size_t workspace_bytes, size_t need) {
  if (!e) return fail(EFFOCR_EINVAL, std::string(fam) + "_forward: NULL encoder");
  if (batch < 0) return fail(EFFOCR_EINVAL, std::string(fam) + "_forward: negative batch");
  if (batch == 0) return EFFOCR_OK;
  if (!x_dev || !emb_dev || !workspace_dev) return fail(EFFOCR_EINVAL, std::string(fam) + "_forward: NULL device pointer");
  if (!e->wdev) return fail(EFFOCR_ESTATE, std::string(fam) + "_forward: weights were not uploaded");
  if (workspace_bytes < need) return fail(EFFOCR_EWORKSPACE, std::string(fam) + "_forward: workspace too small");
  return EFFOCR_OK;
}

// The sub-batch loop: forward(x, crops, emb) runs one sub-batch of at most `chunk` crops.  Every kernel computes a crop from that crop's
// data alone, so the embeddings are bit-identical for every chunk setting.
template <typename F>
int enc_forward_chunks(const EncoderCore* e, const float* x_dev, int batch, int chunk, float* emb_dev, F forward) {
  const size_t img_elems = (size_t)3 * e->img * e->img;
  for (int b0 = 0; b0 < batch; b0 += chunk) {
    const int rc = forward(x_dev + (size_t)b0 * img_elems, std::min(chunk, batch - b0), emb_dev + (size_t)b0 * e->D);
    if (rc) return rc;
  }
  return EFFOCR_OK;
}

// What enc_check_status reports in the f16 mode, where more than one family words it alike.
constexpr const char* ENC_F16_OPERAND_OVERFLOW =
    "forward: non-finite embedding — an f16 operand overflowed (a LayerNorm, attention or GELU output beyond 65504) or the "
    "input was not finite; use precision bf16 or fp32 for this checkpoint";
constexpr const char* ENC_F16_ACTIVATION_OVERFLOW =
    "forward: non-finite embedding — an f16 activation overflowed (beyond 65504) or the input was not finite; use "
    "precision bf16 or fp32 for this checkpoint";

// Read and clear the sticky status word at workspace offset 0 (synchronises `stream`).  fp16_msg: what the family's f16 mode can overflow.
static inline int enc_check_status(const char* fam, const EncoderCore* e, const void* workspace_dev, void* stream, const char* fp16_msg) {
  if (!e || !workspace_dev) return fail(EFFOCR_EINVAL, std::string(fam) + "_check_status: NULL argument");
  int st = 0;
  hipError_t er = hipMemcpyAsync(&st, workspace_dev, sizeof(int), hipMemcpyDeviceToHost, S(stream));
  if (er == hipSuccess) er = hipStreamSynchronize(S(stream));
  if (er == hipSuccess && st != 0) er = hipMemsetAsync(const_cast<void*>(workspace_dev), 0, sizeof(int), S(stream));   // read-and-clear
  if (er != hipSuccess) return fail(EFFOCR_EHIP, std::string(fam) + "_check_status: " + hipGetErrorString(er));
  if (st != 0)
    return fail(EFFOCR_EOVERFLOW, e->prec == PREC_FP16 ? fp16_msg : "forward: non-finite embedding — the input crops or the weights hold inf / nan");
  return EFFOCR_OK;
}

// Clear the status word without reading it (asynchronous on `stream`).
static inline int enc_reset_status(const char* fam, const EncoderCore* e, void* workspace_dev, void* stream) {
  if (!e || !workspace_dev) return fail(EFFOCR_EINVAL, std::string(fam) + "_reset_status: NULL argument");
  const hipError_t er = hipMemsetAsync(workspace_dev, 0, sizeof(int), S(stream));
  if (er != hipSuccess) return fail(EFFOCR_EHIP, std::string(fam) + "_reset_status: " + hipGetErrorString(er));
  return EFFOCR_OK;
}

}  // namespace effocr
