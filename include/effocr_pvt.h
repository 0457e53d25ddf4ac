/* effocr_pvt.h — C ABI of libeffocr_pvt.so: the PVTv2 recognizer encoders
 * (timm.create_model("pvt_v2_b0" | "pvt_v2_b1" | "pvt_v2_b2" | "pvt_v2_b3" | "pvt_v2_b4" | "pvt_v2_b5", num_classes=0),
 * what the reference builds for `--auto_model_timm <name>` in train_effocr_recognizer.py / infer_effocr.py) on the
 * MI355X (gfx950).  PVTv2 is a four-stage hierarchical transformer: every stage opens with an overlapping patch
 * embedding (7x7 stride 4 on the crop, then 3x3 stride 2 on the previous stage's tokens) that ends in a LayerNorm,
 * runs pre-norm blocks whose attention lets all N tokens attend to the (img/32)^2 <= 49 tokens a strided
 * convolution + LayerNorm reduces them to (ratios 8, 4, 2, 1 per stage), and whose MLP has a depthwise 3x3 + GELU
 * between its two linears, and closes with a LayerNorm.  The embedding is the mean of the last stage's tokens.
 *
 * A library of its own: libeffocr_hip.so is at its size cap (DESIGN.md "Library split"), so this one neither
 * links against it nor shares its error state.  Conventions are those of effocr_hip.h:
 *   - every *_dev pointer is caller-owned DEVICE memory; the library allocates no device memory;
 *   - calls that take a `stream` are asynchronous on it (hipStream_t passed as void*; NULL = the default stream);
 *   - 0 on success, a negative EFFOCR_PVT_E* code on failure (the same values as effocr_hip.h's EFFOCR_E* codes),
 *     the message from effocr_pvt_last_error() (thread-local).
 *
 * The handle mirrors the encoder handle of effocr_hip.h: create -> set_param x N -> upload -> forward ...;
 * parameter names are timm's state-dict keys WITHOUT the "net." prefix and without the classifier head (written
 * from memory of timm's pvt_v2.py, not verified against a timm install):
 *   patch_embed.{proj, norm}.{weight, bias}
 *   stages.i.downsample.{proj, norm}.{weight, bias}                                            (i = 1, 2, 3)
 *   stages.i.blocks.j.{norm1, attn.q, attn.kv, attn.proj, attn.sr, attn.norm, norm2, mlp.fc1, mlp.dwconv, mlp.fc2}.{weight, bias}
 *   stages.i.norm.{weight, bias}
 * (attn.sr and attn.norm do not exist in stage 3, whose reduction ratio is 1).
 */
#ifndef EFFOCR_PVT_H
#define EFFOCR_PVT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an exported signature or the meaning of an argument changes; effocr_amd/_lib.py
 * refuses a library whose effocr_pvt_abi_version() differs */
#define EFFOCR_PVT_ABI_VERSION 1

enum effocr_pvt_status {
  EFFOCR_PVT_OK = 0,
  EFFOCR_PVT_EINVAL = -1,        /* bad argument (NULL pointer, bad img_size or precision, wrong numel)  */
  EFFOCR_PVT_EUNSUPPORTED = -2,  /* an architecture name or a shape this library does not implement      */
  EFFOCR_PVT_EWORKSPACE = -3,    /* caller-provided workspace / weight buffer too small                 */
  EFFOCR_PVT_EHIP = -4,          /* HIP runtime error                                                   */
  EFFOCR_PVT_ESTATE = -5,        /* call order violated (forward before upload, a parameter never set)  */
  EFFOCR_PVT_EOVERFLOW = -6      /* non-finite embedding (f16 operand overflow or non-finite input)     */
};

typedef struct effocr_pvt effocr_pvt_t;

int effocr_pvt_abi_version(void);
const char* effocr_pvt_last_error(void);

/* arch: "pvt_v2_b0" ... "pvt_v2_b5", or the test miniatures "pvt_v2_mini32_test" (widths 32-64-96-128, head
 * width 32) and "pvt_v2_mini64_test" (widths 64-128-192-256, head width 64); anything else (pvt_v2_b2_li, PVT v1)
 * is EFFOCR_PVT_EUNSUPPORTED.  img_size: a multiple of 32 from 32 to 224 (EFFOCR_PVT_EINVAL otherwise): every
 * stage then reduces to (img_size/32)^2 <= 49 keys.  The parameters do not depend on img_size.  precision =
 * EFFOCR_PREC_BF16 (0), EFFOCR_PREC_FP16 (1) or EFFOCR_PREC_FP32 (2) of effocr_hip.h — the type of the weights, of
 * the activations between the kernels and of the MFMA operands (the residual stream, accumulators, LayerNorm and
 * softmax statistics, biases and the embedding are fp32 in every mode). */
int effocr_pvt_create(const char* arch, int img_size, int precision, effocr_pvt_t** out);
void effocr_pvt_destroy(effocr_pvt_t* enc);
int effocr_pvt_embed_dim(const effocr_pvt_t* enc);                  /* 256 for pvt_v2_b0, 512 for b1 ... b5 */

int effocr_pvt_num_params(const effocr_pvt_t* enc);
const char* effocr_pvt_param_name(const effocr_pvt_t* enc, int i);  /* NULL when i is out of range */
int64_t effocr_pvt_param_numel(const effocr_pvt_t* enc, int i);     /* -1 when i is out of range */
/* host fp32 copy of one parameter (timm's layout and shape, numel must match) */
int effocr_pvt_set_param(effocr_pvt_t* enc, const char* name, const float* host, int64_t numel);
size_t effocr_pvt_weights_bytes(const effocr_pvt_t* enc);
/* packs every parameter into the device blob weights_dev (>= effocr_pvt_weights_bytes; synchronous copy) */
int effocr_pvt_upload(effocr_pvt_t* enc, void* weights_dev, size_t bytes);

/* Device workspace a forward of `batch` crops needs (0 for batch <= 0).  Calls run in sub-batches of
 * effocr_pvt_set_chunk crops (0 = the default: the largest sub-batch whose workspace stays under 1 GB, at most
 * 256 crops), so this stops growing at the sub-batch size.  The first 256 bytes hold the sticky status word; zero
 * them once in a fresh workspace. */
size_t effocr_pvt_workspace_bytes(const effocr_pvt_t* enc, int batch);
int effocr_pvt_set_chunk(effocr_pvt_t* enc, int crops_per_chunk);

/* x_dev [batch,3,img_size,img_size] fp32 (NCHW, ImageNet-normalised crops) -> emb_dev [batch,D] fp32: the mean
 * over the last stage's normalised tokens (what timm returns with num_classes=0), L2-normalised (F.normalize) when
 * l2_normalize != 0.  A crop's embedding is bitwise independent of `batch`, of the crop's position and of the
 * chunk setting.  A non-finite embedding ORs 1 into the workspace's status word. */
int effocr_pvt_forward(effocr_pvt_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize,
                       void* workspace_dev, size_t workspace_bytes, void* stream);

/* Reads and clears the status word (synchronises `stream`): EFFOCR_PVT_EOVERFLOW if any forward on this
 * workspace since the last check produced a non-finite embedding, else 0. */
int effocr_pvt_check_status(const effocr_pvt_t* enc, const void* workspace_dev, void* stream);
/* Clears the status word without reading it (asynchronous on `stream`). */
int effocr_pvt_reset_status(const effocr_pvt_t* enc, void* workspace_dev, void* stream);

/* Test entry points (no product code calls them).  `dtype` is an EFFOCR_PREC_* value: the element type of every
 * buffer not declared fp32.  Every pointer must be 16-byte aligned.
 *
 * The attention kernel alone: out = softmax(q k^T / sqrt(hd)) v per (crop, head).  q_dev [batch*n][heads*hd], kv_dev
 * [batch*m][2*heads*hd] (head h's keys at h*hd, its values at heads*hd + h*hd), out_dev [batch*n][heads*hd];
 * hd 32 or 64, 1 <= m <= 49.  Rounding points of the 16-bit modes: p rounded for the P V product, the output
 * rounded on the store; everything else fp32 (csrc/pvt.hpp). */
int effocr_pvt_op_attention(const void* q_dev, const void* kv_dev, int batch, int n, int m, int heads, int hd, int dtype,
                            void* out_dev, void* stream);
/* Depthwise 3x3 (zero pad 1) + bias + exact GELU on token rows in_dev / out_dev [batch][h*w][c] (c % 4 == 0); w_dev
 * [9][c] fp32 (row ky*3 + kx), bias_dev [c] fp32. */
int effocr_pvt_op_dwconv_gelu(const void* in_dev, int batch, int h, int w, int c, const float* w_dev, const float* bias_dev,
                              int dtype, void* out_dev, void* stream);
/* The 7x7 stride-4 pad-3 patch embedding + LayerNorm (eps 1e-6): x_dev [batch][3][img][img] fp32 (rounded to dtype as
 * it is read), w_dev [cout][160] in dtype (k = (c*7 + ky)*7 + kx, zeros from 147 on), bias / lnw / lnb [cout] fp32 ->
 * out_dev [batch*(img/4)^2][cout] fp32.  img % 4 == 0, cout % 32 == 0, cout <= 512. */
int effocr_pvt_op_stem(const float* x_dev, int batch, int img, int cout, const void* w_dev, const float* bias_dev,
                       const float* lnw_dev, const float* lnb_dev, int dtype, float* out_dev, void* stream);
/* A convolution of token rows as an implicit GEMM + LayerNorm (eps 1e-6): in_dev [batch][side*side][cin] in dtype,
 * w_dev [cout][ksize*ksize*cin] in dtype (k = (ky*ksize + kx)*cin + c), bias / lnw / lnb [cout] fp32 -> out_dev
 * [batch*oside^2][cout] fp32, oside = (side + 2 pad - ksize)/stride + 1.  ksize 3, stride 2, pad 1: the down-sampling
 * patch embedding; ksize = stride = sr, pad 0: the spatial reduction.  cin % 8 == 0, cout % 32 == 0, cout <= 512. */
int effocr_pvt_op_conv_ln(const void* in_dev, int batch, int side, int cin, int cout, int ksize, int stride, int pad,
                          const void* w_dev, const float* bias_dev, const float* lnw_dev, const float* lnb_dev, int dtype,
                          float* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFOCR_PVT_H */
