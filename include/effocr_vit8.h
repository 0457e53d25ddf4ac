/* effocr_vit8.h — C ABI of libeffocr_vit8.so: the patch-8 ViT recognizer encoders
 * (timm.create_model("vit_small_patch8_224" | "vit_base_patch8_224", num_classes=0), what the reference
 * builds for `--auto_model_timm <name>` in train_effocr_recognizer.py / infer_effocr.py) on the MI355X (gfx950).
 * With 8x8 patches a 224^2 crop is 784 patch tokens + cls = 785 tokens, so the attention here streams its
 * key tiles with a running softmax instead of holding a crop's whole score matrix in a workgroup.
 *
 * A library of its own: libeffocr_hip.so is at its size cap (DESIGN.md "Library split"), so this one
 * neither links against it nor shares its error state; the GEMMs and the ViT helper kernels it needs are
 * compiled into it once more with hidden visibility.  Conventions are those of effocr_hip.h:
 *   - every *_dev pointer is caller-owned DEVICE memory; the library allocates no device memory;
 *   - calls that take a `stream` are asynchronous on it (hipStream_t passed as void*; NULL = the
 *     default stream);
 *   - 0 on success, a negative EFFOCR_VIT8_E* code on failure (the same values as effocr_hip.h's
 *     EFFOCR_E* codes), the message from effocr_vit8_last_error() (thread-local).
 *
 * The handle mirrors the encoder handle of effocr_hip.h: create -> set_param x N -> upload ->
 * forward ...; parameter names are timm's state-dict keys WITHOUT the "net." prefix and without the
 * classifier head: cls_token, pos_embed, patch_embed.proj.{weight,bias}, blocks.i.{norm1.*,attn.qkv.*,
 * attn.proj.*,norm2.*,mlp.fc1.*,mlp.fc2.*}, norm.{weight,bias}.
 */
#ifndef EFFOCR_VIT8_H
#define EFFOCR_VIT8_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an exported signature or the meaning of an argument changes; effocr_amd/_lib.py
 * refuses a library whose effocr_vit8_abi_version() differs */
#define EFFOCR_VIT8_ABI_VERSION 1

enum effocr_vit8_status {
  EFFOCR_VIT8_OK = 0,
  EFFOCR_VIT8_EINVAL = -1,        /* bad argument (NULL pointer, bad img_size or precision, wrong numel)  */
  EFFOCR_VIT8_EUNSUPPORTED = -2,  /* an architecture name this library does not implement                */
  EFFOCR_VIT8_EWORKSPACE = -3,    /* caller-provided workspace / weight buffer too small                 */
  EFFOCR_VIT8_EHIP = -4,          /* HIP runtime error                                                   */
  EFFOCR_VIT8_ESTATE = -5,        /* call order violated (forward before upload, a parameter never set)  */
  EFFOCR_VIT8_EOVERFLOW = -6      /* non-finite embedding (f16 operand overflow or non-finite input)     */
};

typedef struct effocr_vit8 effocr_vit8_t;

int effocr_vit8_abi_version(void);
const char* effocr_vit8_last_error(void);

/* arch: "vit_small_patch8_224" (width 384, depth 12, 6 heads), "vit_base_patch8_224" (width 768, depth 12,
 * 12 heads) or the test miniature "vit8_tiny_test" (width 128, depth 2, 2 heads); anything else is
 * EFFOCR_VIT8_EUNSUPPORTED.  img_size: a multiple of 8 from 8 to 224 (EFFOCR_VIT8_EINVAL otherwise); a crop
 * is (img_size/8)^2 + 1 tokens, the rows of pos_embed.  precision = EFFOCR_PREC_BF16 (0), EFFOCR_PREC_FP16 (1)
 * or EFFOCR_PREC_FP32 (2) of effocr_hip.h — the type of the linears' and the attention MFMAs' operands (the
 * residual stream, LayerNorm, softmax statistics, biases and the embedding are fp32 in every mode). */
int effocr_vit8_create(const char* arch, int img_size, int precision, effocr_vit8_t** out);
void effocr_vit8_destroy(effocr_vit8_t* enc);
int effocr_vit8_embed_dim(const effocr_vit8_t* enc);                  /* 384 / 768 (128 for vit8_tiny_test) */

int effocr_vit8_num_params(const effocr_vit8_t* enc);
const char* effocr_vit8_param_name(const effocr_vit8_t* enc, int i);  /* NULL when i is out of range */
int64_t effocr_vit8_param_numel(const effocr_vit8_t* enc, int i);     /* -1 when i is out of range */
/* host fp32 copy of one parameter (timm's layout and shape, numel must match) */
int effocr_vit8_set_param(effocr_vit8_t* enc, const char* name, const float* host, int64_t numel);
size_t effocr_vit8_weights_bytes(const effocr_vit8_t* enc);
/* packs every parameter into the device blob weights_dev (>= effocr_vit8_weights_bytes; synchronous copy) */
int effocr_vit8_upload(effocr_vit8_t* enc, void* weights_dev, size_t bytes);

/* Device workspace a forward of `batch` crops needs (0 for batch <= 0).  Calls run in sub-batches of
 * effocr_vit8_set_chunk crops (0 = the default: the largest sub-batch whose workspace stays under
 * 1 GB, at most 256 crops), so this stops growing at the sub-batch size.  The first 256 bytes hold the
 * sticky status word; zero them once in a fresh workspace. */
size_t effocr_vit8_workspace_bytes(const effocr_vit8_t* enc, int batch);
int effocr_vit8_set_chunk(effocr_vit8_t* enc, int crops_per_chunk);

/* x_dev [batch,3,img_size,img_size] fp32 (NCHW, ImageNet-normalised crops) -> emb_dev [batch,D] fp32:
 * norm(x)[:, 0], the final LayerNorm of the class token, L2-normalised (F.normalize) when
 * l2_normalize != 0.  A crop's embedding is bitwise independent of `batch` and of the chunk setting.  A
 * non-finite embedding ORs 1 into the workspace's status word. */
int effocr_vit8_forward(effocr_vit8_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize,
                        void* workspace_dev, size_t workspace_bytes, void* stream);

/* Reads and clears the status word (synchronises `stream`): EFFOCR_VIT8_EOVERFLOW if any forward on this
 * workspace since the last check produced a non-finite embedding, else 0. */
int effocr_vit8_check_status(const effocr_vit8_t* enc, const void* workspace_dev, void* stream);
/* Clears the status word without reading it (asynchronous on `stream`). */
int effocr_vit8_reset_status(const effocr_vit8_t* enc, void* workspace_dev, void* stream);

/* Test entry points (no product code calls them).
 * The streaming attention kernel alone on caller-made tensors: out = softmax(q k^T / 8) v, head dim 64.
 * qkv_dev [batch*tokens][3*heads*64] (q | k | v) and out_dev [batch*tokens][heads*64] in `dtype`'s element
 * type (EFFOCR_PREC_*), 1 <= tokens <= 1024 (EFFOCR_VIT8_EUNSUPPORTED otherwise). */
int effocr_vit8_op_attn(const void* qkv_dev, int batch, int tokens, int heads, int dtype, void* out_dev, void* stream);
/* The 8x8 patch embedding alone: x_dev [batch,3,img_size,img_size] fp32 -> out_dev [batch*T][embed_dim] fp32,
 * T = (img_size/8)^2 + 1: row b*T = cls_pos0_dev [embed_dim] (cls_token + pos_embed[0]), row b*T + 1 + p =
 * conv(x)[p] + bias_dev + pos_dev[1 + p].  w_dev [embed_dim][192] in `dtype`'s element type (the conv weight
 * flattened), bias_dev [embed_dim] and pos_dev [T][embed_dim] fp32; col_dev: scratch for the im2col rows,
 * batch*(T-1)*192 elements of `dtype`'s type.  embed_dim a multiple of 128. */
int effocr_vit8_op_patch_embed(const float* x_dev, int batch, int img_size, int embed_dim, int dtype, const void* w_dev,
                               const float* bias_dev, const float* cls_pos0_dev, const float* pos_dev, void* col_dev,
                               float* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFOCR_VIT8_H */
