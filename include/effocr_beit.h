/* effocr_beit.h — C ABI of libeffocr_beit.so: the BEiT base recognizer encoders
 * (timm.create_model("beit_base_patch16_224" | "beitv2_base_patch16_224", num_classes=0), what the reference
 * builds for `--auto_model_timm <name>` in train_effocr_recognizer.py / infer_effocr.py) on the MI355X (gfx950).
 * The two names are one module with the same keys and shapes (they differ in how they were pre-trained), so
 * they run the same code here.
 *
 * A library of its own: libeffocr_hip.so is at its size cap (DESIGN.md "Library split"), so this one
 * neither links against it nor shares its error state; the GEMMs and the ViT helper kernels it needs are
 * compiled into it a second time with hidden visibility.  Conventions are those of effocr_hip.h:
 *   - every *_dev pointer is caller-owned DEVICE memory; the library allocates no device memory;
 *   - calls that take a `stream` are asynchronous on it (hipStream_t passed as void*; NULL = the
 *     default stream);
 *   - 0 on success, a negative EFFOCR_BEIT_E* code on failure (the same values as effocr_hip.h's
 *     EFFOCR_E* codes), the message from effocr_beit_last_error() (thread-local).
 *
 * The handle mirrors the encoder handle of effocr_hip.h: create -> set_param x N -> upload ->
 * forward ...; parameter names are timm's state-dict keys WITHOUT the "net." prefix and without the
 * classifier head: cls_token, patch_embed.proj.{weight,bias}, blocks.i.{gamma_1,gamma_2,norm1.*,
 * attn.q_bias,attn.v_bias,attn.relative_position_bias_table,attn.qkv.weight,attn.proj.*,norm2.*,
 * mlp.fc1.*,mlp.fc2.*}, fc_norm.{weight,bias}.
 */
#ifndef EFFOCR_BEIT_H
#define EFFOCR_BEIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an exported signature or the meaning of an argument changes; effocr_amd/_lib.py
 * refuses a library whose effocr_beit_abi_version() differs */
#define EFFOCR_BEIT_ABI_VERSION 1

enum effocr_beit_status {
  EFFOCR_BEIT_OK = 0,
  EFFOCR_BEIT_EINVAL = -1,        /* bad argument (NULL pointer, bad img_size or precision, wrong numel)  */
  EFFOCR_BEIT_EUNSUPPORTED = -2,  /* an architecture name this library does not implement                */
  EFFOCR_BEIT_EWORKSPACE = -3,    /* caller-provided workspace / weight buffer too small                 */
  EFFOCR_BEIT_EHIP = -4,          /* HIP runtime error                                                   */
  EFFOCR_BEIT_ESTATE = -5,        /* call order violated (forward before upload, a parameter never set)  */
  EFFOCR_BEIT_EOVERFLOW = -6      /* non-finite embedding (f16 operand overflow or non-finite input)     */
};

typedef struct effocr_beit effocr_beit_t;

int effocr_beit_abi_version(void);
const char* effocr_beit_last_error(void);

/* arch: "beit_base_patch16_224" or "beitv2_base_patch16_224" (width 768, depth 12, 12 heads), or the test
 * miniature "beit_tiny_test" (width 128, depth 2, 2 heads); anything else is EFFOCR_BEIT_EUNSUPPORTED.
 * img_size: a multiple of 16 from 16 to 224 (EFFOCR_BEIT_EINVAL otherwise); a crop is (img_size/16)^2 + 1
 * tokens, and the bias tables have (2 img_size/16 - 1)^2 + 3 rows.  precision = EFFOCR_PREC_BF16 (0),
 * EFFOCR_PREC_FP16 (1) or EFFOCR_PREC_FP32 (2) of effocr_hip.h — the type of the linears' and the attention
 * MFMAs' operands (the residual stream, LayerNorm, softmax, bias add, layer scale and the embedding are fp32
 * in every mode). */
int effocr_beit_create(const char* arch, int img_size, int precision, effocr_beit_t** out);
void effocr_beit_destroy(effocr_beit_t* enc);
int effocr_beit_embed_dim(const effocr_beit_t* enc);                  /* 768 (128 for beit_tiny_test) */

int effocr_beit_num_params(const effocr_beit_t* enc);
const char* effocr_beit_param_name(const effocr_beit_t* enc, int i);  /* NULL when i is out of range */
int64_t effocr_beit_param_numel(const effocr_beit_t* enc, int i);     /* -1 when i is out of range */
/* host fp32 copy of one parameter (timm's layout and shape, numel must match) */
int effocr_beit_set_param(effocr_beit_t* enc, const char* name, const float* host, int64_t numel);
size_t effocr_beit_weights_bytes(const effocr_beit_t* enc);
/* packs every parameter into the device blob weights_dev (>= effocr_beit_weights_bytes; synchronous copy) */
int effocr_beit_upload(effocr_beit_t* enc, void* weights_dev, size_t bytes);

/* Device workspace a forward of `batch` crops needs (0 for batch <= 0).  Calls run in sub-batches of
 * effocr_beit_set_chunk crops (0 = the default: the largest sub-batch whose workspace stays under
 * 1 GB, at most 256 crops), so this stops growing at the sub-batch size.  The first 256 bytes hold the
 * sticky status word; zero them once in a fresh workspace. */
size_t effocr_beit_workspace_bytes(const effocr_beit_t* enc, int batch);
int effocr_beit_set_chunk(effocr_beit_t* enc, int crops_per_chunk);

/* x_dev [batch,3,img_size,img_size] fp32 (NCHW, ImageNet-normalised crops) -> emb_dev [batch,D] fp32:
 * fc_norm(mean of the patch tokens), L2-normalised (F.normalize) when l2_normalize != 0.  A crop's
 * embedding is bitwise independent of `batch` and of the chunk setting.  A non-finite embedding ORs 1
 * into the workspace's status word. */
int effocr_beit_forward(effocr_beit_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize,
                        void* workspace_dev, size_t workspace_bytes, void* stream);

/* Reads and clears the status word (synchronises `stream`): EFFOCR_BEIT_EOVERFLOW if any forward on this
 * workspace since the last check produced a non-finite embedding, else 0. */
int effocr_beit_check_status(const effocr_beit_t* enc, const void* workspace_dev, void* stream);
/* Clears the status word without reading it (asynchronous on `stream`). */
int effocr_beit_reset_status(const effocr_beit_t* enc, void* workspace_dev, void* stream);

/* Test entry point (no product code calls it): the bias-attention kernel alone on caller-made tensors.
 * qkv_dev [batch*T][3*heads*64] (q | k | v) and out_dev [batch*T][heads*64] in `dtype`'s element type
 * (EFFOCR_PREC_*), T = patches_per_side^2 + 1, 1 <= patches_per_side <= 14; table_dev
 * [(2 patches_per_side - 1)^2 + 3][heads] fp32. */
int effocr_beit_op_attn(const void* qkv_dev, const float* table_dev, int batch, int patches_per_side, int heads, int dtype,
                        void* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFOCR_BEIT_H */
