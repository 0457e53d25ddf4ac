/* effocr_swin.h — C ABI of libeffocr_swin.so: the Swin-T recognizer encoder
 * (timm.create_model("swin_tiny_patch4_window7_224", num_classes=0), what the reference builds for
 * `--auto_model_timm swin_tiny_patch4_window7_224` in train_effocr_recognizer.py / infer_effocr.py)
 * on the MI355X (gfx950).
 *
 * A library of its own: libeffocr_hip.so is at its size cap (DESIGN.md "Library split"), so this one
 * neither links against it nor shares its error state; the GEMMs it needs are compiled into it a
 * second time with hidden visibility.  Conventions are those of effocr_hip.h:
 *   - every *_dev pointer is caller-owned DEVICE memory; the library allocates no device memory;
 *   - calls that take a `stream` are asynchronous on it (hipStream_t passed as void*; NULL = the
 *     default stream);
 *   - 0 on success, a negative EFFOCR_SWIN_E* code on failure (the same values as effocr_hip.h's
 *     EFFOCR_E* codes), the message from effocr_swin_last_error() (thread-local).
 *
 * The handle mirrors the encoder handle of effocr_hip.h: create -> set_param x N -> upload ->
 * forward ...; parameter names are timm's state-dict keys (timm >= 0.9 layout: the patch merging of
 * stage i > 0 is `layers.i.downsample`) WITHOUT the "net." prefix and without the classifier head.
 */
#ifndef EFFOCR_SWIN_H
#define EFFOCR_SWIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an exported signature or the meaning of an argument changes; effocr_amd/_lib.py
 * refuses a library whose effocr_swin_abi_version() differs */
#define EFFOCR_SWIN_ABI_VERSION 1

enum effocr_swin_status {
  EFFOCR_SWIN_OK = 0,
  EFFOCR_SWIN_EINVAL = -1,        /* bad argument (NULL pointer, unknown name or precision, wrong numel) */
  EFFOCR_SWIN_EUNSUPPORTED = -2,  /* valid request outside what the kernels implement (img_size != 224) */
  EFFOCR_SWIN_EWORKSPACE = -3,    /* caller-provided workspace / weight buffer too small                 */
  EFFOCR_SWIN_EHIP = -4,          /* HIP runtime error                                                   */
  EFFOCR_SWIN_ESTATE = -5,        /* call order violated (forward before upload, a parameter never set)  */
  EFFOCR_SWIN_EOVERFLOW = -6      /* non-finite embedding (f16 operand overflow or non-finite input)     */
};

typedef struct effocr_swin effocr_swin_t;

int effocr_swin_abi_version(void);
const char* effocr_swin_last_error(void);

/* arch must be "swin_tiny_patch4_window7_224"; img_size must be 224 (the reference never passes img_size
 * to timm: EFFOCR_SWIN_EUNSUPPORTED otherwise); precision = EFFOCR_PREC_BF16 (0), EFFOCR_PREC_FP16 (1) or
 * EFFOCR_PREC_FP32 (2) of effocr_hip.h — the type of the linears' operands (LayerNorm, softmax, biases,
 * the residual stream and the embedding are fp32 in every mode). */
int effocr_swin_create(const char* arch, int img_size, int precision, effocr_swin_t** out);
void effocr_swin_destroy(effocr_swin_t* enc);
int effocr_swin_embed_dim(const effocr_swin_t* enc);                  /* 768 */

int effocr_swin_num_params(const effocr_swin_t* enc);
const char* effocr_swin_param_name(const effocr_swin_t* enc, int i);  /* NULL when i is out of range */
int64_t effocr_swin_param_numel(const effocr_swin_t* enc, int i);     /* -1 when i is out of range */
/* host fp32 copy of one parameter (timm's layout and shape, numel must match) */
int effocr_swin_set_param(effocr_swin_t* enc, const char* name, const float* host, int64_t numel);
size_t effocr_swin_weights_bytes(const effocr_swin_t* enc);
/* packs every parameter into the device blob weights_dev (>= effocr_swin_weights_bytes; synchronous copy) */
int effocr_swin_upload(effocr_swin_t* enc, void* weights_dev, size_t bytes);

/* Device workspace a forward of `batch` crops needs (0 for batch <= 0).  Calls run in sub-batches of
 * effocr_swin_set_chunk crops (0 = the default: the largest sub-batch whose workspace stays under
 * 1 GB, at most 192 crops), so this stops growing at the sub-batch size.  The first 256 bytes hold the
 * sticky status word; zero them once in a fresh workspace. */
size_t effocr_swin_workspace_bytes(const effocr_swin_t* enc, int batch);
int effocr_swin_set_chunk(effocr_swin_t* enc, int crops_per_chunk);

/* x_dev [batch,3,224,224] fp32 (NCHW, ImageNet-normalised crops) -> emb_dev [batch,768] fp32 pooled
 * features, L2-normalised (F.normalize) when l2_normalize != 0.  A crop's embedding is bitwise
 * independent of `batch` and of the chunk setting.  A non-finite embedding ORs 1 into the workspace's
 * status word. */
int effocr_swin_forward(effocr_swin_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize,
                        void* workspace_dev, size_t workspace_bytes, void* stream);

/* Reads and clears the status word (synchronises `stream`): EFFOCR_SWIN_EOVERFLOW if any forward on this
 * workspace since the last check produced a non-finite embedding, else 0. */
int effocr_swin_check_status(const effocr_swin_t* enc, const void* workspace_dev, void* stream);

/* ---- test entry points (tests/test_gpu_swin_ops.py) ------------------------------------------------------
 * One kernel launch each, on caller-made device tensors in the kernels' own layouts, so that the tests can
 * run every kernel and linear of the forward at shapes the 224 x 224 forward never reaches.  NULL pointers
 * and non-positive sizes give EFFOCR_SWIN_EINVAL, a geometry the launcher does not implement
 * EFFOCR_SWIN_EUNSUPPORTED, both before anything is launched.  LayerNorm eps is the forward's (1e-5).
 * `precision` is the operand type of the linears as in effocr_swin_create; activations with
 * `padded_channels` > `channels` hold pad channels that are never read on input and written as 0 on output. */
/* x [batch,3,img_size,img_size] fp32; w [48 taps (c, ky, kx)][128], b / lnw / lnb [128] fp32 (zero beyond
 * `channels`) -> out [batch * (img_size/4)^2][128] fp32: 4x4/s4 conv + bias + LayerNorm over `channels` */
int effocr_swin_op_stem(const float* x_dev, int batch, int img_size, const float* w_dev, const float* b_dev,
                        const float* lnw_dev, const float* lnb_dev, int channels, float* out_dev, void* stream);
/* x [rows][padded_channels] fp32 -> out [rows][padded_channels] in precision's type */
int effocr_swin_op_layernorm(int precision, const float* x_dev, int64_t rows, int channels, int padded_channels,
                             const float* lnw_dev, const float* lnb_dev, void* out_dev, void* stream);
/* patch merging: x [batch][map_size][map_size][padded_channels] fp32, lnw / lnb [4 channels] ->
 * out [batch * (map_size/2)^2][4 channels] in precision's type (2x2 gather in timm's order + LayerNorm) */
int effocr_swin_op_merge(int precision, const float* x_dev, int batch, int map_size, int channels, int padded_channels,
                         const float* lnw_dev, const float* lnb_dev, void* out_dev, void* stream);
/* qkv [batch * map_size^2][3][padded_channels] and out [batch * map_size^2][padded_channels] in precision's
 * type; table [169][channels / 32] fp32; shift: the cyclic shift of SW-MSA (0 = W-MSA) */
int effocr_swin_op_window_attention(int precision, const void* qkv_dev, int batch, int map_size, int channels,
                                    int padded_channels, int shift, const float* table_dev, void* out_dev, void* stream);
/* x [batch][tokens][padded_channels] fp32 -> emb [batch][channels] fp32 (LayerNorm, mean over the tokens,
 * F.normalize when l2_normalize != 0); a non-finite embedding ORs 1 into status_dev[0] */
int effocr_swin_op_head(const float* x_dev, int batch, int tokens, int channels, int padded_channels, const float* lnw_dev,
                        const float* lnb_dev, int l2_normalize, float* emb_dev, int* status_dev, void* stream);
/* out [rows][n] = epilogue(x [rows][k] . w [n][k]^T + bias [n]) through the forward's own dispatch; x and w in
 * precision's type, bias fp32.  epilogue: 0 bias, 1 bias + GELU (both: out in precision's type), 2 bias +
 * fp32 residual resid [rows][n] -> fp32 out (resid_dev may equal out_dev), 5 bias -> fp32 out. */
int effocr_swin_op_linear(int precision, int epilogue, const void* x_dev, const void* w_dev, const float* bias_dev,
                          const float* resid_dev, void* out_dev, int64_t rows, int n, int k, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFOCR_SWIN_H */
