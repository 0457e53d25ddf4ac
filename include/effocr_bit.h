/* effocr_bit.h — C ABI of libeffocr_bit.so: the Big Transfer (BiT) ResNetV2 recognizer encoders
 * (timm.create_model("resnetv2_50x1_bitm" | "resnetv2_101x1_bitm", num_classes=0), what the reference
 * builds for `--auto_model_timm resnetv2_50x1_bitm`; timm >= 0.9 names the same modules
 * resnetv2_50x1_bit / resnetv2_101x1_bit) on the MI355X (gfx950).
 *
 * A library of its own: libeffocr_hip.so is at its size cap (DESIGN.md "Library split"), so this one
 * neither links against it nor shares its error state; the convolution kernels of the ResNet paths
 * (resnet16.hip, resnet.hip) are compiled into it once more with hidden visibility.  Conventions are
 * those of effocr_hip.h:
 *   - every *_dev pointer is caller-owned DEVICE memory; the library allocates no device memory;
 *   - calls that take a `stream` are asynchronous on it (hipStream_t passed as void*; NULL = the
 *     default stream);
 *   - 0 on success, a negative EFFOCR_BIT_E* code on failure (the same values as effocr_hip.h's
 *     EFFOCR_E* codes), the message from effocr_bit_last_error() (thread-local).
 *
 * The network: a weight-standardised 7x7/2 stem convolution (no norm, no activation), a zero pad of 1
 * and a 3x3/2 max pool, four stages of pre-activation bottlenecks (GroupNorm(32) + ReLU before each of
 * the three weight-standardised convolutions, a 1x1 shortcut convolution on the first block's
 * pre-activation), a final GroupNorm(32) + ReLU and the global average pool.  No convolution has a bias.
 *
 * The handle mirrors the encoder handle of effocr_hip.h: create -> set_param x N -> upload ->
 * forward ...; parameter names are timm's state-dict keys (stem.conv.weight,
 * stages.I.blocks.J.{downsample.conv.weight,norm1,conv1,norm2,conv2,norm3,conv3}, norm) WITHOUT the
 * "net." prefix and without the classifier head.fc.
 */
#ifndef EFFOCR_BIT_H
#define EFFOCR_BIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an exported signature or the meaning of an argument changes; effocr_amd/_lib.py
 * refuses a library whose effocr_bit_abi_version() differs */
#define EFFOCR_BIT_ABI_VERSION 1

enum effocr_bit_status {
  EFFOCR_BIT_OK = 0,
  EFFOCR_BIT_EINVAL = -1,        /* bad argument (NULL pointer, unknown name or precision, wrong numel, bad img_size) */
  EFFOCR_BIT_EUNSUPPORTED = -2,  /* valid request outside what the kernels implement (another architecture)          */
  EFFOCR_BIT_EWORKSPACE = -3,    /* caller-provided workspace / weight buffer too small                               */
  EFFOCR_BIT_EHIP = -4,          /* HIP runtime error                                                                 */
  EFFOCR_BIT_ESTATE = -5,        /* call order violated (forward before upload, a parameter never set)                */
  EFFOCR_BIT_EOVERFLOW = -6      /* non-finite embedding (f16 activation overflow or non-finite input / weights)      */
};

typedef struct effocr_bit effocr_bit_t;

int effocr_bit_abi_version(void);
const char* effocr_bit_last_error(void);

/* arch = "resnetv2_50x1_bitm", "resnetv2_50x1_bit", "resnetv2_101x1_bitm" or "resnetv2_101x1_bit"; img_size a
 * positive multiple of 32; precision = EFFOCR_PREC_BF16 (0), EFFOCR_PREC_FP16 (1) or EFFOCR_PREC_FP32 (2)
 * of effocr_hip.h — the type of the convolutions' operands AND of the activations and the residual
 * stream stored between layers (accumulation, GroupNorm statistics and the head are fp32 in every mode). */
int effocr_bit_create(const char* arch, int img_size, int precision, effocr_bit_t** out);
void effocr_bit_destroy(effocr_bit_t* enc);
int effocr_bit_embed_dim(const effocr_bit_t* enc);                  /* 2048 */

int effocr_bit_num_params(const effocr_bit_t* enc);
const char* effocr_bit_param_name(const effocr_bit_t* enc, int i);  /* NULL when i is out of range */
int64_t effocr_bit_param_numel(const effocr_bit_t* enc, int i);     /* -1 when i is out of range */
/* host fp32 copy of one parameter (torch's layout and shape, numel must match) */
int effocr_bit_set_param(effocr_bit_t* enc, const char* name, const float* host, int64_t numel);
size_t effocr_bit_weights_bytes(const effocr_bit_t* enc);
/* standardises every convolution weight (per output channel, in double) and packs the device blob weights_dev
 * (>= effocr_bit_weights_bytes; synchronous copy) */
int effocr_bit_upload(effocr_bit_t* enc, void* weights_dev, size_t bytes);

/* Device workspace a forward of `batch` crops needs (0 for batch <= 0).  Calls run in sub-batches of
 * effocr_bit_set_chunk crops (0 = the default: the largest sub-batch whose workspace stays under
 * 1 GB, at most 256 crops), so this stops growing at the sub-batch size.  The first 256 bytes hold the
 * sticky status word; zero them once in a fresh workspace. */
size_t effocr_bit_workspace_bytes(const effocr_bit_t* enc, int batch);
int effocr_bit_set_chunk(effocr_bit_t* enc, int crops_per_chunk);

/* x_dev [batch,3,img,img] fp32 (NCHW, normalised crops) -> emb_dev [batch,2048] fp32 pooled features,
 * L2-normalised (F.normalize) when l2_normalize != 0.  A crop's embedding is bitwise independent of
 * `batch` and of the chunk setting.  A non-finite embedding ORs 1 into the workspace's status word. */
int effocr_bit_forward(effocr_bit_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize,
                       void* workspace_dev, size_t workspace_bytes, void* stream);

/* Reads and clears the status word (synchronises `stream`): EFFOCR_BIT_EOVERFLOW if any forward on this
 * workspace since the last check produced a non-finite embedding, else 0. */
int effocr_bit_check_status(const effocr_bit_t* enc, const void* workspace_dev, void* stream);
/* Clears the status word without reading it (asynchronous on `stream`). */
int effocr_bit_reset_status(const effocr_bit_t* enc, void* workspace_dev, void* stream);

/* ---- test entry points: one operator per call; no product code calls them.  dtype = a precision
 * code: the element type of x_dev / out_dev, NHWC.  GroupNorm has 32 groups and eps 1e-5. ---- */

/* out_dev [batch, hw, channels] = relu(GroupNorm(x_dev) * gamma_dev + beta_dev), statistics in fp32, rounded
 * once to dtype; out_dev may be x_dev.  channels a power of two from 64 to 2048.  scratch_dev: at least
 * batch * ceil(hw / max(1, 16384 / channels)) * 512 bytes. */
int effocr_bit_op_groupnorm_relu(int dtype, const void* x_dev, int batch, int hw, int channels, const float* gamma_dev,
                                 const float* beta_dev, void* out_dev, void* scratch_dev, size_t scratch_bytes, void* stream);
/* out_dev [batch, (h-1)/2+1, (w-1)/2+1, channels] = max_pool2d(pad(x_dev [batch,h,w,channels], 1, value 0), 3, 2);
 * channels a multiple of 8 */
int effocr_bit_op_stem_pool(int dtype, const void* x_dev, int batch, int h, int w, int channels, void* out_dev, void* stream);
/* emb_dev [batch, channels] fp32 = mean over hw of relu(GroupNorm(x_dev) * gamma_dev + beta_dev) in fp32,
 * L2-normalised when l2_normalize != 0; ORs 1 into *status_dev (may be NULL) on a non-finite embedding.
 * channels a multiple of 256, at most 2048. */
int effocr_bit_op_head(int dtype, const void* x_dev, int batch, int hw, int channels, const float* gamma_dev, const float* beta_dev,
                       int l2_normalize, float* emb_dev, int* status_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFOCR_BIT_H */
