/* effocr_resnet.h — C ABI of libeffocr_resnet.so: the ResNet-34 and ResNet-50 recognizer encoders
 * (timm.create_model("resnet34" | "resnet50", num_classes=0), what the reference builds for
 * `--auto_model_timm resnet34` / `resnet50`) on the MI355X (gfx950).
 *
 * A library of its own: libeffocr_hip.so is at its size cap (DESIGN.md "Library split"), so this one
 * neither links against it nor shares its error state; the exact-fp32 convolution pipeline of the
 * resnet18 path (resnet.hip) is compiled into it a second time with hidden visibility for the fp32
 * mode.  resnet18 stays on effocr_encoder_create (effocr_hip.h).  Conventions are those of effocr_hip.h:
 *   - every *_dev pointer is caller-owned DEVICE memory; the library allocates no device memory;
 *   - calls that take a `stream` are asynchronous on it (hipStream_t passed as void*; NULL = the
 *     default stream);
 *   - 0 on success, a negative EFFOCR_RESNET_E* code on failure (the same values as effocr_hip.h's
 *     EFFOCR_E* codes), the message from effocr_resnet_last_error() (thread-local).
 *
 * The handle mirrors the encoder handle of effocr_hip.h: create -> set_param x N -> upload ->
 * forward ...; parameter names are timm's / torchvision's state-dict keys (conv1, bn1,
 * layerN.M.{conv1,bn1,conv2,bn2[,conv3,bn3]}, layerN.0.downsample.{0,1}) WITHOUT the "net." prefix,
 * without the classifier `fc` and without `num_batches_tracked`.
 */
#ifndef EFFOCR_RESNET_H
#define EFFOCR_RESNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an exported signature or the meaning of an argument changes; effocr_amd/_lib.py
 * refuses a library whose effocr_resnet_abi_version() differs */
#define EFFOCR_RESNET_ABI_VERSION 1

enum effocr_resnet_status {
  EFFOCR_RESNET_OK = 0,
  EFFOCR_RESNET_EINVAL = -1,        /* bad argument (NULL pointer, unknown name or precision, wrong numel, bad img_size) */
  EFFOCR_RESNET_EUNSUPPORTED = -2,  /* valid request outside what the kernels implement (another architecture)          */
  EFFOCR_RESNET_EWORKSPACE = -3,    /* caller-provided workspace / weight buffer too small                               */
  EFFOCR_RESNET_EHIP = -4,          /* HIP runtime error                                                                 */
  EFFOCR_RESNET_ESTATE = -5,        /* call order violated (forward before upload, a parameter never set)                */
  EFFOCR_RESNET_EOVERFLOW = -6      /* non-finite embedding (f16 activation overflow or non-finite input)                */
};

typedef struct effocr_resnet effocr_resnet_t;

int effocr_resnet_abi_version(void);
const char* effocr_resnet_last_error(void);

/* arch = "resnet34" or "resnet50"; img_size a positive multiple of 32; precision = EFFOCR_PREC_BF16 (0),
 * EFFOCR_PREC_FP16 (1) or EFFOCR_PREC_FP32 (2) of effocr_hip.h — the type of the convolutions' operands
 * AND of the activations stored between layers (accumulation, bias and the pooled embedding are fp32 in
 * every mode). */
int effocr_resnet_create(const char* arch, int img_size, int precision, effocr_resnet_t** out);
void effocr_resnet_destroy(effocr_resnet_t* enc);
int effocr_resnet_embed_dim(const effocr_resnet_t* enc);              /* 512 (resnet34) or 2048 (resnet50) */

int effocr_resnet_num_params(const effocr_resnet_t* enc);
const char* effocr_resnet_param_name(const effocr_resnet_t* enc, int i);  /* NULL when i is out of range */
int64_t effocr_resnet_param_numel(const effocr_resnet_t* enc, int i);     /* -1 when i is out of range */
/* host fp32 copy of one parameter (torch's layout and shape, numel must match) */
int effocr_resnet_set_param(effocr_resnet_t* enc, const char* name, const float* host, int64_t numel);
size_t effocr_resnet_weights_bytes(const effocr_resnet_t* enc);
/* folds every BatchNorm into its convolution and packs the device blob weights_dev (>= effocr_resnet_weights_bytes; synchronous copy) */
int effocr_resnet_upload(effocr_resnet_t* enc, void* weights_dev, size_t bytes);

/* Device workspace a forward of `batch` crops needs (0 for batch <= 0).  Calls run in sub-batches of
 * effocr_resnet_set_chunk crops (0 = the default: the largest sub-batch whose workspace stays under
 * 1 GB, at most 256 crops), so this stops growing at the sub-batch size.  The first 256 bytes hold the
 * sticky status word; zero them once in a fresh workspace. */
size_t effocr_resnet_workspace_bytes(const effocr_resnet_t* enc, int batch);
int effocr_resnet_set_chunk(effocr_resnet_t* enc, int crops_per_chunk);

/* x_dev [batch,3,img,img] fp32 (NCHW, ImageNet-normalised crops) -> emb_dev [batch,D] fp32 globally
 * average-pooled features, L2-normalised (F.normalize) when l2_normalize != 0.  A crop's embedding is
 * bitwise independent of `batch` and of the chunk setting.  A non-finite embedding ORs 1 into the
 * workspace's status word. */
int effocr_resnet_forward(effocr_resnet_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize,
                          void* workspace_dev, size_t workspace_bytes, void* stream);

/* Reads and clears the status word (synchronises `stream`): EFFOCR_RESNET_EOVERFLOW if any forward on this
 * workspace since the last check produced a non-finite embedding, else 0. */
int effocr_resnet_check_status(const effocr_resnet_t* enc, const void* workspace_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFOCR_RESNET_H */
