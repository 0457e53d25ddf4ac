/* effocr_effnet.h — C ABI of libeffocr_effnet.so: the EfficientNet-B0 recognizer encoders efficientnet_b0 and
 * tf_efficientnet_b0 (timm.create_model(name, num_classes=0), what the reference builds for
 * `--auto_model_timm <name>`) on the MI355X (gfx950).
 *
 * A library of its own: libeffocr_hip.so is at its size cap (DESIGN.md "Library split") and libeffocr_mnv3.so
 * keeps its forward as it is; both go on refusing these names.  The activations live in HBM between launches
 * (fp32, channels-last), as in libeffocr_mnv3.so, whose pointwise GEMM, pool and normalisation kernels are
 * compiled into this library a second time (hidden).  The library derives the block list from the
 * architecture name (timm's _gen_efficientnet at multipliers 1.0 / 1.0: a 32-channel stem, one
 * DepthwiseSeparable and fifteen InvertedResidual blocks, squeeze-excite in all sixteen with the width
 * round(0.25 x the block's INPUT channels), SiLU everywhere, conv_head 320 -> 1280 + bn2 + SiLU BEFORE the
 * global average pool).  The two names share keys and shapes and differ in the BatchNorm eps (1e-5 / 1e-3)
 * and in the padding: efficientnet_b0 pads k/2 on both sides, tf_efficientnet_b0 as TensorFlow's SAME does
 * (stride-2 convolutions on the even maps that occur: 0 before / 1 after for k = 3, 1 before / 2 after for
 * k = 5).  Every other name — efficientnet_b1..b7, efficientnet_lite*, efficientnetv2_*, the _ns / _ap
 * weight tags, the MobileNetV3s — is refused (EFFOCR_EFFNET_EUNSUPPORTED).  Conventions are those of
 * effocr_hip.h:
 *   - every *_dev pointer is caller-owned DEVICE memory; the library allocates no device memory;
 *   - calls that take a `stream` are asynchronous on it (hipStream_t passed as void*; NULL = the
 *     default stream);
 *   - 0 on success, a negative EFFOCR_EFFNET_E* code on failure (the same values as effocr_hip.h's
 *     EFFOCR_E* codes), the message from effocr_effnet_last_error() (thread-local).
 *
 * The handle mirrors effocr_mnv3.h: create -> set_param x N -> upload -> forward ...; parameter names are
 * timm's state-dict keys (conv_stem, bn1, blocks.0.0.{conv_dw,bn1,se.conv_reduce,se.conv_expand,conv_pw,bn2},
 * blocks.i.j.{conv_pw,bn1,conv_dw,bn2,se.conv_reduce,se.conv_expand,conv_pwl,bn3}, conv_head, bn2) WITHOUT
 * the "net." prefix, without `classifier` and without `num_batches_tracked`.  timm is not a dependency of
 * this project and is not installed where it is developed: the key names were checked against no timm
 * install (UNVERIFIED); the architecture is pinned against transformers.EfficientNetModel, which holds the
 * same network under other names (tests/test_efficientnet_host.py).
 */
#ifndef EFFOCR_EFFNET_H
#define EFFOCR_EFFNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an exported signature or the meaning of an argument changes; effocr_amd/_lib.py
 * refuses a library whose effocr_effnet_abi_version() differs */
#define EFFOCR_EFFNET_ABI_VERSION 1

enum effocr_effnet_status {
  EFFOCR_EFFNET_OK = 0,
  EFFOCR_EFFNET_EINVAL = -1,        /* bad argument (NULL pointer, unknown precision, wrong numel, bad img_size)        */
  EFFOCR_EFFNET_EUNSUPPORTED = -2,  /* valid request outside what the kernels implement (another architecture, 16-bit crops) */
  EFFOCR_EFFNET_EWORKSPACE = -3,    /* caller-provided workspace / weight buffer too small                             */
  EFFOCR_EFFNET_EHIP = -4,          /* HIP runtime error                                                               */
  EFFOCR_EFFNET_ESTATE = -5,        /* call order violated (forward before upload, a parameter never set)              */
  EFFOCR_EFFNET_EOVERFLOW = -6      /* non-finite embedding (f16 operand overflow or non-finite input / weights)       */
};

typedef struct effocr_effnet effocr_effnet_t;

int effocr_effnet_abi_version(void);
const char* effocr_effnet_last_error(void);

/* arch = "efficientnet_b0" | "tf_efficientnet_b0"; img_size a multiple of 32 in [32, 224]; precision =
 * EFFOCR_PREC_BF16 (0), EFFOCR_PREC_FP16 (1) or EFFOCR_PREC_FP32 (2) of effocr_hip.h — the type of the 1x1
 * convolutions' WEIGHTS (conv_head among them).  Activations are fp32 in every mode (they enter the 16-bit
 * MFMAs as a high part plus the rounding of the remainder); the stem, the depthwise convolutions,
 * squeeze-excite, biases and residual adds are fp32 in every mode. */
int effocr_effnet_create(const char* arch, int img_size, int precision, effocr_effnet_t** out);
void effocr_effnet_destroy(effocr_effnet_t* enc);
int effocr_effnet_embed_dim(const effocr_effnet_t* enc);                  /* 1280 */

int effocr_effnet_num_params(const effocr_effnet_t* enc);
const char* effocr_effnet_param_name(const effocr_effnet_t* enc, int i);  /* NULL when i is out of range; timm's state-dict order */
int64_t effocr_effnet_param_numel(const effocr_effnet_t* enc, int i);     /* -1 when i is out of range */
/* host fp32 copy of one parameter (torch's layout and shape, numel must match) */
int effocr_effnet_set_param(effocr_effnet_t* enc, const char* name, const float* host, int64_t numel);
size_t effocr_effnet_weights_bytes(const effocr_effnet_t* enc);
/* folds every BatchNorm into its convolution (fp32, the name's eps) and packs the device blob weights_dev
 * (>= effocr_effnet_weights_bytes; synchronous copy) */
int effocr_effnet_upload(effocr_effnet_t* enc, void* weights_dev, size_t bytes);

/* Device workspace a forward of `batch` crops needs (0 for batch <= 0).  Calls run in sub-batches of
 * effocr_effnet_set_chunk crops (0 = the default: the largest sub-batch whose workspace stays within
 * 512 MiB, at most 256 crops), so this stops growing at the sub-batch size.  The first 256 bytes hold the
 * sticky status word; zero them once in a fresh workspace. */
size_t effocr_effnet_workspace_bytes(const effocr_effnet_t* enc, int batch);
/* crops_per_chunk in [0, 65535]; anything else is EFFOCR_EFFNET_EINVAL */
int effocr_effnet_set_chunk(effocr_effnet_t* enc, int crops_per_chunk);

/* x_dev [batch,3,img,img] NCHW, ImageNet-normalised crops of type x_dtype, which must be EFFOCR_PREC_FP32
 * (the stem is an fp32 convolution in every mode; 16-bit crops: EFFOCR_EFFNET_EUNSUPPORTED) -> emb_dev
 * [batch,1280] fp32: the global average pool of SiLU(bn2(conv_head)), L2-normalised (F.normalize) when
 * l2_normalize != 0.  A crop's embedding is bitwise independent of `batch` and of the chunk setting.  A
 * non-finite embedding ORs 1 into the workspace's status word.  Every argument is checked, the workspace
 * size included, before the first launch. */
int effocr_effnet_forward(effocr_effnet_t* enc, const void* x_dev, int x_dtype, int batch, float* emb_dev, int l2_normalize,
                          void* workspace_dev, size_t workspace_bytes, void* stream);

/* Reads and clears the status word (synchronises `stream`): EFFOCR_EFFNET_EOVERFLOW if any forward on this
 * workspace since the last check or reset produced a non-finite embedding, else 0. */
int effocr_effnet_check_status(const effocr_effnet_t* enc, const void* workspace_dev, void* stream);
/* Clears the status word without reading it (asynchronous on `stream`). */
int effocr_effnet_reset_status(const effocr_effnet_t* enc, void* workspace_dev, void* stream);

/* TEST ENTRY POINT (tests/test_gpu_efficientnet.py; no product code calls it): the depthwise kernel and the
 * squeeze-excite gate kernel of the forward, on caller-made tensors.  in_dev [B,H,H,C] fp32 channels-last,
 * dw_w_dev [k*k][C] tap-major, dw_b_dev [C] -> dw_out_dev [B,Ho,Ho,C] (Ho = (H - 1) / stride + 1) =
 * SiLU(depthwise conv + bias) and part_dev [B][effocr_effnet_op_tiles(Ho)][C], the per-tile channel sums;
 * then gate_dev [B,C] = sigmoid(expand(SiLU(reduce(mean)))) from the tile sums alone, with se_reduce_w_dev
 * [R][C], se_expand_wt_dev [R][C] (conv_expand's weight transposed).  C % 4 == 0, C <= 1152, R <= 48. */
int effocr_effnet_op_tiles(int out_size);
/* TEST ENTRY POINT: the stem kernel of the forward.  x_dev [B,3,S,S] fp32 NCHW (S even), w_dev [27][32] tap-major ((ci, ky, kx) taps),
 * b_dev [32] -> out_dev [B,S/2,S/2,32] channels-last = SiLU(conv3x3/2 + bias); tap (ky, kx) reads input pixel
 * (2 oy + ky - pad_before, 2 ox + kx - pad_before): pad_before 1 = symmetric padding, 0 = TensorFlow SAME. */
int effocr_effnet_op_stem(const float* x_dev, int batch, int img_size, int pad_before, const float* w_dev, const float* b_dev,
                          float* out_dev, void* stream);
int effocr_effnet_op_dw_se(const float* in_dev, int batch, int in_size, int channels, int kernel, int stride, int pad_before,
                           const float* dw_w_dev, const float* dw_b_dev, int se_width, const float* se_reduce_w_dev,
                           const float* se_reduce_b_dev, const float* se_expand_wt_dev, const float* se_expand_b_dev,
                           float* dw_out_dev, float* part_dev, float* gate_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFOCR_EFFNET_H */
