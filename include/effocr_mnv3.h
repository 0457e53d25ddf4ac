/* effocr_mnv3.h — C ABI of libeffocr_mnv3.so: the MobileNetV3 recognizer encoders mobilenetv3_small_075,
 * mobilenetv3_small_100 and mobilenetv3_large_100 (timm.create_model(name, num_classes=0), what the
 * reference builds for `--auto_model_timm <name>`) on the MI355X (gfx950).
 *
 * A library of its own: libeffocr_hip.so is at its size cap (DESIGN.md "Library split") and is not touched;
 * its effocr_encoder_create keeps serving mobilenetv3_small_050 (every activation of a crop in LDS) and keeps
 * refusing the names above.  Here the activations live in HBM between blocks (fp32, channels-last), which is
 * what the wider expansions need.  The library derives the block list from the architecture name (timm's
 * Small and Large arch definitions, multipliers 0.5 / 0.75 / 1.0, make_divisible with round limit 0.9, the
 * fixed 16-channel stem below 0.75, the squeeze-excite width from the expansion), so it accepts
 * mobilenetv3_small_050 too: the package never sends it here, a test does, to compare two independent
 * implementations of one network.  mobilenetv3_large_075 and every other name are refused
 * (EFFOCR_MNV3_EUNSUPPORTED).  Conventions are those of effocr_hip.h:
 *   - every *_dev pointer is caller-owned DEVICE memory; the library allocates no device memory;
 *   - calls that take a `stream` are asynchronous on it (hipStream_t passed as void*; NULL = the
 *     default stream);
 *   - 0 on success, a negative EFFOCR_MNV3_E* code on failure (the same values as effocr_hip.h's
 *     EFFOCR_E* codes), the message from effocr_mnv3_last_error() (thread-local).
 *
 * The handle mirrors the encoder handle of effocr_hip.h: create -> set_param x N -> upload -> forward ...;
 * parameter names are timm's state-dict keys (conv_stem, bn1,
 * blocks.i.j.{conv_pw,bn1,conv_dw,bn2,se.conv_reduce,se.conv_expand,conv_pwl,bn3}, blocks.N.0.{conv,bn1},
 * conv_head) WITHOUT the "net." prefix, without `classifier` and without `num_batches_tracked`.  timm is not
 * a dependency of this project and is not installed where it is developed: the key names were checked
 * against no timm install; the block tables are pinned by timm's published parameter counts.
 */
#ifndef EFFOCR_MNV3_H
#define EFFOCR_MNV3_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an exported signature or the meaning of an argument changes; effocr_amd/_lib.py
 * refuses a library whose effocr_mnv3_abi_version() differs */
#define EFFOCR_MNV3_ABI_VERSION 1

enum effocr_mnv3_status {
  EFFOCR_MNV3_OK = 0,
  EFFOCR_MNV3_EINVAL = -1,        /* bad argument (NULL pointer, unknown precision, wrong numel, bad img_size)          */
  EFFOCR_MNV3_EUNSUPPORTED = -2,  /* valid request outside what the kernels implement (another architecture)          */
  EFFOCR_MNV3_EWORKSPACE = -3,    /* caller-provided workspace / weight buffer too small                               */
  EFFOCR_MNV3_EHIP = -4,          /* HIP runtime error                                                                 */
  EFFOCR_MNV3_ESTATE = -5,        /* call order violated (forward before upload, a parameter never set)                */
  EFFOCR_MNV3_EOVERFLOW = -6      /* non-finite embedding (f16 operand overflow or non-finite input / weights)         */
};

typedef struct effocr_mnv3 effocr_mnv3_t;

int effocr_mnv3_abi_version(void);
const char* effocr_mnv3_last_error(void);

/* arch = "mobilenetv3_small_050" | "mobilenetv3_small_075" | "mobilenetv3_small_100" | "mobilenetv3_large_100";
 * img_size a multiple of 32 in [32, 224]; precision = EFFOCR_PREC_BF16 (0), EFFOCR_PREC_FP16 (1) or
 * EFFOCR_PREC_FP32 (2) of effocr_hip.h — the type of the 1x1 convolutions' WEIGHTS.  Activations are fp32 in
 * every mode (they enter the 16-bit MFMAs as a high part plus the rounding of the remainder); the stem, the
 * depthwise convolutions, squeeze-excite, biases and residual adds are fp32 in every mode. */
int effocr_mnv3_create(const char* arch, int img_size, int precision, effocr_mnv3_t** out);
void effocr_mnv3_destroy(effocr_mnv3_t* enc);
int effocr_mnv3_embed_dim(const effocr_mnv3_t* enc);                  /* 1024 (Small) or 1280 (Large) */

int effocr_mnv3_num_params(const effocr_mnv3_t* enc);
const char* effocr_mnv3_param_name(const effocr_mnv3_t* enc, int i);  /* NULL when i is out of range; timm's state-dict order */
int64_t effocr_mnv3_param_numel(const effocr_mnv3_t* enc, int i);     /* -1 when i is out of range */
/* host fp32 copy of one parameter (torch's layout and shape, numel must match) */
int effocr_mnv3_set_param(effocr_mnv3_t* enc, const char* name, const float* host, int64_t numel);
size_t effocr_mnv3_weights_bytes(const effocr_mnv3_t* enc);
/* folds every BatchNorm into its convolution (fp32) and packs the device blob weights_dev (>= effocr_mnv3_weights_bytes; synchronous copy) */
int effocr_mnv3_upload(effocr_mnv3_t* enc, void* weights_dev, size_t bytes);

/* Device workspace a forward of `batch` crops needs (0 for batch <= 0).  Calls run in sub-batches of
 * effocr_mnv3_set_chunk crops (0 = the default: the largest sub-batch whose workspace stays under
 * 512 MiB, at most 256 crops), so this stops growing at the sub-batch size.  The first 256 bytes hold the
 * sticky status word; zero them once in a fresh workspace. */
size_t effocr_mnv3_workspace_bytes(const effocr_mnv3_t* enc, int batch);
int effocr_mnv3_set_chunk(effocr_mnv3_t* enc, int crops_per_chunk);

/* x_dev [batch,3,img,img] fp32 (NCHW, ImageNet-normalised crops) -> emb_dev [batch,D] fp32: conv_head +
 * hard-swish of the globally average-pooled features, L2-normalised (F.normalize) when l2_normalize != 0.
 * A crop's embedding is bitwise independent of `batch` and of the chunk setting.  A non-finite embedding
 * ORs 1 into the workspace's status word. */
int effocr_mnv3_forward(effocr_mnv3_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize,
                        void* workspace_dev, size_t workspace_bytes, void* stream);

/* Reads and clears the status word (synchronises `stream`): EFFOCR_MNV3_EOVERFLOW if any forward on this
 * workspace since the last check produced a non-finite embedding, else 0. */
int effocr_mnv3_check_status(const effocr_mnv3_t* enc, const void* workspace_dev, void* stream);

/* TEST ENTRY POINTS: the six kernels of the forward, one launch each, on caller-made DEVICE tensors (tests/test_gpu_mobilenetv3_ops.py
 * compares each with a float64 restatement).  All tensors fp32 and channels-last unless stated; act = 0 none, 1 ReLU, 2 hard-swish,
 * 3 SiLU.  Every argument is checked before the launch: a NULL pointer or a non-positive size is EFFOCR_MNV3_EINVAL, a geometry the
 * kernel does not implement EFFOCR_MNV3_EUNSUPPORTED.  No product code calls them.
 *   op_stem     x [batch,3,S,S] NCHW (S even) -> out [batch,S/2,S/2,16] = hardswish(conv3x3/2 pad 1 + b); w [27][16], row (ci*3+ky)*3+kx
 *   op_dw       in [batch,H,H,C] -> out [batch,Ho,Ho,C] = act(depthwise k x k, pad k/2 + b), Ho = (H-1)/stride+1; w [k*k][C], row ky*k+kx;
 *               C % 4 == 0, k 3 or 5, stride 1 or 2
 *   op_se_gate  t [batch,pixels,C] -> gate [batch,C] = hardsigmoid(expand_w . relu(reduce_w . mean(t) + reduce_b) + expand_b);
 *               reduce_w [R][C], expand_w [C][R]; C <= 1024, R <= 256
 *   op_pw       out [rows,N] = act((a [rows,K] * gate[row / pixels_per_crop][k]) . w^T + bias) (+ resid [rows,N]); gate [crops,K] and resid
 *               may be NULL; K % 4 == 0, N % 4 == 0.  w as the forward reads it: precision 2 (fp32): [N][K] fp32; 0 / 1 (bf16 / f16):
 *               [16 ceil(N/16)][Kp] of that type, Kp = K rounded up to 16, zero padded
 *   op_pool     t [batch,pixels,C] -> out [batch,C], the mean over the pixels
 *   op_finish   emb [batch,D] in place: F.normalize when l2_normalize != 0; ORs 1 into *status_dev (int32) if a value read was non-finite */
int effocr_mnv3_op_stem(const float* x_dev, int batch, int img_size, const float* w_dev, const float* b_dev, float* out_dev, void* stream);
int effocr_mnv3_op_dw(const float* in_dev, int batch, int in_size, int channels, int kernel, int stride, const float* w_dev,
                      const float* b_dev, int act, float* out_dev, void* stream);
int effocr_mnv3_op_se_gate(const float* t_dev, int batch, int pixels, int channels, int se_width, const float* reduce_w_dev,
                           const float* reduce_b_dev, const float* expand_w_dev, const float* expand_b_dev, float* gate_dev, void* stream);
int effocr_mnv3_op_pw(int precision, const float* a_dev, int64_t rows, int k, const void* w_dev, int n, const float* bias_dev,
                      const float* gate_dev, int pixels_per_crop, int act, const float* resid_dev, float* out_dev, void* stream);
int effocr_mnv3_op_pool(const float* t_dev, int batch, int pixels, int channels, float* out_dev, void* stream);
int effocr_mnv3_op_finish(float* emb_dev, int batch, int dim, int l2_normalize, int* status_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFOCR_MNV3_H */
