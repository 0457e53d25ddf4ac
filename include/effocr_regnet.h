/* effocr_regnet.h — C ABI of libeffocr_regnet.so: the RegNetX / RegNetY recognizer encoders regnetx_002,
 * regnetx_004, regnetx_006, regnetx_008, regnetx_016, regnety_002, regnety_004, regnety_006, regnety_008 and
 * regnety_016 (timm.create_model(name, num_classes=0), what the reference builds for
 * `--auto_model_timm <name>`) on the MI355X (gfx950).
 *
 * A library of its own, as every encoder family since Swin (DESIGN.md "Library split").  The activations live
 * in HBM between launches (fp32, channels-last), as in libeffocr_mnv3.so, whose pointwise GEMM, pool and
 * normalisation kernels are compiled into this library a second time (hidden); its own kernels are the
 * grouped 3x3 convolution (group width 8, 16 or 24), the squeeze-excite gate of RegNetY, the 32-channel
 * ReLU stem, the row gather of the strided shortcut and the ReLU behind the residual add.  The library derives
 * the block list from the architecture name: a 3x3/2 stem to 32 channels, four stages s1..s4 whose first
 * block has stride 2, every block conv1 (1x1, BN, ReLU) -> conv2 (grouped 3x3, the stride, BN, ReLU) ->
 * [RegNetY: squeeze-excite, reduced width round(0.25 x the block's INPUT width), ReLU / sigmoid] -> conv3
 * (1x1, BN) -> + shortcut (1x1 with the stride + BN in a stage's first block, else the identity) -> ReLU;
 * the embedding is the global average pool of the last block.  regnetx_032 and wider, regnety_032 and wider,
 * regnetz_* and regnetv_* are refused (EFFOCR_REGNET_EUNSUPPORTED).  Conventions are those of effocr_hip.h:
 *   - every *_dev pointer is caller-owned DEVICE memory; the library allocates no device memory;
 *   - calls that take a `stream` are asynchronous on it (hipStream_t passed as void*; NULL = the
 *     default stream);
 *   - 0 on success, a negative EFFOCR_REGNET_E* code on failure (the same values as effocr_hip.h's
 *     EFFOCR_E* codes), the message from effocr_regnet_last_error() (thread-local).
 *
 * The handle mirrors effocr_effnet.h: create -> set_param x N -> upload -> forward ...; parameter names are
 * timm's state-dict keys (stem.{conv,bn}, sI.bJ.{conv1,conv2,conv3,downsample}.{conv,bn}, sI.bJ.se.{fc1,fc2})
 * WITHOUT the "net." prefix, without `head.fc` and without `num_batches_tracked`.  timm is not a dependency
 * of this project and is not installed where it is developed: the key names were checked against no timm
 * install (UNVERIFIED); the architecture is pinned against transformers.RegNetModel, which holds the same
 * network under other names (tests/test_regnet_host.py), and the parameter counts equal timm's published ones.
 */
#ifndef EFFOCR_REGNET_H
#define EFFOCR_REGNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an exported signature or the meaning of an argument changes; effocr_amd/_lib.py
 * refuses a library whose effocr_regnet_abi_version() differs */
#define EFFOCR_REGNET_ABI_VERSION 1

enum effocr_regnet_status {
  EFFOCR_REGNET_OK = 0,
  EFFOCR_REGNET_EINVAL = -1,        /* bad argument (NULL pointer, unknown precision, wrong numel, bad img_size)        */
  EFFOCR_REGNET_EUNSUPPORTED = -2,  /* valid request outside what the kernels implement (another architecture, 16-bit crops) */
  EFFOCR_REGNET_EWORKSPACE = -3,    /* caller-provided workspace / weight buffer too small                             */
  EFFOCR_REGNET_EHIP = -4,          /* HIP runtime error                                                               */
  EFFOCR_REGNET_ESTATE = -5,        /* call order violated (forward before upload, a parameter never set)              */
  EFFOCR_REGNET_EOVERFLOW = -6      /* non-finite embedding (f16 operand overflow or non-finite input / weights)       */
};

typedef struct effocr_regnet effocr_regnet_t;

int effocr_regnet_abi_version(void);
const char* effocr_regnet_last_error(void);

/* arch = one of the ten names above (or a miniature used by the tests: regnetx_mini8_test, regnetx_mini16_test,
 * regnety_mini24_test); img_size a positive multiple of 32; precision = EFFOCR_PREC_BF16 (0), EFFOCR_PREC_FP16
 * (1) or EFFOCR_PREC_FP32 (2) of effocr_hip.h — the type of the convolutions' WEIGHTS (1x1 and grouped 3x3).
 * Activations are fp32 in every mode (they enter the 16-bit MFMAs as a high part plus the rounding of the
 * remainder); the stem, squeeze-excite, biases and residual adds are fp32 in every mode. */
int effocr_regnet_create(const char* arch, int img_size, int precision, effocr_regnet_t** out);
void effocr_regnet_destroy(effocr_regnet_t* enc);
int effocr_regnet_embed_dim(const effocr_regnet_t* enc);                  /* the last stage's width */

int effocr_regnet_num_params(const effocr_regnet_t* enc);
const char* effocr_regnet_param_name(const effocr_regnet_t* enc, int i);  /* NULL when i is out of range; timm's state-dict order */
int64_t effocr_regnet_param_numel(const effocr_regnet_t* enc, int i);     /* -1 when i is out of range */
/* host fp32 copy of one parameter (torch's layout and shape, numel must match) */
int effocr_regnet_set_param(effocr_regnet_t* enc, const char* name, const float* host, int64_t numel);
size_t effocr_regnet_weights_bytes(const effocr_regnet_t* enc);
/* folds every BatchNorm (eps 1e-5) into its convolution in double precision, rounds once to fp32 and, for the
 * 16-bit modes, once more to the operand type, and packs the device blob weights_dev
 * (>= effocr_regnet_weights_bytes; synchronous copy) */
int effocr_regnet_upload(effocr_regnet_t* enc, void* weights_dev, size_t bytes);

/* Device workspace a forward of `batch` crops needs (0 for batch <= 0).  Calls run in sub-batches of
 * effocr_regnet_set_chunk crops (0 = the default: the largest sub-batch whose workspace stays under 1 GB,
 * at most 256 crops), so this stops growing at the sub-batch size.  The first 256 bytes hold the sticky
 * status word; zero them once in a fresh workspace. */
size_t effocr_regnet_workspace_bytes(const effocr_regnet_t* enc, int batch);
/* crops_per_chunk in [0, 65535]; anything else is EFFOCR_REGNET_EINVAL */
int effocr_regnet_set_chunk(effocr_regnet_t* enc, int crops_per_chunk);

/* x_dev [batch,3,img,img] fp32 NCHW, ImageNet-normalised crops -> emb_dev [batch,D] fp32: the global average
 * pool of the last block, L2-normalised (F.normalize) when l2_normalize != 0.  A crop's embedding is bitwise
 * independent of `batch` and of the chunk setting.  A non-finite embedding ORs 1 into the workspace's status
 * word.  Every argument is checked, the workspace size included, before the first launch. */
int effocr_regnet_forward(effocr_regnet_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize,
                          void* workspace_dev, size_t workspace_bytes, void* stream);

/* Reads and clears the status word (synchronises `stream`): EFFOCR_REGNET_EOVERFLOW if any forward on this
 * workspace since the last check or reset produced a non-finite embedding, else 0. */
int effocr_regnet_check_status(const effocr_regnet_t* enc, const void* workspace_dev, void* stream);
/* Clears the status word without reading it (asynchronous on `stream`). */
int effocr_regnet_reset_status(const effocr_regnet_t* enc, void* workspace_dev, void* stream);

/* TEST ENTRY POINTS (tests/test_gpu_regnet_ops.py, tools/regnet_time.py; no product code calls them): the
 * library's own kernels on caller-made tensors.  Activations are fp32 channels-last [B,H,H,C]. */
/* tiles of the per-tile channel sums of an out_size x out_size map (runs of 64 pixels) */
int effocr_regnet_op_tiles(int out_size);
/* HOST side: bytes of the packed grouped weight, and the packing of w_host [C][gw][3][3] fp32 (torch's layout)
 * into packed_host the way upload does it (fp32: [9][C][gw]; 16-bit: rounded once, [C/16 tiles][9][input
 * tiles][16][16] with zeros between groups) */
size_t effocr_regnet_op_gconv_weight_bytes(int precision, int channels, int group_width);
int effocr_regnet_op_pack_gconv(int precision, int channels, int group_width, const float* w_host, void* packed_host);
/* out_dev [B,Ho,Ho,C] = ReLU(grouped conv3x3 pad 1 (in_dev; packed w_dev) + b_dev), Ho = (H - 1) / stride + 1;
 * group_width 8, 16 or 24, C a multiple of it, stride 1 or 2; part_dev NULL or [B][op_tiles(Ho)][C]: the
 * channel sums of out_dev over each run of 64 pixels */
int effocr_regnet_op_gconv(int precision, const float* in_dev, int batch, int in_size, int channels, int stride, int group_width,
                           const void* w_dev, const float* b_dev, float* out_dev, float* part_dev, void* stream);
/* gate_dev [B,C] = sigmoid(fc2(ReLU(fc1(sum of part_dev over its tiles / pixels)))); fc1_w_dev [R][C],
 * fc2_wt_dev [R][C] (fc2's weight TRANSPOSED); C <= 1024, R <= 256 */
int effocr_regnet_op_se_gate(const float* part_dev, int batch, int tiles, int pixels, int channels, int se_width, const float* fc1_w_dev,
                             const float* fc1_b_dev, const float* fc2_wt_dev, const float* fc2_b_dev, float* gate_dev, void* stream);
/* x_dev [B,3,S,S] fp32 NCHW (S even), w_dev [27][32] tap-major ((ci, ky, kx) taps), b_dev [32] -> out_dev
 * [B,S/2,S/2,32] = ReLU(conv3x3/2 pad 1 + bias) */
int effocr_regnet_op_stem(const float* x_dev, int batch, int img_size, const float* w_dev, const float* b_dev, float* out_dev, void* stream);
/* out_dev [B,Ho,Ho,C] = in_dev [B,H,H,C] at the even rows and columns, Ho = (H - 1) / 2 + 1; C % 4 == 0 */
int effocr_regnet_op_gather2(const float* in_dev, int batch, int in_size, int channels, float* out_dev, void* stream);
/* x_dev[i] = max(x_dev[i], 0) in place, numel a multiple of 4 */
int effocr_regnet_op_relu(float* x_dev, int64_t numel, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFOCR_REGNET_H */
