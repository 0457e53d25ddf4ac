/* effocr_levit.h — C ABI of libeffocr_levit.so: the LeViT recognizer encoders
 * (timm.create_model("levit_128s" | "levit_128" | "levit_192" | "levit_256" | "levit_384", num_classes=0), what
 * the reference builds for `--auto_model_timm <name>` in train_effocr_recognizer.py / infer_effocr.py) on the
 * MI355X (gfx950).  LeViT is a transformer at a CNN's cost: a four-convolution stem down to a 14 x 14 token
 * grid at 224^2, three stages of attention + MLP blocks with BatchNorm (folded on the host) in place of
 * LayerNorm, hardswish activations, and between the stages a down-sampling attention whose 7 x 7 (4 x 4)
 * strided queries attend to the 14 x 14 (7 x 7) keys.  Queries and keys are 16 or 32 wide, values 32 to 128, and
 * every attention adds a per-head bias looked up by the absolute row / column offset of query and key.
 *
 * A library of its own: libeffocr_hip.so is at its size cap (DESIGN.md "Library split"), so this one
 * neither links against it nor shares its error state; the GEMMs it needs are compiled into it once more with
 * hidden visibility.  Conventions are those of effocr_hip.h:
 *   - every *_dev pointer is caller-owned DEVICE memory; the library allocates no device memory;
 *   - calls that take a `stream` are asynchronous on it (hipStream_t passed as void*; NULL = the
 *     default stream);
 *   - 0 on success, a negative EFFOCR_LEVIT_E* code on failure (the same values as effocr_hip.h's
 *     EFFOCR_E* codes), the message from effocr_levit_last_error() (thread-local).
 *
 * The handle mirrors the encoder handle of effocr_hip.h: create -> set_param x N -> upload ->
 * forward ...; parameter names are timm >= 0.9's state-dict keys WITHOUT the "net." prefix and without the two
 * classifier heads (written from memory of timm's levit.py, not verified against a timm install):
 *   stem.conv{1..4}.{linear.weight, bn.*}
 *   stages.i.downsample.attn_downsample.{attention_biases, kv.{linear.weight, bn.*}, q.ln.*, proj.ln.*}   (i = 1, 2)
 *   stages.i.downsample.mlp.{ln1, ln2}.{linear.weight, bn.*}                                              (i = 1, 2)
 *   stages.i.blocks.j.attn.{attention_biases, qkv.{linear.weight, bn.*}, proj.ln.{linear.weight, bn.*}}
 *   stages.i.blocks.j.mlp.{ln1, ln2}.{linear.weight, bn.*}
 * with bn.* = bn.{weight, bias, running_mean, running_var}.
 */
#ifndef EFFOCR_LEVIT_H
#define EFFOCR_LEVIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an exported signature or the meaning of an argument changes; effocr_amd/_lib.py
 * refuses a library whose effocr_levit_abi_version() differs */
#define EFFOCR_LEVIT_ABI_VERSION 1

enum effocr_levit_status {
  EFFOCR_LEVIT_OK = 0,
  EFFOCR_LEVIT_EINVAL = -1,        /* bad argument (NULL pointer, bad img_size or precision, wrong numel)  */
  EFFOCR_LEVIT_EUNSUPPORTED = -2,  /* an architecture name or a shape this library does not implement      */
  EFFOCR_LEVIT_EWORKSPACE = -3,    /* caller-provided workspace / weight buffer too small                 */
  EFFOCR_LEVIT_EHIP = -4,          /* HIP runtime error                                                   */
  EFFOCR_LEVIT_ESTATE = -5,        /* call order violated (forward before upload, a parameter never set)  */
  EFFOCR_LEVIT_EOVERFLOW = -6      /* non-finite embedding (f16 activation overflow or non-finite input)  */
};

typedef struct effocr_levit effocr_levit_t;

int effocr_levit_abi_version(void);
const char* effocr_levit_last_error(void);

/* arch: "levit_128s", "levit_128", "levit_192", "levit_256", "levit_384", or the test miniatures
 * "levit_tiny_test" (widths 128-128-128, key width 16) and "levit_tiny32_test" (widths 128-192-256, key width
 * 32); anything else (levit_conv_*, levit_384_s8, levit_512*) is EFFOCR_LEVIT_EUNSUPPORTED.  img_size: a
 * multiple of 16 from 32 to 224 (EFFOCR_LEVIT_EINVAL otherwise); the token grid is img_size/16 per side and
 * fixes the length of every attention_biases row.  precision = EFFOCR_PREC_BF16 (0), EFFOCR_PREC_FP16 (1) or
 * EFFOCR_PREC_FP32 (2) of effocr_hip.h — the type of the weights, of the activations between the kernels and of
 * the MFMA operands (the residual stream, accumulators, softmax statistics, biases and the embedding are fp32
 * in every mode). */
int effocr_levit_create(const char* arch, int img_size, int precision, effocr_levit_t** out);
void effocr_levit_destroy(effocr_levit_t* enc);
int effocr_levit_embed_dim(const effocr_levit_t* enc);                  /* 384 / 384 / 384 / 512 / 768 */

int effocr_levit_num_params(const effocr_levit_t* enc);
const char* effocr_levit_param_name(const effocr_levit_t* enc, int i);  /* NULL when i is out of range */
int64_t effocr_levit_param_numel(const effocr_levit_t* enc, int i);     /* -1 when i is out of range */
/* host fp32 copy of one parameter (timm's layout and shape, numel must match) */
int effocr_levit_set_param(effocr_levit_t* enc, const char* name, const float* host, int64_t numel);
size_t effocr_levit_weights_bytes(const effocr_levit_t* enc);
/* folds every BatchNorm (double precision) and packs every parameter into the device blob weights_dev
 * (>= effocr_levit_weights_bytes; synchronous copy) */
int effocr_levit_upload(effocr_levit_t* enc, void* weights_dev, size_t bytes);

/* Device workspace a forward of `batch` crops needs (0 for batch <= 0).  Calls run in sub-batches of
 * effocr_levit_set_chunk crops (0 = the default: the largest sub-batch whose workspace stays under
 * 1 GB, at most 256 crops), so this stops growing at the sub-batch size.  The first 256 bytes hold the
 * sticky status word; zero them once in a fresh workspace. */
size_t effocr_levit_workspace_bytes(const effocr_levit_t* enc, int batch);
int effocr_levit_set_chunk(effocr_levit_t* enc, int crops_per_chunk);

/* x_dev [batch,3,img_size,img_size] fp32 (NCHW, ImageNet-normalised crops) -> emb_dev [batch,D] fp32: the
 * mean over the final tokens (what timm returns with num_classes=0), L2-normalised (F.normalize) when
 * l2_normalize != 0.  A crop's embedding is bitwise independent of `batch` and of the chunk setting.  A
 * non-finite embedding ORs 1 into the workspace's status word. */
int effocr_levit_forward(effocr_levit_t* enc, const float* x_dev, int batch, float* emb_dev, int l2_normalize,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

/* Reads and clears the status word (synchronises `stream`): EFFOCR_LEVIT_EOVERFLOW if any forward on this
 * workspace since the last check produced a non-finite embedding, else 0. */
int effocr_levit_check_status(const effocr_levit_t* enc, const void* workspace_dev, void* stream);
/* Clears the status word without reading it (asynchronous on `stream`). */
int effocr_levit_reset_status(const effocr_levit_t* enc, void* workspace_dev, void* stream);

/* Test entry points (no product code calls them).
 * The attention kernel alone: out = act(softmax(q k^T kd^-0.5 + bias[h][|dy| grid + |dx|]) v).  Keys and values:
 * the grid x grid tokens of every crop (1 <= grid <= 14), rows of kv_dev [batch*grid^2][ldkv], head h's keys at
 * feature h*kv_head_stride + k_off (kd wide) and values at h*kv_head_stride + v_off (vd wide).  Queries: rows of
 * q_dev [batch*Tq][ldq] at h*q_head_stride + q_off; stride 1: Tq = grid^2, the same positions; stride 2:
 * Tq = ((grid-1)/2 + 1)^2, query i at the even rows and columns of the key grid.  q_dev may equal kv_dev.
 * bias_dev [heads][grid^2] fp32.  out_dev [batch*Tq][heads*vd].  (kd, vd) is (16, 32), (16, 64), (32, 64) or
 * (32, 128); act: 0 = none, 1 = hardswish.  Elements are of `dtype`'s type (EFFOCR_PREC_*); strides and offsets
 * are multiples of 8 elements. */
int effocr_levit_op_attention(const void* q_dev, int64_t ldq, int q_head_stride, int q_off, const void* kv_dev, int64_t ldkv,
                              int kv_head_stride, int k_off, int v_off, const float* bias_dev, int batch, int grid, int stride,
                              int heads, int kd, int vd, int act, int dtype, void* out_dev, void* stream);
/* One stem convolution alone: 3x3, stride 2, pad 1, + bias_dev [cout] (+ hardswish when act).  in_dev: nchw = 1:
 * [batch][cin][size][size] fp32, rounded to `dtype`'s type as it is read; nchw = 0: [batch][size*size][cin] in
 * `dtype`'s type (cin % 8 == 0).  wt_dev [9*cin][cout] fp32, row (ky*3 + kx)*cin + c.  out_dev
 * [batch][OH*OH][ldo], OH = (size-1)/2 + 1, in `dtype`'s type or fp32 (out_f32); columns cout .. ldo are zeroed. */
int effocr_levit_op_stem_conv(const void* in_dev, int nchw, int batch, int size, int cin, const float* wt_dev, const float* bias_dev,
                              int cout, int act, int dtype, void* out_dev, int ldo, int out_f32, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFOCR_LEVIT_H */
