/* effocr_yolo11.h — C ABI of libeffocr_yolo11.so: the ultralytics YOLO11 detection networks
 * yolo11n / s / m / l / x as character / word localizers on the MI355X (gfx950) — what the ultralytics
 * package has trained by default since late 2024 (yolo11.yaml: 3x3 stem, C3k2 blocks, a C2PSA block of
 * multi-head self-attention on the stride-32 map, the YOLOv8 anchor-free head with a depthwise class
 * branch).
 *
 * UNVERIFIED against an ultralytics install: the network was written from the published yaml and
 * nn/modules, none was at hand to compare a forward with.  What pins it is the parameter count —
 * learnable parameters plus the 16 of the DFL — which equals the five figures ultralytics prints for
 * the unfused models at 80 classes (tests/test_yolo11_host.py):
 *     scale   nc = 80        nc = 2
 *     n        2 624 080      2 590 230
 *     s        9 458 752      9 428 566
 *     m       20 114 688     20 054 550
 *     l       25 372 160     25 312 022
 *     x       56 966 176     56 876 086
 *
 * A library of its own, like libeffocr_yolov8.so: it neither links against libeffocr_hip.so nor shares
 * its error state; the implicit-GEMM convolution (resnet.hip), the YOLOv5 engine's data-movement kernels
 * (yolo.hip) and the YOLOv8 stem and decode (yolov8.hip) are compiled into it once more with hidden
 * visibility.  forward writes rows of 5 + nc floats (cx, cy, w, h, 1.0, class scores) — the layout of a
 * YOLOv5 prediction with the objectness column the constant 1.0f — so effocr_nms / effocr_nms_batch of
 * effocr_hip.h apply to them unchanged.  Conventions are those of effocr_hip.h:
 *   - every *_dev pointer is caller-owned DEVICE memory; the library allocates no device memory;
 *   - calls that take a `stream` are asynchronous on it (hipStream_t passed as void*; NULL = the
 *     default stream);
 *   - 0 on success, a negative EFFOCR_YOLO11_E* code on failure (the same values as effocr_hip.h's
 *     EFFOCR_E* codes), the message from effocr_yolo11_last_error() (thread-local).
 *
 * The protocol is the one of effocr_yolov8.h: create -> set_param x N -> upload -> forward ...;
 * parameter names are the ultralytics state-dict keys (model.0.conv.weight ... model.23.cv3.2.2.bias,
 * model.23.dfl.conv.weight) without `num_batches_tracked`.
 *
 * Operand rule of "bf16_operands": every implicit-GEMM convolution — the ones without an activation in
 * C2PSA (attn.qkv, attn.proj, ffn.1) included — takes bf16-rounded weights (BN folded first) and inputs
 * and accumulates in fp32.  Exceptions, fp32 operands in both modes: the stem (model.0), the last 1x1
 * convolution of each Detect branch, the attention kernel and every depthwise 3x3 convolution (attn.pe
 * and the class branch's two), which are about 1 % of yolo11n's FLOPs and 0.1 % of yolo11x's.
 */
#ifndef EFFOCR_YOLO11_H
#define EFFOCR_YOLO11_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an exported signature or the meaning of an argument changes; effocr_amd/_lib.py
 * refuses a library whose effocr_yolo11_abi_version() differs */
#define EFFOCR_YOLO11_ABI_VERSION 1

/* tokens (pixels of the stride-32 map) per image the attention kernel is tested up to: a 1280 x 1280 input */
#define EFFOCR_YOLO11_MAX_TOKENS 1600

enum effocr_yolo11_status {
  EFFOCR_YOLO11_OK = 0,
  EFFOCR_YOLO11_EINVAL = -1,        /* bad argument (NULL pointer, unknown name or option, wrong numel, bad size, a DFL tensor that is not 0..15) */
  EFFOCR_YOLO11_EUNSUPPORTED = -2,  /* valid request outside what the kernels implement (another architecture, more tokens than the cap) */
  EFFOCR_YOLO11_EWORKSPACE = -3,    /* caller-provided workspace / weight buffer too small */
  EFFOCR_YOLO11_EHIP = -4,          /* HIP runtime error */
  EFFOCR_YOLO11_ESTATE = -5         /* call order violated (forward before upload, a parameter never set) */
};

typedef struct effocr_yolo11 effocr_yolo11_t;

int effocr_yolo11_abi_version(void);
const char* effocr_yolo11_last_error(void);

/* arch = "yolo11n" | "yolo11s" | "yolo11m" | "yolo11l" | "yolo11x" (ultralytics dropped the "v"; anything
 * else, e.g. "yolov11n", "yolo11n-seg", "yolo11n-pose", "yolo11n-obb", "yolo11n-cls", "yolo12n", "yolov8s",
 * is EFFOCR_YOLO11_EUNSUPPORTED); num_classes in 1..80; in_h, in_w positive multiples of 32 with
 * (in_h / 32)(in_w / 32) <= EFFOCR_YOLO11_MAX_TOKENS, more is EFFOCR_YOLO11_EUNSUPPORTED. */
int effocr_yolo11_create(const char* arch, int num_classes, int in_h, int in_w, effocr_yolo11_t** out);
void effocr_yolo11_destroy(effocr_yolo11_t* loc);

int effocr_yolo11_num_params(const effocr_yolo11_t* loc);
const char* effocr_yolo11_param_name(const effocr_yolo11_t* loc, int i);   /* NULL when i is out of range */
int64_t effocr_yolo11_param_numel(const effocr_yolo11_t* loc, int i);      /* -1 when i is out of range */
/* host fp32 copy of one parameter (torch's layout and shape, numel must match) */
int effocr_yolo11_set_param(effocr_yolo11_t* loc, const char* name, const float* host, int64_t numel);
size_t effocr_yolo11_weights_bytes(const effocr_yolo11_t* loc);
/* folds every BatchNorm into its convolution and packs the device blob weights_dev (>= effocr_yolo11_weights_bytes;
 * synchronous copy).  EFFOCR_YOLO11_EINVAL unless model.23.dfl.conv.weight is the constant 0, 1, ... 15. */
int effocr_yolo11_upload(effocr_yolo11_t* loc, void* weights_dev, size_t bytes);

/* options, as effocr_yolov8_set_option: "bf16_operands" (the rule above), "call_size_invariant" (1: no
 * convolution splits K, an image's rows are bitwise the same in every batch size and position; the
 * attention and depthwise kernels have that property in both settings), "direct_stem" (default 1; 0: the
 * stem as im2col rows + the 1x1 implicit GEMM, the cross-check) */
int effocr_yolo11_set_option(effocr_yolo11_t* loc, const char* name, int value);

int64_t effocr_yolo11_num_predictions(const effocr_yolo11_t* loc);   /* (H/8)(W/8) + (H/16)(W/16) + (H/32)(W/32): 8400 at 640 x 640 */
int effocr_yolo11_num_outputs(const effocr_yolo11_t* loc);           /* 5 + num_classes */
size_t effocr_yolo11_workspace_bytes(const effocr_yolo11_t* loc, int batch);   /* 0 for batch <= 0 */

/* x_dev [batch,3,in_h,in_w] fp32 (NCHW, letterboxed, RGB, 0..1) -> pred_dev [batch, num_predictions, 5 + nc]:
 * rows of level stride 8, then 16, then 32, anchor points row-major inside a level;
 * (cx, cy, w, h) in input pixels, 1.0f, sigmoid class scores. */
int effocr_yolo11_forward(effocr_yolo11_t* loc, const float* x_dev, int batch, float* pred_dev, void* workspace_dev, size_t workspace_bytes,
                          void* stream);

/* ---- test entry points: one kernel each on dense tensors; no product code calls them ---- */
/* qkv_dev NHWC fp32 [batch, H*W, heads*128], channel head*128 + (q 0..31 | k 32..63 | v 64..127) — what the qkv
 * convolution writes — -> out_dev [batch, H*W, heads*64] = softmax_m(32^-1/2 q_n . k_m) v_m per head.
 * H*W <= EFFOCR_YOLO11_MAX_TOKENS. */
int effocr_yolo11_op_attention(const float* qkv_dev, int batch, int H, int W, int heads, float* out_dev, void* stream);
/* depthwise 3x3, stride 1, zero pad 1: x_dev NHWC fp32 rows of ld_in >= C floats, w_dev [C][9] (tap ky*3 + kx),
 * bias_dev [C], silu 0 | 1 -> out_dev rows of ld_out >= C floats.  C, ld_in, ld_out multiples of 4. */
int effocr_yolo11_op_dwconv3x3(const float* x_dev, int batch, int H, int W, int C, int ld_in, const float* w_dev, const float* bias_dev, int silu,
                               float* out_dev, int ld_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFOCR_YOLO11_H */
