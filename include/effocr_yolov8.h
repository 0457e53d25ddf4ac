/* effocr_yolov8.h — C ABI of libeffocr_yolov8.so: the ultralytics YOLOv8 detection networks
 * yolov8n / s / m / l / x as character / word localizers on the MI355X (gfx950) — what a localizer
 * trained with today's ultralytics package is (yolov8.yaml: 3x3 stem, C2f blocks, an anchor-free
 * decoupled head whose box branch is a 16-bin distribution per side, no objectness).
 *
 * A library of its own: libeffocr_hip.so is at its size cap (DESIGN.md "Library split"), so this one
 * neither links against it nor shares its error state; the implicit-GEMM convolution (resnet.hip) and
 * the YOLOv5 engine's data-movement kernels (yolo.hip) are compiled into it a second time with hidden
 * visibility.  YOLOv5 stays on effocr_localizer_create (effocr_hip.h), and so do the letterbox and the
 * NMS: forward writes rows of 5 + nc floats (cx, cy, w, h, 1.0, class scores) — the layout of a YOLOv5
 * prediction with the objectness column the constant 1.0f — so effocr_nms / effocr_nms_batch of
 * effocr_hip.h apply to them unchanged.  Conventions are those of effocr_hip.h:
 *   - every *_dev pointer is caller-owned DEVICE memory; the library allocates no device memory;
 *   - calls that take a `stream` are asynchronous on it (hipStream_t passed as void*; NULL = the
 *     default stream);
 *   - 0 on success, a negative EFFOCR_YOLOV8_E* code on failure (the same values as effocr_hip.h's
 *     EFFOCR_E* codes), the message from effocr_yolov8_last_error() (thread-local).
 *
 * The protocol is the one of the effocr_localizer_* section of effocr_hip.h: create -> set_param x N ->
 * upload -> forward ...; parameter names are the ultralytics state-dict keys (model.0.conv.weight ...
 * model.22.cv3.2.2.bias, model.22.dfl.conv.weight) without `num_batches_tracked`.
 */
#ifndef EFFOCR_YOLOV8_H
#define EFFOCR_YOLOV8_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an exported signature or the meaning of an argument changes; effocr_amd/_lib.py
 * refuses a library whose effocr_yolov8_abi_version() differs */
#define EFFOCR_YOLOV8_ABI_VERSION 1

enum effocr_yolov8_status {
  EFFOCR_YOLOV8_OK = 0,
  EFFOCR_YOLOV8_EINVAL = -1,        /* bad argument (NULL pointer, unknown name or option, wrong numel, bad size, a DFL tensor that is not 0..15) */
  EFFOCR_YOLOV8_EUNSUPPORTED = -2,  /* valid request outside what the kernels implement (another architecture) */
  EFFOCR_YOLOV8_EWORKSPACE = -3,    /* caller-provided workspace / weight buffer too small */
  EFFOCR_YOLOV8_EHIP = -4,          /* HIP runtime error */
  EFFOCR_YOLOV8_ESTATE = -5         /* call order violated (forward before upload, a parameter never set) */
};

typedef struct effocr_yolov8 effocr_yolov8_t;

int effocr_yolov8_abi_version(void);
const char* effocr_yolov8_last_error(void);

/* arch = "yolov8n" | "yolov8s" | "yolov8m" | "yolov8l" | "yolov8x" (the detection yaml; anything else,
 * e.g. "yolov5s", "yolov8s6", "yolov8s-seg", is EFFOCR_YOLOV8_EUNSUPPORTED); num_classes in 1..80;
 * in_h, in_w positive multiples of 32. */
int effocr_yolov8_create(const char* arch, int num_classes, int in_h, int in_w, effocr_yolov8_t** out);
void effocr_yolov8_destroy(effocr_yolov8_t* loc);

int effocr_yolov8_num_params(const effocr_yolov8_t* loc);
const char* effocr_yolov8_param_name(const effocr_yolov8_t* loc, int i);   /* NULL when i is out of range */
int64_t effocr_yolov8_param_numel(const effocr_yolov8_t* loc, int i);      /* -1 when i is out of range */
/* host fp32 copy of one parameter (torch's layout and shape, numel must match) */
int effocr_yolov8_set_param(effocr_yolov8_t* loc, const char* name, const float* host, int64_t numel);
size_t effocr_yolov8_weights_bytes(const effocr_yolov8_t* loc);
/* folds every BatchNorm into its convolution and packs the device blob weights_dev (>= effocr_yolov8_weights_bytes;
 * synchronous copy).  EFFOCR_YOLOV8_EINVAL unless model.22.dfl.conv.weight is the constant 0, 1, ... 15. */
int effocr_yolov8_upload(effocr_yolov8_t* loc, void* weights_dev, size_t bytes);

/* options, as effocr_localizer_set_option: "bf16_operands" (1: bf16-rounded operands for every convolution
 * with an activation, fp32 accumulation; the stem and the last 1x1 convolution of each Detect branch stay
 * fp32), "call_size_invariant" (1: no convolution splits K, an image's rows are bitwise the same in every
 * batch size and position), "direct_stem" (default 1; 0: the stem as im2col rows + the 1x1 implicit GEMM,
 * the cross-check) */
int effocr_yolov8_set_option(effocr_yolov8_t* loc, const char* name, int value);

int64_t effocr_yolov8_num_predictions(const effocr_yolov8_t* loc);   /* (H/8)(W/8) + (H/16)(W/16) + (H/32)(W/32): 8400 at 640 x 640 */
int effocr_yolov8_num_outputs(const effocr_yolov8_t* loc);           /* 5 + num_classes */
size_t effocr_yolov8_workspace_bytes(const effocr_yolov8_t* loc, int batch);   /* 0 for batch <= 0 */

/* x_dev [batch,3,in_h,in_w] fp32 (NCHW, letterboxed, RGB, 0..1) -> pred_dev [batch, num_predictions, 5 + nc]:
 * rows of level stride 8, then 16, then 32, anchor points row-major inside a level;
 * (cx, cy, w, h) in input pixels, 1.0f, sigmoid class scores. */
int effocr_yolov8_forward(effocr_yolov8_t* loc, const float* x_dev, int batch, float* pred_dev, void* workspace_dev, size_t workspace_bytes,
                          void* stream);

/* ---- test entry points: one kernel each on caller-made device tensors (tests/test_gpu_localizer_ops.py); no handle, nothing of
 * forward's state.  libeffocr_yolo11.so runs the same two kernels and has no entry points of its own for them.
 *
 * Detect decode of one level: box_dev [batch * ny * nx][box_ld] (the first 64 floats of a row: left, top, right, bottom x 16 bin
 * logits; box_ld >= 64, a multiple of 4), cls_dev [batch * ny * nx][cls_ld] (nc class logits, cls_ld >= nc) -> rows row0 .. row0 + ny * nx
 * of pred_dev [batch][total][5 + nc] = (cx, cy, w, h) * stride, 1.0f, sigmoid class scores; no other row is touched. */
int effocr_yolov8_op_decode(const float* box_dev, int box_ld, const float* cls_dev, int cls_ld, float* pred_dev, int batch, int ny, int nx, int nc,
                            float stride, int64_t total, int64_t row0, void* stream);
/* The 3x3 / stride 2 / pad 1 stem + SiLU: x_dev [batch][3][H][W], wt_dev [27][wt_ld] (row (ky * 3 + kx) * 3 + c, wt_ld >= cout_st, a
 * multiple of 4), bias_dev [cout_st] (0 from cout on) -> channels out_off .. out_off + cout_st of out_dev [batch * OH * OW][out_ld], the
 * channels cout .. cout_st exactly 0.  OH = ceil(H / 2), OW = ceil(W / 2) a multiple of 4; cout, cout_st multiples of 16. */
int effocr_yolov8_op_stem(const float* x_dev, const float* wt_dev, int wt_ld, const float* bias_dev, float* out_dev, int batch, int H, int W, int OH,
                          int OW, int out_ld, int out_off, int cout, int cout_st, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFOCR_YOLOV8_H */
