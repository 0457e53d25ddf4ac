/* effocr_head.h — C ABI of libeffocr_head.so: the FFNN classifier head of EffOCR's recognizer
 * (infer_effocr.py:325-333 — `logits = net(x)`, `logits.argmax(-1)` — with the timm classifier head
 * of models/classifiers.py:35-83) on the MI355X (gfx950).
 *
 * A library of its own: libeffocr_hip.so is at its size cap (DESIGN.md "Library split"), so this one
 * neither links against it nor shares its error state.  Conventions are those of effocr_hip.h:
 *   - every *_dev pointer is caller-owned DEVICE memory; the library allocates nothing;
 *   - calls are asynchronous on `stream` (hipStream_t passed as void*; NULL = the default stream);
 *   - 0 on success, a negative EFFOCR_HEAD_E* code on failure, the message from
 *     effocr_head_last_error() (thread-local).  A refused call launches nothing.
 */
#ifndef EFFOCR_HEAD_H
#define EFFOCR_HEAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an exported signature or the meaning of an argument changes; effocr_amd/_lib.py
 * refuses a library whose effocr_head_abi_version() differs */
#define EFFOCR_HEAD_ABI_VERSION 1

enum effocr_head_status {
  EFFOCR_HEAD_OK = 0,
  EFFOCR_HEAD_EINVAL = -1,   /* bad argument (shape, NULL / misaligned pointer, workspace too small) */
  EFFOCR_HEAD_EHIP = -4      /* HIP runtime error (launch failure)                                */
};

int effocr_head_abi_version(void);
const char* effocr_head_last_error(void);

/* Device bytes effocr_classifier_head needs as workspace when it is asked for ids (0 for batch <= 0). */
size_t effocr_classifier_head_workspace_bytes(int64_t batch, int n_classes);

/* logits[b, n] = dot(emb[b, :], w[n, :]) + bias[n] in exact fp32 (v_mfma_f32_16x16x4_f32), and/or
 * ids[b] = argmax_n logits[b, n] with torch.argmax's rules (first index of the maximum; a NaN is the
 * maximum and the first NaN wins).
 *   emb_dev    [batch, d] fp32, row-major, 16-byte aligned — the encoder's embedding BEFORE L2 normalisation
 *   w_dev      [n_classes, d] fp32 (timm's head weight, nn.Linear layout), 16-byte aligned
 *   b_dev      [n_classes] fp32
 *   logits_dev [batch, n_classes] fp32 or NULL (then no logit is written)
 *   ids_dev    [batch] int64 or NULL
 * The dot product runs in one fixed order for every (b, n) — k-blocks of 16 ascending; inside a block
 * k = 16j + t, 16j + 4 + t, 16j + 8 + t, 16j + 12 + t for t = 0..3, each step an fp32 fma — so every
 * logit and every id is bitwise independent of `batch`, of `n_classes` and of the tiling.
 * EFFOCR_HEAD_EINVAL: d % 4 != 0, d < 4, d > 4096, n_classes < 1, batch < 0, both outputs NULL, a NULL or
 * misaligned input, or (ids_dev != NULL) workspace_bytes < effocr_classifier_head_workspace_bytes().
 * batch == 0 (with valid d and n_classes) succeeds without looking at the pointers and launches nothing.
 * At most two kernel launches. */
int effocr_classifier_head(const float* emb_dev, int64_t batch, int d, const float* w_dev, const float* b_dev,
                           int n_classes, float* logits_dev, int64_t* ids_dev,
                           void* workspace_dev, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFOCR_HEAD_H */
