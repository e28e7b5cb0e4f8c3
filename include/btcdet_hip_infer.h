/* btcdet_hip_infer.h -- inference entry points of libbtcdet_hip.so (gfx950), the second public header beside btcdet_hip.h.
 *
 * Same common rules as btcdet_hip.h: every pointer is a DEVICE pointer unless its name starts with h_; the caller allocates every
 * buffer; `stream` is a hipStream_t (NULL = the default stream) and every call only enqueues work on it; an entry point returns
 * BTC_OK or a BTC_E* code, with the text in btc_last_error(), and never exits the process.  The constants (BTC_OK, BTC_OPERANDS_*)
 * are those of btcdet_hip.h. */
#ifndef BTCDET_HIP_INFER_H
#define BTCDET_HIP_INFER_H

#include <stddef.h>
#include <stdint.h>

#include "btcdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sparse conv -> BatchNorm1d in EVAL mode (running statistics) -> optional ReLU as ONE launch, for a forward pass nobody
 * differentiates: the conv kernel applies
 *
 *     y[r][c] = relu?( (v - running_mean[c]) * rstd[c] * gamma[c] + beta[c] ),   rstd[c] = 1.0f / sqrtf(running_var[c] + eps)
 *
 * in its epilogue, to the result tile it holds in registers, where v is the value btc_conv_apply_src would have stored in its
 * result (bias added; for bf16 activations rounded to bf16 and widened again).  Only y [n_rows][Cout] (activation type of
 * `operands`) is written: no conv result, no saved statistics, no BatchNorm workspace.  y is bit-identical to
 * btc_conv_apply_src(BTC_PASS_FWD, ...) followed by btc_bn_relu_fwd[_bf16](training = 0) on the same inputs.
 *
 *   operands, src, src_rows, W, bias, nbr, order, n_rows, K, Cin, Cout : as btc_conv_apply_src with pass = BTC_PASS_FWD (every
 *       operand kind; src_rows is required for BTC_OPERANDS_F32_SPLIT; order may be NULL).  n_rows >= 1.
 *   gamma, beta   : [Cout] fp32, each may be NULL (1 / 0)
 *   running_mean, running_var : [Cout] fp32, READ ONLY (num_batches_tracked is not an argument: nothing is tracked)
 *   Cout <= 1024. */
int btc_conv_bn_eval_fwd(int operands, const void* src, long long src_rows, const void* W, const float* bias, const int32_t* nbr,
                         const int32_t* order, int n_rows, int K, int Cin, int Cout, const float* gamma, const float* beta,
                         const float* running_mean, const float* running_var, float eps, int relu, void* y, void* stream);

/* ---- Detections from the eval-mode head outputs: the reference's Detector3DTemplate.post_processing (score threshold, class-agnostic
 * NMS, padded outputs, recall record) as TWO launches per batch and no read-back.
 *
 * btc_det_select_nms -- per scene: score = max over classes of sigmoid(cls_preds) (of cls_preds itself when `normalized`); candidates
 * = the min(pre_max, count) boxes with score >= score_thresh (a NaN fails) in descending score order, equal scores in ascending input
 * index; the greedy NMS chain over them (rotated BEV IoU when `rotated`, axis-aligned BEV IoU otherwise; a box is suppressed by a kept
 * box of higher rank with IoU > nms_thresh), stopped at post_max kept boxes.  One launch behind a memset of `batch` counters.
 *
 *   cls_preds  [batch][n][num_class] fp32          box_preds [batch][n][box_stride] fp32, a box = its first 7 values
 *   keep       [batch][post_max] int64  OUT  input indices (0 .. n-1) of the kept boxes in descending score order, -1 padded
 *   num_keep   [batch] int32            OUT
 *   best_class [batch][n] int32         OUT  index of the class with the highest score (the first of equal ones)
 *   ws         btc_det_select_nms_ws_bytes(batch, n) bytes, contents arbitrary
 *   n <= 1024 (BTC_EINVAL beyond: sort the scores and use btc_nms_topk), num_class >= 1, box_stride >= 7, pre_max >= 1,
 *   1 <= post_max <= 4096. */
size_t btc_det_select_nms_ws_bytes(int batch, int n);
int btc_det_select_nms(const float* cls_preds, const float* box_preds, int batch, int n, int num_class, int box_stride, int normalized,
                       float score_thresh, float nms_thresh, int rotated, int pre_max, int post_max, long long* keep, int32_t* num_keep,
                       int32_t* best_class, void* ws, size_t ws_bytes, void* stream);

/* btc_det_finish -- the kept rows gathered into padded outputs and the recall record of generate_recall_record, one launch.
 *
 *   keep, num_keep : as btc_det_select_nms writes them (an entry outside 0 .. n-1 is treated as padding)
 *   best_class     : [batch][n] int32; labels: [batch][n] int64 or NULL.  pred_labels = labels[kept] when given, best_class[kept] + 1 otherwise
 *   pred_boxes  [batch][post_max][box_stride]  OUT  rows of box_preds; padding rows are zeros, in every output
 *   pred_scores [batch][post_max] fp32         OUT  the score as above, or max over classes of cls_preds as it is when raw_score
 *   pred_labels [batch][post_max] int64        OUT
 *   pred_iou    [batch][post_max] fp32         OUT  without rois: the best 3-D IoU of kept box k with the scene's ground truth; with rois:
 *                                                   of INPUT box k (k < n) -- the reference takes the row maxima of the matrix it built
 *   gt_boxes    [batch][n_gt][gt_stride >= 7] or NULL (no recall record, pred_iou = 0).  Per scene the trailing rows whose entries sum
 *               to zero are trimmed, but never the first row: a scene without boxes counts ONE ground truth, as in the reference.
 *   rois        [batch][n_rois][roi_stride >= 7] or NULL
 *   h_thresh    HOST [n_thresh <= 8] recall thresholds
 *   counters    int64 [1 + 2 n_thresh], ADDED TO: [0] += ground truths; [1 + t] += ground truths whose best 3-D IoU over the rois
 *               exceeds h_thresh[t] (0 without rois); [1 + n_thresh + t] += the same over ALL n boxes of box_preds when rois are given
 *               (as the reference), over the kept boxes otherwise.  3-D IoU as iou3d_nms_utils.boxes_iou3d_gpu. */
int btc_det_finish(const float* cls_preds, const float* box_preds, int batch, int n, int num_class, int box_stride, int normalized,
                   int raw_score, const long long* keep, const int32_t* num_keep, const int32_t* best_class, const long long* labels,
                   int post_max, const float* gt_boxes, int n_gt, int gt_stride, const float* rois, int n_rois, int roi_stride,
                   const float* h_thresh, int n_thresh, float* pred_boxes, float* pred_scores, long long* pred_labels, float* pred_iou,
                   long long* counters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BTCDET_HIP_INFER_H */
