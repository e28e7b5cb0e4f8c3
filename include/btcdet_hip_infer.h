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

/* ---- Occupancy metrics of an eval batch: the counts behind the reference's Detector3DTemplate.occ_post_processing (precision / recall / F1
 * of the predicted occupancy at 0.5, and the ground-truth boxes that receive an added occupancy point at probability >= 0.1 .. 0.9) as one
 * memset and at most TWO launches per batch, for any number of scenes, boxes and points, and no read-back.
 *
 * btc_occ_metrics fully overwrites one row of 16 int64 counters:
 *
 *   [0] total        sum of cls_mask (general_cls_loss_mask)          [1] pos_num  sum of pos_mask        [2] neg_num  sum of neg_mask
 *   [3] pos_predict  cells with prob >= 0.5f (ALL cells: the head has multiplied prob by the mask; a NaN fails)
 *   [4] pos_correct  cells with pos_mask set and prob >= 0.5f         [5] pos_all_num, copied through
 *   [6] box_num_sum  sum over the scenes of gt_boxes_num              (also when there is no point)
 *   [7 + k], k = 0 .. 8: valid boxes that contain at least one point whose probability is >= (float)((k + 1) * 0.1) -- the product in
 *                    double, rounded to float32 once: the value torch compares a float32 tensor with.  Each scene's boxes against that
 *                    scene's points only; a point inside several boxes counts for each of them.
 *
 *   prob      [n_cells] fp32          cls_mask, pos_mask, neg_mask  [n_cells] bytes, 0 / 1 (a non-zero byte counts once); ANY alignment
 *   pos_all_num  one int32
 *   occ_pnts  [n_points][4] fp32  x y z probability (>= 0; 16-byte aligned)      occ_b_ind [n_points] int64, the point's scene; a point whose
 *             scene is outside 0 .. batch-1 takes no part.  n_points may be 0 (both pointers may be NULL then): counters 7 .. 15 are 0.
 *   gt_boxes  [batch][max_boxes][gt_stride >= 7] fp32  x y z dx dy dz heading; gt_boxes_num [batch] int32, clamped to 0 .. max_boxes.  ONLY
 *             the first gt_boxes_num[b] rows of scene b are read.  A point is inside a box when, in the box's frame, |x| <= dx / 2,
 *             |y| <= dy / 2 and |z| <= dz / 2 (both faces inclusive).  max_boxes has no limit.
 *   ws        btc_occ_metrics_ws_bytes(batch, max_boxes) bytes, contents arbitrary */
size_t btc_occ_metrics_ws_bytes(int batch, int max_boxes);
int btc_occ_metrics(const float* prob, const uint8_t* cls_mask, const uint8_t* pos_mask, const uint8_t* neg_mask, long long n_cells,
                    const int32_t* pos_all_num, const float* occ_pnts, const long long* occ_b_ind, long long n_points, const float* gt_boxes,
                    const int32_t* gt_boxes_num, int batch, int max_boxes, int gt_stride, long long* counters, void* ws, size_t ws_bytes,
                    void* stream);

/* ---- KITTI AP evaluation: the reference's kitti_object_eval_python (eval.py's overlaps and the two passes of compute_statistics_jit) for
 * a whole dataset in a constant number of launches.  The ground truths, detections and DontCare boxes of ALL frames arrive concatenated,
 * everything float64 (scores are never rounded: ties are decided on the caller's values):
 *
 *   gt_rows  [NG][12]  image box x1 y1 x2 y2, location x y z (camera frame, y the bottom face), dimensions l h w, rotation_y, alpha
 *   dt_rows  [ND][13]  the same 12 and the score
 *   dc_boxes [NC][4]   the image boxes of a frame's DontCare ground truths, in their order
 *   frames   [n_frames + 1][3] int32  index of each frame's first ground truth / detection / DontCare box (row n_frames: NG, ND, NC)
 *   pairs    [n_frames + 1][2] int64  exclusive prefix sums over the frames of n_dt * n_gt and of n_dt * n_dc
 *   h_frames HOST copy of `frames`: the argument checks read it.  A frame with more than 1024 detections or more than 1024 ground
 *            truths is BTC_EINVAL (refused, never truncated); zero frames and frames without boxes are valid.
 *
 * btc_kitti_overlaps -- per frame, and only within it, the [n_dt][n_gt] blocks of the three metrics, one launch:
 *   ov    [3][P] OUT  P = pairs[n_frames][0]; metric 0 the image-box IoU (image_box_overlap, criterion -1), 1 the rotated BEV IoU of
 *                     (x, z, l, w, rotation_y), 2 d3_box_overlap: the BEV intersection x the height overlap over the union of volumes.
 *                     Entry pairs[f][0] + j * n_gt + i is detection j against ground truth i of frame f.
 *   ov_dc [PD]   OUT  detection against DontCare box, the detection's area as denominator (image_box_overlap criterion 0), at
 *                     pairs[f][1] + j * n_dc + i.
 *   The rotated intersection is exact convex clipping in float64 (no margin, unlike the NMS kernels' box_overlap). */
int btc_kitti_overlaps(const double* gt_rows, const double* dt_rows, const double* dc_boxes, const int32_t* frames, const long long* pairs,
                       const int32_t* h_frames, int n_frames, double* ov, double* ov_dc, void* stream);

/* The matching.  A combination is (metric, class, difficulty, overlap level), index ((m * n_class + c) * n_diff + d) * n_level + k, the
 * metrics being metric_first .. metric_first + n_metric - 1 (0 bbox, 1 bev, 2 3d).
 *
 *   ign_gt [n_class * n_diff][NG] int8, ign_dt [n_class * n_diff][ND] int8: clean_data's 0 counted / 1 ignored / -1 another class
 *   min_overlaps [n_level][3][n_class] float64
 *
 * btc_kitti_match_tp -- pass A (thresh = 0, compute_fp = False) of every frame and combination, a memset and one launch:
 *   tp_det   [combinations][NG] int32 OUT  index into dt_rows of the detection ground truth g matched as a true positive, else -1
 *   tp_count [combinations] int32     OUT  the number of true positives
 *
 * btc_kitti_match_stats -- pass B (compute_fp = True) of every frame, combination and threshold: memsets and two launches.
 *   thresholds [combinations][41] float64, n_thresholds [combinations] int32 (0 .. 41): get_thresholds' list of each combination
 *   counts     [combinations][41][3] int32 OUT  tp, fp (DontCare detections subtracted for metric 0), fn, summed over the frames
 *   similarity [n_class * n_diff * n_level][41] float64 OUT  sum over the true positives of (1 + cos(alpha_gt - alpha_dt)) / 2 for
 *              metric 0 when compute_aos and metric_first == 0, zeros otherwise; per-frame partials summed in frame order (same bits
 *              every run)
 *   ws         btc_kitti_match_stats_ws_bytes(...) bytes, contents arbitrary */
int btc_kitti_match_tp(const double* ov, const double* dt_rows, const int8_t* ign_gt, const int8_t* ign_dt, const double* min_overlaps,
                       const int32_t* frames, const long long* pairs, const int32_t* h_frames, int n_frames, int metric_first, int n_metric,
                       int n_class, int n_diff, int n_level, int32_t* tp_det, int32_t* tp_count, void* stream);
size_t btc_kitti_match_stats_ws_bytes(int n_frames, int n_class, int n_diff, int n_level, int compute_aos);
int btc_kitti_match_stats(const double* ov, const double* ov_dc, const double* gt_rows, const double* dt_rows, const int8_t* ign_gt,
                          const int8_t* ign_dt, const double* min_overlaps, const double* thresholds, const int32_t* n_thresholds,
                          const int32_t* frames, const long long* pairs, const int32_t* h_frames, int n_frames, int metric_first, int n_metric,
                          int n_class, int n_diff, int n_level, int compute_aos, int32_t* counts, double* similarity, void* ws,
                          size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BTCDET_HIP_INFER_H */
