/* btcdet_hip_roi_targets.h -- the ROI head's training targets, fused: matching, sampling, gather, labels and the canonical transform
 * in ONE launch per batch; entry points of libbtcdet_hip.so (gfx950); the eleventh public header, the ROI-head counterpart of
 * btcdet_hip_heads.h (csrc/roi_targets.hip).
 *
 * Same common rules as btcdet_hip.h: every pointer is a DEVICE pointer (the configuration block alone is a HOST struct, read before the
 * call returns); the caller allocates every buffer; `stream` is a hipStream_t (NULL = the default stream) and every call only enqueues
 * work on it; an entry point returns BTC_OK or a BTC_E* code, with the text in btc_last_error(), and never exits the process.  No
 * memset, no read-back, no atomics on floating-point values: the same inputs give the same bits.
 *
 * What is replaced: ProposalTargetLayer.forward followed by canonical_targets (btcdet_amd/roi_targets.py; the reference's
 * proposal_target_layer.py:13-228 and roi_head_template.py:102-134) -- a per-scene Python loop of a pairwise-overlap launch, a dozen
 * elementwise launches, three sorts and five gathers, then five stacks, the label arithmetic and the transform.
 *
 *   rois (B, N, 7) f32 ; roi_scores (B, N) f32 ; roi_labels (B, N) i64, 1-based ; gt_boxes (B, G, 8) f32, zero-padded, class in column 7
 *   exactly one of  uniforms (B, 4, M) f32, M = max(R, N), values in [0, 1): the kernel samples from it
 *                   sampled_in (B, R) i64: the draw itself, nothing is sampled (an index outside [0, N) is clamped into it)
 *   cfg             struct BtcRoiTargetsConfig below (host memory)
 *   outputs, EVERY element written (the caller allocates them uninitialised):
 *   rois_out (B, R, 7) f32 ; gt_of_rois (B, R, 8) f32, canonical ; gt_of_rois_src (B, R, 8) f32 ; gt_iou_of_rois (B, R) f32 ;
 *   roi_scores_out (B, R) f32 ; roi_labels_out (B, R) i64 ; reg_valid_mask (B, R) i64 ;
 *   rcnn_cls_labels (B, R): f32 with score_type BTC_ROI_SCORE_ROI_IOU, i64 with BTC_ROI_SCORE_CLS ;
 *   max_overlaps (B, N) f32 ; gt_assignment (B, N) i64 ; sampled_inds (B, R) i64
 *   limits: 1 <= N <= BTC_ROI_TARGETS_MAX_N, 1 <= R <= BTC_ROI_TARGETS_MAX_R, G >= 1, B >= 1, every element count below 2^31
 * Every operation below is one float32 operation rounded on its own (no fused multiply-add) unless it says double; `/` is the
 * correctly rounded division; sinf, cosf are the device library's (not correctly rounded: compare with a bound); a comparison with NaN
 * is false, and max / min / clamp hand a NaN operand on, as torch's do.
 *
 * ==== matching, per (scene, roi n, box g)
 *   o      = box_overlap(roi, box) of csrc/iou3d_dev.h: the bits btc_boxes_pairwise_bev mode 0 gives
 *   hmax = z + dz / 2, hmin = z - dz / 2 of either box ; h = max(min(hmax_a, hmax_b) - max(hmin_a, hmin_b), 0)
 *   o3 = o * h ; vol = (dx * dy) * dz ; iou = o3 / max((vol_a + vol_b) - o3, 1e-6f)
 *   by_class: a pair with (int64) box[7] != roi_labels[n] is skipped without computing its overlap and takes the value -1
 *   max_overlaps[n], gt_assignment[n] = the largest value and its box; among equal values the LOWEST box index wins (a NaN counts as
 *   the largest).  by_class: a best value below 0 (no same-class box) becomes overlap 0 and box 0
 * ==== sampling (skipped with sampled_in), per scene, ov = max_overlaps; thresholds are the float32 values of cfg
 *   fg: ov >= fg_thresh ; easy: ov < cls_bg_lo ; hard: ov < reg_fg && ov >= cls_bg_lo ; n_fg, n_easy, n_hard their sizes, n_bg = n_easy + n_hard
 *   fg_this  = n_bg > 0 ? min(n_fg, fg_quota) : (n_fg > 0 ? R : 0) ; m = R - fg_this
 *   hard_num = n_hard > 0 && n_easy > 0 ? min((long) floor((double) m * hard_bg_ratio), n_hard) : (n_hard > 0 ? m : 0)
 *   fg_order : the foreground members ranked by (uniforms[b, 0, i], i) ascending -- a stable order (the torch route's plain sort leaves
 *              ties among foreground keys undefined); only the first n_fg ranks are ever read
 *   hard_list, easy_list: the set's members in ascending index, then the non-members in ascending index
 *   draw(row, n)[j] = min((long) floor((double) uniforms[b, row, j] * (double) n), max(n, 1) - 1), not below 0
 *   slot j < fg_this : n_bg > 0 ? fg_order[min(j, N - 1)] : fg_order[draw(1, n_fg)[j]]                 (no background: with replacement)
 *   other slots      : j - fg_this < hard_num ? hard_list[draw(2, n_hard)[j]] : easy_list[draw(3, n_easy)[j]]
 * ==== gather and labels, per slot j with s = sampled_inds[j], a = gt_assignment[s]
 *   rois_out = rois[s] ; gt_of_rois_src = gt_boxes[a] ; gt_iou_of_rois = iou = ov[s] ; roi_scores_out, roi_labels_out likewise
 *   reg_valid_mask = iou > reg_fg
 *   roi_iou: iou > cls_fg ? 1 : iou < cls_bg ? 0 : (iou - cls_bg) * inv, inv = 1.0f / cls_span: the float32 reciprocal torch's device
 *            backend forms for a division by a host scalar (btcdet_hip_heads.h); a CPU run divides
 *   cls    : iou > cls_fg ? 1 : 0, and -1 where iou > cls_bg && iou < cls_fg
 * ==== canonical transform, two_pi = float32(2 pi), pi = float32(pi), mod(x) = fmodf(x, two_pi), + two_pi when that is negative
 *   ry = mod(rois_out[6]) ; lx = gt[0] - roi[0], ly = gt[1] - roi[1], lz = gt[2] - roi[2] ; lh = gt[6] - ry
 *   c = cosf(-ry), s = sinf(-ry) ; x' = lx * c - ly * s ; y' = lx * s + ly * c                         (each product and sum on its own)
 *   hd = mod(lh) ; if hd > float32(pi / 2) && hd < float32(3 pi / 2): hd = mod(hd + pi) ; if hd > pi: hd = hd - two_pi ;
 *   hd = clamp(hd, -float32(pi / 2), float32(pi / 2))
 *   gt_of_rois = (x', y', lz, gt[3], gt[4], gt[5], hd, gt[7])
 * Compared on the GPU against the torch route (tests/test_hip_roi_targets_device.py): every output but x', y' holds the torch route's
 * bits on every listed case; x', y' are held to the bound derived in tests/roi_targets_ref.py.
 *
 * Launch structure, ONE launch: workgroups of BTC_ROI_TARGETS_THREADS threads tile (scene, block of BTC_ROI_TARGETS_TILE rois), tiles =
 * ceil(N / BTC_ROI_TARGETS_TILE) per scene; the BTC_ROI_TARGETS_LANES lanes of a roi take boxes lane, lane + LANES, ... and meet in a
 * butterfly whose comparison is a total order, so the result does not depend on the meeting order.  max_overlaps / gt_assignment leave
 * with agent-scope stores; the workgroup that completes its scene (the last-arriver protocol of csrc/btc_common.h on the scene's
 * counter) reads them back into LDS and runs that scene's sampling, gather, labels and transform.  Nothing waits on another workgroup.
 * Workspace: btc_roi_targets_ws_bytes(B, N) = B counters of 4 bytes, rounded up to 256 bytes (0 for refused B, N); ALL of it is zero on
 * entry and left zero on exit.  Memory past it is never touched.
 *
 * Refused before any launch (BTC_EINVAL, nothing written, nothing enqueued): a violated limit, a NULL among rois / roi_scores /
 * roi_labels / gt_boxes / cfg / the eleven outputs / ws, both or neither of uniforms / sampled_in, R or fg_quota outside their ranges
 * (0 <= fg_quota <= R), an unknown score_type, a workspace below btc_roi_targets_ws_bytes(B, N). */
#ifndef BTCDET_HIP_ROI_TARGETS_H
#define BTCDET_HIP_ROI_TARGETS_H

#include <stddef.h>
#include <stdint.h>

#define BTC_ROI_TARGETS_MAX_N 1024
#define BTC_ROI_TARGETS_MAX_R 1024
#define BTC_ROI_TARGETS_THREADS 256
#ifndef BTC_ROI_TARGETS_LANES
#define BTC_ROI_TARGETS_LANES 16
#endif
#define BTC_ROI_TARGETS_TILE (BTC_ROI_TARGETS_THREADS / BTC_ROI_TARGETS_LANES)

#define BTC_ROI_SCORE_ROI_IOU 0
#define BTC_ROI_SCORE_CLS 1

#ifdef __cplusplus
extern "C" {
#endif

/* host memory; the thresholds are float32(the configured double); fg_thresh = min(REG_FG_THRESH, CLS_FG_THRESH);
 * cls_span = float32(CLS_FG_THRESH - CLS_BG_THRESH), the difference formed in double; fg_quota = int(round(FG_RATIO * R)) */
typedef struct BtcRoiTargetsConfig {
  int32_t R, fg_quota, by_class, score_type;
  float reg_fg, cls_fg, cls_bg, cls_bg_lo, fg_thresh;
  float cls_span;
  double hard_bg_ratio;
} BtcRoiTargetsConfig;

size_t btc_roi_targets_ws_bytes(int B, int N);
int btc_roi_targets(const float* rois, const float* roi_scores, const int64_t* roi_labels, const float* gt_boxes, const float* uniforms,
                    const int64_t* sampled_in, int B, int N, int G, const BtcRoiTargetsConfig* cfg, float* rois_out, float* gt_of_rois,
                    float* gt_of_rois_src, float* gt_iou_of_rois, float* roi_scores_out, int64_t* roi_labels_out,
                    int64_t* reg_valid_mask, void* rcnn_cls_labels, float* max_overlaps, int64_t* gt_assignment,
                    int64_t* sampled_inds, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
