/* btcdet_hip_heads.h -- the anchor head's targets and boxes: fused target assignment + box encoding, and box decoding with the direction
 * bins, entry points of libbtcdet_hip.so (gfx950); the ninth public header beside btcdet_hip.h, btcdet_hip_infer.h,
 * btcdet_hip_augment.h, btcdet_hip_bestmatch.h, btcdet_hip_frames.h, btcdet_hip_gtdb.h, btcdet_hip_templates.h and btcdet_hip_infos.h
 * (csrc/anchor_targets.hip).
 *
 * Same common rules as btcdet_hip.h: every pointer is a DEVICE pointer unless its name starts with h_; the caller allocates every
 * buffer; `stream` is a hipStream_t (NULL = the default stream) and every call only enqueues work on it; an entry point returns
 * BTC_OK or a BTC_E* code, with the text in btc_last_error(), and never exits the process.  ws contents are arbitrary on entry;
 * results are the same from run to run (the only atomics are integer maxima, whose outcome does not depend on the order of arrival).
 *
 * What is replaced: the reference's AxisAlignedTargetAssigner.assign_targets (dense_heads/target_assigner/
 * axis_aligned_target_assigner.py:36-213, the single-head path with POS_FRACTION < 0, MATCH_HEIGHT false, NORM_BY_NUM_EXAMPLES false)
 * with ResidualCoder.encode_torch (utils/box_coder_utils.py), and AnchorHeadTemplate.generate_predicted_boxes
 * (anchor_head_template.py:227-274: ResidualCoder.decode_torch and the direction-bin correction), code size 7.
 *
 * ==== btc_anchor_targets: labels, regression targets and weights of every (scene, anchor)
 *   anchors (A, 7) f32 [x, y, z, dx, dy, dz, r]: location slowest, then the `slots` anchors of a location; A a multiple of slots
 *   h_slot_cfg (slots) i32 HOST: the anchor-class configuration of each slot, in [0, ncfg); slots <= BTC_HEADS_MAX_SLOTS
 *   h_matched, h_unmatched (ncfg) f32 HOST: the thresholds of each configuration; 1 <= ncfg <= BTC_HEADS_MAX_CFGS
 *   h_class_cfg (num_class + 1) i32 HOST: ground-truth class id -> configuration, -1 for none; num_class < BTC_HEADS_MAX_CLASSES.
 *     Entry 0 is the caller's to fill: the reference indexes class_names[c - 1], so class 0 lands on the LAST class name.
 *   gt (B, M, 8) f32 [x, y, z, dx, dy, dz, r, class]; zero rows pad the tail of a scene
 *   labels (B, A) i32 ; targets (B, A, 7) f32 ; weights (B, A) f32 -- every element is written by the call
 * Values are finite (a NaN is not defined here).  Every operation below is one float32 operation rounded on its own (no fused
 * multiply-add); `/` is the correctly rounded division, sqrt the correctly rounded square root.
 *   rows of a scene   s_j = (((((x + y) + z) + dx) + dy) + dz) + r of row j, summed in that order.  n_b = 0 for M == 0, else
 *                     max(1, 1 + the last j with s_j != 0): trailing padding is trimmed, row 0 is kept even when it is padding
 *   class             c_j = (int)class (truncation); cfg_j = h_class_cfg[c_j] for 0 <= c_j <= num_class, else -1 (the torch route
 *                     raises for such an id).  Box j is offered only to the anchors whose slot has configuration cfg_j
 *   footprint         q = r * (1/pi) ; lp = r - floor(q + 0.5) * pi ; snapped = |lp| < pi/4     pi, 1/pi = 1.0f / pi and pi/4 in float32
 *                     (wx, wy) = snapped ? (dx, dy) : (dy, dx)
 *                     x0 = x - wx/2, y0 = y - wy/2, x1 = x + wx/2, y1 = y + wy/2 ; area = (x1 - x0) * (y1 - y0)
 *                     `r * (1/pi)` is the form torch's device backend gives `r / np.pi`: a division by a host scalar is a
 *                     multiplication by its float32 reciprocal there (compared on the GPU: all of 2^20 random values equal the
 *                     product bit for bit, 15 % of them differ from the quotient); the reference run on a CPU divides.  The two
 *                     decide differently only for a heading within rounding of pi/4 from an axis
 *   overlap           w = max(min(ax1, gx1) - max(ax0, gx0), 0) ; h likewise in y ; inter = w * h
 *                     iou = inter / max((area_a + area_g) - inter, 1e-6)                          iou >= 0 always
 *   best box          best_a = max_j iou(a, j) over the offered boxes, j_a = the smallest such j (numpy's argmax)
 *   forced anchors    top_j = max over the anchors of cfg_j of iou(a, j).  Anchor a is forced when iou(a, j) == top_j > 0 for some
 *                     offered j: a box no anchor touches forces nothing, every anchor that ties is forced
 *   labels            no offered box: 0.  Else forced: c of box j_a (the class of the anchor's OWN best box, not of the box it
 *                     ties -- the reference's quirk); else best_a < unmatched: 0; else best_a >= matched: c of box j_a; else -1
 *   targets           labels > 0: ResidualCoder.encode_torch of box g = j_a against anchor a, sizes clamped at 1e-5 first:
 *                     diag = sqrt(dxa*dxa + dya*dya)
 *                     [(xg - xa) / diag, (yg - ya) / diag, (zg - za) / dza, log(dxg / dxa), log(dyg / dya), log(dzg / dza), rg - ra]
 *                     else seven zeros.  log is the device library's logf (not correctly rounded: compare it with a tolerance)
 *   weights           labels > 0 ? 1.0 : 0.0
 * Launch structure, three launches:
 *   prepare  one workgroup per scene: n_b and the scene's M per-box maxima in ws cleared
 *   top      one thread per (scene, anchor), 256 per workgroup, a workgroup inside one scene.  The scene's boxes are staged in LDS
 *            as snapped footprints with area and configuration, 64 at a time (no bound on M); per box one wave-level maximum of the
 *            overlaps' bit patterns (iou >= 0: the unsigned order is the float order), one LDS maximum per wave with a hit and one
 *            global atomic maximum per (workgroup, box with a hit)
 *   assign   the same staging; every overlap is recomputed THROUGH THE SAME DEVICE FUNCTION, so `iou == top` compares identical
 *            bits; each thread tracks its best box, decides forced / background / positive and writes its label, target row, weight
 * The bound: at KITTI size (A = 70 400, B = 2, a few dozen boxes) a few million overlap evaluations and 5 MB written -- microseconds
 * of work on this device; the call is expected to be bound by the three launches, not by throughput.  No profile of the kernels alone
 * has been taken to confirm that; tools/anchor_targets_bench.py records the time per call on the host clock (23.4 us at that size, the
 * order of three launches, against 2 420 us and 283 launches of the torch formulation; profiles/anchor_targets_bench.json).
 * btc_anchor_targets_ws_bytes(B, M): B row counts and B * M maxima, each block 256-byte aligned; 0 for refused arguments.
 * Refused before any launch (BTC_EINVAL, nothing written): B < 1, A < 0, M < 0, slots < 1 or above BTC_HEADS_MAX_SLOTS, A not a
 * multiple of slots, ncfg < 1 or above BTC_HEADS_MAX_CFGS, num_class < 0 or >= BTC_HEADS_MAX_CLASSES, an h_slot_cfg entry outside
 * [0, ncfg), an h_class_cfg entry outside [-1, ncfg), a NULL h_slot_cfg / h_matched / h_unmatched / h_class_cfg / ws, NULL anchors /
 * labels / targets / weights with A > 0, NULL gt with M > 0 and A > 0, B * max(A, M) * 8 >= 2^31, a workspace below
 * btc_anchor_targets_ws_bytes(B, M).  A == 0 launches nothing; M == 0 makes every anchor background.
 *
 * ==== btc_decode_anchor_boxes: the head's boxes from its regression output
 *   box_preds (B, A, 7) f32 ; anchors (A, 7) f32 ; dir_cls_preds (B, A, bins) f32 or NULL ; boxes (B, A, 7) f32
 * One launch, one thread per (scene, anchor): each input is read once, the output written once.  Arithmetic, one float32 operation
 * per step, t = box_preds row, a = anchor row:
 *   diag = sqrt(dxa*dxa + dya*dya)
 *   x = t0 * diag + xa ; y = t1 * diag + ya ; z = t2 * dza + za            (product, then sum)
 *   dx = exp(t3) * dxa ; dy = exp(t4) * dya ; dz = exp(t5) * dza           (the device library's expf: compare with a tolerance)
 *   rot = t6 + ra
 * and with dir_cls_preds, period = 2*pi/bins formed in double and rounded to float32, inv = 1.0f / period:
 *   v = rot - dir_offset ; q = v * inv ; lp = v - floor(q + dir_limit_offset) * period
 *   rot = (lp + dir_offset) + period * (float)k,  k = the smallest index of the largest logit
 * `v * inv` again is the form of torch's device backend for `v / period`; a CPU run divides, which can move floor() only for a
 * quotient within rounding of an integer.
 * Refused before any launch (BTC_EINVAL, nothing written): B < 1, A < 0, B * A * 8 >= 2^31, NULL box_preds / anchors / boxes with
 * A > 0, bins < 1 with dir_cls_preds.  A == 0 launches nothing. */
#ifndef BTCDET_HIP_HEADS_H
#define BTCDET_HIP_HEADS_H

#include <stddef.h>
#include <stdint.h>

#include "btcdet_hip.h"

#define BTC_HEADS_MAX_SLOTS 64
#define BTC_HEADS_MAX_CFGS 16
#define BTC_HEADS_MAX_CLASSES 64

#ifdef __cplusplus
extern "C" {
#endif

size_t btc_anchor_targets_ws_bytes(int B, int M);
int btc_anchor_targets(const float* anchors, int A, int slots, const int32_t* h_slot_cfg, int ncfg, const float* h_matched,
                       const float* h_unmatched, const int32_t* h_class_cfg, int num_class, const float* gt, int B, int M,
                       int32_t* labels, float* targets, float* weights, void* ws, size_t ws_bytes, void* stream);

int btc_decode_anchor_boxes(const float* box_preds, const float* anchors, const float* dir_cls_preds, int B, int A, int bins,
                            float dir_offset, float dir_limit_offset, float* boxes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
