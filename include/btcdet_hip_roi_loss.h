/* btcdet_hip_roi_loss.h -- the ROI head's loss, fused: forward in one launch, backward in one launch; entry points of
 * libbtcdet_hip.so (gfx950); the twelfth public header, beside btcdet_hip_roi_targets.h whose outputs it consumes without conversion
 * (csrc/roi_loss.hip).
 *
 * Same common rules as btcdet_hip.h: every pointer is a DEVICE pointer; the caller allocates every buffer; `stream` is a hipStream_t
 * (NULL = the default stream) and every call only enqueues work on it; an entry point returns BTC_OK or a BTC_E* code, with the text in
 * btc_last_error(), and never exits the process.  No memset, no read-back, no atomics on floating-point values: the same inputs give
 * the same bits.
 *
 * What is replaced: ConvHead.get_loss -> rcnn_cls_loss / rcnn_reg_loss of btcdet_amd/roi_targets.py (the reference's
 * RoIHeadTemplate.get_loss, roi_heads/roi_head_template.py:134-229, with ResidualCoder, WeightedSmoothL1Loss and get_corner_loss_lidar),
 * CLS_LOSS BinaryCrossEntropy, REG_LOSS smooth-l1, code size 7, no sin/cos angle code -- a sigmoid and a binary cross-entropy, two clones
 * with in-place edits, an encode and a decode, a rotation, three corner expansions, two norms, a min, two smooth-L1s and masked sums, and
 * an autograd twin for each.
 *
 *   N = B * R sampled rois, flat: the normalisers are global, not per scene
 *   rcnn_cls (N) f32 ; rcnn_reg (N, 7) f32 ; rois (N, 7) f32
 *   gt_of_rois, gt_of_rois_src (N, gt_width) f32, gt_width >= 7: only columns 0..6 are read (btc_roi_targets writes 8)
 *   reg_valid_mask (N) i64: foreground where > 0
 *   cls_labels (N): f32 with label_kind BTC_ROI_SCORE_ROI_IOU (soft labels in [0, 1]), i64 with BTC_ROI_SCORE_CLS (-1 ignore, 0, 1)
 *   out (5) f32 = cls | reg | corner | reg + corner | total ; norms (2) f32 = 1 / n_valid, 1 / n_fg
 * Every operation below is one float32 operation rounded on its own (no fused multiply-add) unless it says double; `/` is the
 * correctly rounded division; expf, logf, sqrtf, sinf, cosf are the device library's (not correctly rounded: compare with a bound); a
 * comparison with NaN is false.
 *
 * ==== btc_roi_loss_fwd
 *   class term  over valid rois (label >= 0), x = rcnn_cls, t = max((float) label, 0):
 *                 e = expf(-|x|) ; r = 1 / (1 + e) ; p = x >= 0 ? r : e * r ; om = 1 - p               (p = sigmoid(x), never an overflow)
 *                 term = (t - 1) * max(logf(om), -100) - t * max(logf(p), -100)
 *               torch's binary_cross_entropy on a float32 sigmoid, its clamp at -100 included: where p rounds to 1.0f (x above
 *               24 ln 2 = 16.64) the term is 100 * (1 - t), and where p underflows it is 100 * t.  Part of the contract.
 *               n_valid = max(#valid, 1), over all N
 *   regression  over foreground rois, r_k = rcnn_reg, a_k = max(roi_k, 1e-5f) and g_k = max(gt_of_rois_k, 1e-5f) for k = 3..5,
 *               beta = float32(1/9):
 *                 diag = sqrtf(a_3 * a_3 + a_4 * a_4)
 *                 v_0 = gt_0 / diag ; v_1 = gt_1 / diag ; v_2 = gt_2 / a_5 ; v_k = logf(g_k / a_k), k = 3..5 ; v_6 = gt_6
 *                 d = r_k - v_k ; n = |d| ; term = n < beta ? 0.5 * (n * n) / beta : n - 0.5 * beta
 *               (the anchor is the roi with its centre and heading zeroed, so the encoder's subtractions are exact and left out); a
 *               column whose v is NaN contributes 0 and gets gradient 0.  These max are x < c ? c : x: a NaN dim is handed on, as
 *               torch's clamp_min does, and its column is skipped (the two max of the class term drop a NaN operand instead).
 *               No code weights.  n_fg = max(#foreground, 1), over all N
 *   corner      only with with_corner, over foreground rois; s_k = roi_k, k = 3..5, UNCLAMPED (the torch route clamps a clone);
 *               pi = float32(pi); w = gt_of_rois_src:
 *                 dg = sqrtf(s_3 * s_3 + s_4 * s_4) ; bx = r_0 * dg ; by = r_1 * dg ; bz = r_2 * s_5
 *                 l_k = expf(r_k) * s_k, k = 3..5 ; h = r_6 + roi_6
 *                 c = cosf(roi_6) ; s = sinf(roi_6)                                                     (roi_6 is not reduced)
 *                 cx = (bx * c - by * s) + roi_0 ; cy = (bx * s + by * c) + roi_1 ; cz = bz + roi_2
 *               corner j = 0..7 with signs (sx, sy, sz) in the reference's order (+ + -) (+ - -) (- - -) (- + -) (+ + +) (+ - +) (- - +) (- + +):
 *                 x = l_3 * (0.5 sx) ; y = l_4 * (0.5 sy) ; z = l_5 * (0.5 sz)
 *                 R_x = x * cosf(h) - y * sinf(h) ; R_y = x * sinf(h) + y * cosf(h) ; P = (R_x + cx, R_y + cy, z + cz)
 *                 Q(a) likewise from dims w_3..5, heading a and centre w_0..2 ; Q = Q(w_6), Q' = Q(w_6 + pi), the half-turn twin
 *                 D = P - Q ; dist(Q) = sqrtf((D_x * D_x + D_y * D_y) + D_z * D_z) ; m = min(dist(Q), dist(Q'))
 *                 term_j = 0.125 * (m < 1 ? (0.5 * m) * m : m - 0.5)
 *   sums        every term enters a DOUBLE sum per quantity (class, regression, corner; each of the eight term_j on its own), per
 *               workgroup, then over the workgroups in a fixed order
 *   out[0]      = float32(S_cls * (1 / n_valid) * cls_weight) in double ; out[1] = float32(S_reg * (1 / n_fg) * reg_weight) ;
 *   out[2]      = float32(S_corner * (1 / n_fg) * corner_weight), 0 without with_corner ; with no foreground roi out[1] = out[2] = 0
 *   out[3]      = out[1] + out[2] ; out[4] = out[0] + out[3], both in float32, the order in which get_loss adds them
 *   norms       = float32(1 / n_valid), float32(1 / n_fg) from double, kept for the backward
 * Excluded entries: rcnn_cls of an ignored roi, and rcnn_reg / rois / gt_of_rois / gt_of_rois_src of a non-foreground roi are never
 * read: NaN placed there changes no output bit.
 * Launch structure, ONE launch: workgroups of BTC_ROI_LOSS_THREADS threads; BTC_ROI_LOSS_LANES lanes share a roi (1: one thread walks the
 * eight corners; 8: one lane per corner, lane 0 also takes the class and regression terms), so a workgroup covers BTC_ROI_LOSS_TILE
 * rois at a time; tiles = min(max(ceil(N / TILE), 1), BTC_ROI_LOSS_MAX_TILES) workgroups, tile g takes rois g * TILE + i, then strides by
 * tiles * TILE (one sweep covers tiles * TILE rois).  A workgroup stores five doubles (three sums, two counts); the last workgroup to
 * arrive (the last-arriver protocol of csrc/btc_common.h) adds them in a fixed order and writes out and norms.
 * Workspace: btc_roi_loss_ws_bytes(N) = 256 + tiles * 40 bytes (0 for a refused N).  Its first 256 bytes are zero on entry and left
 * zero on exit; the rest may hold anything.
 * N == 0 is valid: out = 0, norms = 1, nothing is read.
 *
 * ==== btc_roi_loss_bwd
 *   grad_total (1) f32: the upstream gradient of out[4], read on the device ; norms (2) from the forward
 *   d_cls (N), d_reg (N, 7): EVERY element is written -- zeros at ignored rois (d_cls) and at non-foreground rois (d_reg) -- so the
 *   caller allocates them uninitialised.
 * ONE launch, the forward's lanes per roi, no grid cap; the per-element terms are recomputed from the inputs.
 *   s_0 = (grad_total * norms[0]) * cls_weight ; s_1 = (grad_total * norms[1]) * reg_weight ; s_2 = ((grad_total * norms[1]) * corner_weight) * 0.125
 *   d_cls  pq = om * p ; d = ((p - t) / max(pq, 1e-12f)) * pq ; d_cls = s_0 * d      torch's two backward formulas composed: exactly 0
 *          where p rounds to 1.0f or underflows to 0
 *   d_reg  gr = n < beta ? d / beta : sign(d) ; d_reg_k = s_1 * gr, so a column with n >= beta holds exactly +-s_1 where no corner term
 *          is requested; with with_corner the corner part below is ADDED to it, d_reg_k = s_1 * gr + corner_k
 *   corner per corner j the nearer twin is taken; on an exact tie of the two distances the UNFLIPPED twin takes the whole gradient
 *          (torch's min splits it in half).  With D and m of that twin:
 *            G = m < 1 ? D : D / m            (quadratic branch: the difference itself, no division, 0 at m = 0; linear: D / m)
 *            qx = G_x * cosf(h) + G_y * sinf(h) ; qy = G_y * cosf(h) - G_x * sinf(h)
 *            u_j = (G_x, G_y, G_z, qx * (0.5 sx), qy * (0.5 sy), G_z * (0.5 sz), G_y * R_x - G_x * R_y)
 *          the seven components are summed over the corners in float32 as ((u_0 + u_4) + (u_2 + u_6)) + ((u_1 + u_5) + (u_3 + u_7)) = U:
 *            ex = U_0 * c + U_1 * s ; ey = U_1 * c - U_0 * s
 *            corner_0 = s_2 * (ex * dg) ; corner_1 = s_2 * (ey * dg) ; corner_2 = s_2 * (U_2 * s_5)
 *            corner_k = s_2 * (U_k * l_k), k = 3..5 ; corner_6 = s_2 * U_6
 * Nothing of the inputs is written.
 *
 * Refused before any launch (BTC_EINVAL, nothing written, nothing enqueued): N < 0, N * 8 >= 2^31, gt_width < 7, a label_kind other
 * than BTC_ROI_SCORE_ROI_IOU / BTC_ROI_SCORE_CLS, with N > 0 a NULL rcnn_cls / rcnn_reg / rois / gt_of_rois / gt_of_rois_src /
 * reg_valid_mask / cls_labels, a NULL out / norms / ws (forward), a workspace below btc_roi_loss_ws_bytes(N), a NULL norms /
 * grad_total, and with N > 0 a NULL d_cls / d_reg (backward). */
#ifndef BTCDET_HIP_ROI_LOSS_H
#define BTCDET_HIP_ROI_LOSS_H

#include <stddef.h>
#include <stdint.h>

#include "btcdet_hip_roi_targets.h"

#define BTC_ROI_LOSS_THREADS 256
#ifndef BTC_ROI_LOSS_LANES
#define BTC_ROI_LOSS_LANES 1
#endif
#define BTC_ROI_LOSS_TILE (BTC_ROI_LOSS_THREADS / BTC_ROI_LOSS_LANES)
#define BTC_ROI_LOSS_MAX_TILES 512

#ifdef __cplusplus
extern "C" {
#endif

size_t btc_roi_loss_ws_bytes(int N);
int btc_roi_loss_fwd(const float* rcnn_cls, const float* rcnn_reg, const float* rois, const float* gt_of_rois, const float* gt_of_rois_src,
                     int gt_width, const int64_t* reg_valid_mask, const void* cls_labels, int label_kind, int N, int with_corner,
                     float cls_weight, float reg_weight, float corner_weight, float* out, float* norms, void* ws, size_t ws_bytes,
                     void* stream);
int btc_roi_loss_bwd(const float* rcnn_cls, const float* rcnn_reg, const float* rois, const float* gt_of_rois, const float* gt_of_rois_src,
                     int gt_width, const int64_t* reg_valid_mask, const void* cls_labels, int label_kind, int N, int with_corner,
                     float cls_weight, float reg_weight, float corner_weight, const float* norms, const float* grad_total, float* d_cls,
                     float* d_reg, void* stream);

#ifdef __cplusplus
}
#endif
#endif
