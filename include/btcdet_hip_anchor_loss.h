/* btcdet_hip_anchor_loss.h -- the anchor head's loss, fused: forward in one launch, backward in one launch; entry points of
 * libbtcdet_hip.so (gfx950); the tenth public header, beside btcdet_hip_heads.h whose outputs it consumes without conversion
 * (csrc/anchor_loss.hip).
 *
 * Same common rules as btcdet_hip.h: every pointer is a DEVICE pointer; the caller allocates every buffer; `stream` is a hipStream_t
 * (NULL = the default stream) and every call only enqueues work on it; an entry point returns BTC_OK or a BTC_E* code, with the text in
 * btc_last_error(), and never exits the process.  No memset, no read-back, no atomics on floating-point values: the same inputs give
 * the same bits.
 *
 * What is replaced: the reference's AnchorHeadTemplate.get_loss (dense_heads/anchor_head_template.py:102-225: get_cls_layer_loss,
 * get_box_reg_layer_loss) with SigmoidFocalClassificationLoss, WeightedSmoothL1Loss and WeightedCrossEntropyLoss of
 * utils/loss_utils.py, single head, code size 7, no sin/cos angle code -- a one-hot tensor over (B, A, C + 1), the anchors repeated B
 * times, two cats for the heading products, several dozen elementwise launches and their autograd twins.
 *
 *   cls_preds (B, A, C) f32 ; box_preds (B, A, 7) f32 ; dir_cls_preds (B, A, bins) f32, or NULL with bins = 0
 *   box_cls_labels (B, A) i32: -1 ignore, 0 background, otherwise a class id (what btc_anchor_targets writes) ; box_reg_targets (B, A, 7) f32
 *   anchors (A, 7) f32, not repeated per scene (only column 6, the heading, is read)
 *   out (4) f32 ; norms (B) f32 ; limits: 1 <= C < BTC_HEADS_MAX_CLASSES, 0 <= bins <= BTC_ANCHOR_LOSS_MAX_BINS
 * Every operation below is one float32 operation rounded on its own (no fused multiply-add) unless it says double; `/` is the
 * correctly rounded division; expf, logf, log1pf, sinf, cosf are the device library's (not correctly rounded: compare with a bound).
 *
 * ==== btc_anchor_loss_fwd
 *   normaliser  n_b = max(#{a : label(b, a) > 0}, 1), per scene
 *   class term  over cared anchors (label >= 0) and every class c in 1..C, x the logit of class c, t = (label' == c), label' = the
 *               label, except that every positive label counts as 1 when C == 1:
 *                 e = expf(-|x|) ; r = 1 / (1 + e) ; p = x >= 0 ? r : e * r ; om = 1 - p            (p = sigmoid(x), never an overflow)
 *                 pt = t ? om : p ; alpha_t = t ? 0.25 : 0.75
 *                 bce = (max(x, 0) - (t ? x : 0)) + log1pf(e)                                       (the difference is exact)
 *                 term = (alpha_t * (pt * pt)) * bce
 *               `om = 1 - p` is formed in float32 as the reference forms it, so both routes round a confident positive alike
 *   location    over positives (label > 0), the 7 columns k, p_k of box_preds, t_k of box_reg_targets, beta = float32(1/9):
 *                 k < 6: u = p_k, v = t_k ;  k = 6: u = sinf(p_6) * cosf(t_6), v = cosf(p_6) * sinf(t_6)
 *                 d = u - v ; n = |d| ; term = n < beta ? 0.5 * (n * n) / beta : n - 0.5 * beta
 *               a column whose v is NaN contributes 0 and gets gradient 0 (the reference's where(isnan(target), pred, target)).
 *               This holds for column 6 too, where the reference's own loss is NaN (a NaN t_6 makes its prediction side NaN as well)
 *               No code weights: the reference builds them and never applies them
 *   direction   only with bins > 0, over positives, z_j the bins logits, two_pi = float32(2 pi), w = float32(2 pi / bins) formed in double:
 *                 rot = t_6 + anchor_6 ; v = rot - dir_offset ; q = v * (1 / two_pi) ; lp = v - floor(q) * two_pi
 *                 k = (int) min(max(floor(lp * (1 / w)), 0), bins - 1)                               1 / two_pi, 1 / w: float32 reciprocals
 *                 m = max_j z_j ; s = sum_j expf(z_j - m), j ascending ; term = logf(s) - (z_k - m)
 *               the two divisions are multiplications by the float32 reciprocal, the form torch's device backend gives a division by
 *               a host scalar (btcdet_hip_heads.h); a CPU run divides, which moves floor() only for a quotient within rounding of an integer
 *   sums        every term enters a DOUBLE sum per scene and quantity; S_q(b) over the scene's workgroups in ascending order
 *   out[q]      = float32( (sum_b S_q(b) / n_b) / B * weight_q ) in double, q = 0 class, 1 location, 2 direction (0 with bins = 0)
 *   out[3]      = out[0] + (out[1] + out[2]) in float32, the order in which get_loss adds them
 *   norms[b]    = float32(1 / n_b) from double, kept for the backward
 * Excluded entries: cls_preds of an ignored anchor, and box_preds / box_reg_targets / dir_cls_preds / anchors of a non-positive anchor
 * are never read: NaN placed there changes no output bit.
 * Launch structure, ONE launch: workgroups of BTC_ANCHOR_LOSS_THREADS threads, a workgroup stays inside one scene;
 * tiles = min(max(ceil(A / BTC_ANCHOR_LOSS_THREADS), 1), BTC_ANCHOR_LOSS_MAX_TILES) workgroups per scene, B * tiles in all; thread i of
 * tile g takes anchors g * THREADS + i, then strides by tiles * THREADS (one sweep covers tiles * THREADS anchors of each scene).
 * A workgroup stores four doubles (the three sums and its positive count); the last workgroup to arrive (the last-arriver protocol of
 * csrc/btc_common.h) adds each scene's partials in a fixed order and writes out and norms.
 * Workspace: btc_anchor_loss_ws_bytes(B, A) = 256 + B * tiles * 32 bytes (0 for refused B, A).  Its first 256 bytes are zero on entry
 * and left zero on exit; the rest may hold anything.
 * A == 0 is valid: out = 0, norms = 1, nothing is read.
 *
 * ==== btc_anchor_loss_bwd
 *   grad_total (1) f32: the upstream gradient of out[3], read on the device ; norms (B) from the forward
 *   d_cls (B, A, C), d_box (B, A, 7), d_dir (B, A, bins; NULL with bins = 0): EVERY element is written -- zeros at ignored anchors (d_cls)
 *   and at non-positive anchors (d_box, d_dir) -- so the caller allocates them uninitialised.
 * ONE launch, one thread per (scene, anchor); the per-element terms are recomputed from the inputs.  c_q = weight_q / (float) B on the
 * host, s_q = (grad_total * norms[b]) * c_q:
 *   d_cls  qt = t ? p : om ; g = (alpha_t * (pt * pt)) * ((2 * qt) * bce + pt) ; d = s_0 * (t ? -g : g)          (no cancellation)
 *   d_box  gr = n < beta ? d / beta : sign(d) ; k < 6: s_1 * gr ; k = 6: (s_1 * gr) * (cosf(p_6) * cosf(t_6) + sinf(p_6) * sinf(t_6))
 *          so a column of k < 6 with n >= beta holds exactly +-s_1
 *   d_dir  s_2 * (expf(z_j - m) / s - (j == k ? 1 : 0))
 * Nothing of the inputs is written; the labels keep their bits (the reference overwrites positive labels with 1 when C == 1).
 *
 * Refused before any launch (BTC_EINVAL, nothing written, nothing enqueued): B < 1, A < 0, C < 1 or C >= BTC_HEADS_MAX_CLASSES,
 * bins < 0 or bins > BTC_ANCHOR_LOSS_MAX_BINS, B * A * max(C, 7, bins) >= 2^31, with A > 0 a NULL cls_preds / box_preds /
 * box_cls_labels / box_reg_targets / anchors (dir_cls_preds with bins > 0), a NULL out / norms / ws (forward), a workspace below
 * btc_anchor_loss_ws_bytes(B, A), a NULL norms / grad_total, and with A > 0 a NULL d_cls / d_box (d_dir with bins > 0) (backward). */
#ifndef BTCDET_HIP_ANCHOR_LOSS_H
#define BTCDET_HIP_ANCHOR_LOSS_H

#include <stddef.h>
#include <stdint.h>

#include "btcdet_hip_heads.h"

#define BTC_ANCHOR_LOSS_THREADS 256
#define BTC_ANCHOR_LOSS_MAX_TILES 512
#define BTC_ANCHOR_LOSS_MAX_BINS 16

#ifdef __cplusplus
extern "C" {
#endif

size_t btc_anchor_loss_ws_bytes(int B, int A);
int btc_anchor_loss_fwd(const float* cls_preds, const float* box_preds, const float* dir_cls_preds, const int32_t* box_cls_labels,
                        const float* box_reg_targets, const float* anchors, int B, int A, int C, int bins, float cls_weight,
                        float loc_weight, float dir_weight, float dir_offset, float* out, float* norms, void* ws, size_t ws_bytes,
                        void* stream);
int btc_anchor_loss_bwd(const float* cls_preds, const float* box_preds, const float* dir_cls_preds, const int32_t* box_cls_labels,
                        const float* box_reg_targets, const float* anchors, int B, int A, int C, int bins, float cls_weight,
                        float loc_weight, float dir_weight, float dir_offset, const float* norms, const float* grad_total, float* d_cls,
                        float* d_box, float* d_dir, void* stream);

#ifdef __cplusplus
}
#endif
#endif
