/* btcdet_hip_bestmatch.h -- best-match templates placed into the boxes of a resident batch, entry point of libbtcdet_hip.so (gfx950);
 * the fourth public header beside btcdet_hip.h, btcdet_hip_infer.h and btcdet_hip_augment.h (csrc/best_match.hip).
 *
 * Same common rules as btcdet_hip.h: every pointer is a DEVICE pointer unless its name starts with h_; the caller allocates every
 * buffer; `stream` is a hipStream_t (NULL = the default stream) and every call only enqueues work on it; an entry point returns
 * BTC_OK or a BTC_E* code, with the text in btc_last_error(), and never exits the process.
 *
 * What is replaced: the point half of the reference's MltBestMatchQuerier.__call__ without ABLATION
 * (btcdet/datasets/augmentor/multi_best_match_querier.py:50-98,278-296) and the world transforms that follow it in the queue, for a
 * whole batch: `bm_points` = for every ground-truth and pasted box its best-match template, rotated by the box heading, moved to the
 * box centre, then flipped, scaled and rotated with the scene.  The templates live in one resident array (`bank`, TemplateBank of
 * btcdet_amd/device_augmentor.py); which template goes where is O(boxes) and comes from the host as a plan
 * (DeviceAugmentor.plan).  The results equal the host chain's bit for bit.
 *
 * ---- the plan
 *   placements     placement p of n_placements is the rows [bm_first[p], bm_first[p] + bm_rows[p]) of `bank` (bank_rows, 3) f32 and
 *                  bm_place[8 p .. 8 p + 7] = c, ms, s, cx, cy, cz, 0, 0: c = cos(yaw), s = sin(yaw), ms = -1.0 * s as the host's
 *                  get_yaw_rotation forms them from the float32 heading (no device cosf), (cx, cy, cz) the box centre.
 *                  Scene b of `batch` owns the placements [bm_offsets[b], bm_offsets[b+1]).
 *   rows           bm_row_offsets (n_placements + 1) i32 = the exclusive prefix of bm_rows: output row i belongs to the placement p
 *                  with bm_row_offsets[p] <= i < bm_row_offsets[p+1] and is template row t = i - bm_row_offsets[p] of it.  The host
 *                  knows every output row's position; n_out = bm_row_offsets[n_placements].
 *   arithmetic     row (x, y, z) of the template, every product and sum rounded to float32 on its own (nothing fused):
 *                    x' = (((0 + x*c) + y*ms) + z*0) + cx
 *                    y' = (((0 + x*s) + y*c ) + z*0) + cy
 *                    z' = (((0 + x*0) + y*0 ) + z*1) + cz
 *                  which is np.einsum("nj,ij->ni", t, R) + box[:3] for float32 operands, R = [[c, ms, 0], [s, c, 0], [0, 0, 1]]:
 *                  einsum accumulates from +0, which decides the sign of a zero result (a row of -0.0 products gives +0.0;
 *                  tests/test_best_match_cpu.py holds the restatement to np.einsum itself).
 *   op program     then the scene's op program of btcdet_hip_augment.h, ops rows [op_offsets[b], op_offsets[b+1]), in registers as
 *                  btc_world_transform runs it: the rotation form comes from the op's flag (flag != 0: the rounded chain of a set
 *                  below 45 rows), which the host sets from the scene's total bm_points row count.
 *
 * ---- btc_place_templates: one launch, one thread per output row, no workspace, no atomics, no memset
 *   out (n_out, out_ld) f32: out_ld == 3 writes x, y, z; out_ld == 4 writes float(scene), x, y, z (the form collate gives bm_points)
 * Every row < n_out is written and no row >= n_out, whatever the device arrays say.  A template row outside [0, bank_rows), or one at
 * or past its placement's bm_rows, is written as zeros instead of being read.
 * Refused before any launch (BTC_EINVAL, nothing written): out_ld not 3 or 4, batch < 1, a negative count, n_out >= 2^31, a NULL
 * bm_offsets / bm_row_offsets / op_offsets, NULL bank / bm_first / bm_rows / bm_place with n_placements > 0, NULL out with n_out > 0.
 * ops may be NULL: no op.  n_out == 0 launches nothing and returns BTC_OK. */
#ifndef BTCDET_HIP_BESTMATCH_H
#define BTCDET_HIP_BESTMATCH_H

#include <stddef.h>
#include <stdint.h>

#include "btcdet_hip_augment.h"

#ifdef __cplusplus
extern "C" {
#endif

int btc_place_templates(const float* bank, long long bank_rows,
                        const int32_t* bm_first, const int32_t* bm_rows, const float* bm_place,
                        const int32_t* bm_offsets, const int32_t* bm_row_offsets, int n_placements, int batch,
                        const float* ops, const int32_t* op_offsets,
                        long long n_out, int out_ld, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
