/* btcdet_hip_templates.h -- the best-match (shape completion) templates of a class made from the objects of a ground-truth database
 * that already lives in HBM, entry points of libbtcdet_hip.so (gfx950); the seventh public header beside btcdet_hip.h,
 * btcdet_hip_infer.h, btcdet_hip_augment.h, btcdet_hip_bestmatch.h, btcdet_hip_frames.h and btcdet_hip_gtdb.h (csrc/template_match.hip).
 *
 * Same common rules as btcdet_hip.h: every pointer is a DEVICE pointer unless its name starts with h_; the caller allocates every
 * buffer; `stream` is a hipStream_t (NULL = the default stream) and every call only enqueues work on it; an entry point returns
 * BTC_OK or a BTC_E* code, with the text in btc_last_error(), and never exits the process.
 *
 * What is replaced: the point work of the reference's btcdet/datasets/multifindbestfit.py -- remove_voxelpnts (the chamfer filter of
 * mirror and of every greedy round), the padded one-sided chamfer maximum and the remove_outofbox + space_occ_voxelpnts bitmap per
 * (object, candidate) pair, and the greedy loop of find_multi_best_match_boxpnts.  Reading boxes, the rotation, the box IoU and its
 * top-k, the batching and the files stay with btcdet_amd/template_builder.py.
 *
 * ---- the data of one class
 *   points (n, 3) f32   the mirrored sets of all M objects, object j owning rows [seg[j][0], seg[j][0] + seg[j][1]) ; seg (M, 2) i32
 *   half (M, 3) f32     dx/2, dy/2, dz/2 of object j's box, formed in double from the box as given and rounded once
 * A set is what the algorithm below calls "mirrored": the object's rows rotated by -heading about z (in double from a host-formed cos
 * and sin, one rounding to float32), those with z > -dz/2 + bottom kept, and -- for a mirrored class -- (x, -y, z) of every kept row
 * whose nearest kept row is farther than float32(0.05) appended behind them (btc_nn_sqdist gives the distances).  Coordinates are
 * finite.  A segment that reaches outside [0, n) is clamped to it, an object or candidate index outside [0, M) counts as -1.
 *
 * ---- d2, the squared distance of two rows, everywhere in this header
 *   dx = px - qx, dy = py - qy, dz = pz - qz ;  d2 = ((dx*dx) + (dy*dy)) + (dz*dz)
 * every operation rounded to float32 on its own (the library is compiled without contraction), so a numpy restatement is exact.  The
 * reference's compiled chamfer kernel contracts the same expression to FMAs: its decisions are these wherever a distance is not within
 * rounding of a threshold.  A minimum over rows is exact in any order, and sqrt is the correctly rounded one, so nothing depends on the
 * order in which rows are visited.
 *
 * ---- btc_nn_sqdist: a segmented nearest neighbour (step 2, and the device function the greedy rounds filter with)
 *   q_points (nq, 3) f32 ; t_points (nt, 3) f32 ; pairs (P, 4) i32 = q_first, q_rows, t_first, t_rows ; out_offsets (P+1) i32, the
 *   exclusive prefix of q_rows, which the host knows: out_rows = out_offsets[P] is passed as a host scalar ; out (out_rows) f32
 * out[out_offsets[p] + r] = the smallest d2 of query row q_first + r against rows [t_first, t_first + t_rows) of t_points, +inf for an
 * empty target.  One workgroup per pair; the target goes through LDS in tiles of 256 rows that every lane reads at a wave-uniform
 * address.  Query rows outside [0, nq), target rows outside [0, nt) and destinations outside [0, out_rows) are left out.
 * Refused (BTC_EINVAL, nothing written): P < 0, nq < 0, nt < 0, out_rows < 0, NULL pairs or out_offsets with P > 0, NULL q_points with
 * nq > 0, NULL t_points with nt > 0, NULL out with out_rows > 0.
 *
 * ---- the occupancy bitmap: nx * ny bits in W = ceil(nx * ny / 32) 32-bit words, z ignored
 *   ix = floor((x - x0) / cell), iy = floor((y - y0) / cell)    (float32: one subtraction, one correctly rounded division)
 *   bit b = ix * ny + iy of word b >> 5 at position b & 31, set when 0 <= ix < nx and 0 <= iy < ny
 * x0, y0 are the minima over all sets of the class and nx, ny = ceil(extent / cell) formed by the host, so an index equal to nx or ny
 * is possible (an extent that is a whole number of cells): that row sets no bit, where the reference raises an IndexError.  The bits of
 * a word past nx * ny are 0.
 *
 * ---- btc_match_candidates: step 5, per (object i = obj[g], candidate c = cand[g][k]) pair of a batch of G objects
 *   obj (G) i32 ; cand (G, K) i32, -1 = none ; max_dist (G, K) f32 ; sel_occ (G, K, W) u32
 *   max_dist[g][k] = the maximum over i's rows of sqrt(min over c's rows of d2): 0 when i has no rows, +inf when c has none
 *   sel_occ[g][k]  = the bitmap of c's rows with |x| <= half[i][0], |y| <= half[i][1], |z| <= half[i][2] (faces inclusive)
 * For cand[g][k] == -1 (and for obj[g] == -1): max_dist = +inf and sel_occ = 0.  Every word of both outputs is written by the call: no
 * pre-fill.  A workgroup per (object, 8 candidates): the object's rows sit in registers, 4 per lane and 1024 per pass (longer objects
 * loop), the candidate's rows go through LDS in tiles of 512 and are read at a wave-uniform address; the pass that stages a row also
 * sets its bit in an LDS bitmap, which is written out whole.
 * Refused: n, M, G < 0, K < 1, nx or ny < 1, W = ceil(nx * ny / 32) > 2048, cell not > 0, G * K * W >= 2^31, NULL obj / cand /
 * max_dist / sel_occ with G > 0, NULL seg or half with M > 0, NULL points with n > 0.
 *
 * ---- btc_select_templates: step 6, the greedy rounds of find_multi_best_match_boxpnts for the batch
 *   iou (G, K) f32 the box IoU of (i, c), descending along k as the host's top-k left it ; own_occ (M, W) u32 every object's own bitmap
 *   aug = own_occ[i] ; set = i's rows ; alive = the candidates that are not -1 ; at most max_num_bm (<= 8) rounds:
 *     extra[k] = popcount(sel_occ[g][k] & ~aug)
 *     h[k]     = ((max_dist[g][k] + ratio / extra[k]) + (iou[g][k] < iou_thresh ? 2 : 0)) + (extra[k] < 30 ? 1 : 0)
 *                float32, left to right, ratio / 0 = +inf
 *     w        = the alive k of smallest h, the lowest k among equals (none: stop; a NaN never wins)
 *     stop if (iou[g][w] < iou_thresh and the set is not empty) or extra[w] == 0
 *     s        = the r-th candidate that is not -1, r = the number of alive candidates in front of w: the reference deletes a round's
 *                winner from its IoU, index, occupancy and distance arrays but not from its list of point sets, and indexes them all
 *                with one number, so after a deletion in front of w the rows are those of w's predecessor in that list; s = w in the
 *                first round and whenever the earlier winners stood behind w.  Kept, because the templates the shipped model was
 *                trained with were made this way
 *     added    = the rows of candidate s (all of them, in order) whose smallest d2 to the set is > nearest_sq
 *     if there are more than 4: the set grows by them, chosen[g][round] = cand[g][s], aug |= sel_occ[g][w]
 *     stop if one candidate was alive or popcount(aug), as of the last growth (0 before any), >= num_extra_coords;
 *     otherwise w is no longer alive -- also when it added nothing
 *   nearest_sq: the largest float32 whose correctly rounded square root is <= float32(nearest_dist), formed by the host, so that
 *   d2 > nearest_sq is sqrt(d2) > nearest_dist decision for decision.
 *   tmpl_offsets (G+1) i32 ; chosen (G, max_num_bm) i32 the object whose rows the round added, -1 = it added nothing or did not run ;
 *   out (capacity, 3) f32 ; src (capacity, 2) i32 = (source object, row in its set), or NULL
 * Template g is rows [tmpl_offsets[g], tmpl_offsets[g+1]) of out: i's own rows, then what each round added, in that order.
 * tmpl_offsets and chosen are always true, whatever capacity is; out and src are written only below capacity (the caller sees
 * tmpl_offsets[G] > capacity and calls again), and nothing at or past min(total, capacity).  max_rows is a host scalar, the largest
 * number of rows of any set (it sizes the workspace): a set's rows past max_rows are not looked at.  Three launches (pick, offsets,
 * write); ws contents are arbitrary on entry; no atomics on global memory: results are the same from run to run.
 * Refused: G, M, n, capacity, max_rows, num_extra_coords < 0, K < 1 or > 8192, W < 1 or > 2048, max_num_bm < 1 or > 8, a NULL
 * tmpl_offsets / chosen / ws, NULL obj / cand / iou / max_dist / sel_occ with G > 0, NULL seg or own_occ with M > 0, NULL points with
 * n > 0, NULL out with capacity > 0, G * (max_num_bm + 1) * max_rows >= 2^31, a workspace below
 * btc_select_templates_ws_bytes(G, max_num_bm, max_rows) (which is 0 for refused arguments). */
#ifndef BTCDET_HIP_TEMPLATES_H
#define BTCDET_HIP_TEMPLATES_H

#include <stddef.h>
#include <stdint.h>

#include "btcdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int btc_nn_sqdist(const float* q_points, int nq, const float* t_points, int nt, const int32_t* pairs, const int32_t* out_offsets, int P,
                  int out_rows, float* out, void* stream);
int btc_match_candidates(const float* points, int n, const int32_t* seg, const float* half, int M, const int32_t* obj, const int32_t* cand,
                         int G, int K, float x0, float y0, float cell, int nx, int ny, float* max_dist, uint32_t* sel_occ, void* stream);
size_t btc_select_templates_ws_bytes(int G, int max_num_bm, int max_rows);
int btc_select_templates(const float* points, int n, const int32_t* seg, int M, const int32_t* obj, const int32_t* cand, const float* iou,
                         const float* max_dist, const uint32_t* sel_occ, const uint32_t* own_occ, int G, int K, int W, int max_num_bm,
                         int num_extra_coords, float iou_thresh, float ratio, float nearest_sq, int max_rows, int capacity, float* out,
                         int32_t* src, int32_t* tmpl_offsets, int32_t* chosen, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
