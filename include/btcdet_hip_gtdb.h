/* btcdet_hip_gtdb.h -- the objects of a ground-truth database cut from a resident batch of raw scans, entry points of
 * libbtcdet_hip.so (gfx950); the sixth public header beside btcdet_hip.h, btcdet_hip_infer.h, btcdet_hip_augment.h,
 * btcdet_hip_bestmatch.h and btcdet_hip_frames.h (csrc/gt_database.hip).
 *
 * Same common rules as btcdet_hip.h: every pointer is a DEVICE pointer unless its name starts with h_; the caller allocates every
 * buffer; `stream` is a hipStream_t (NULL = the default stream) and every call only enqueues work on it; an entry point returns
 * BTC_OK or a BTC_E* code, with the text in btc_last_error(), and never exits the process.
 *
 * What is replaced: the point work of the reference's KittiDataset.create_groundtruth_database (btcdet/datasets/kitti/
 * kitti_dataset.py:291-300: points_in_boxes_cpu, points[point_indices[i] > 0], gt_points[:, :3] -= gt_boxes[i, :3]) for a whole batch
 * of raw scans that already lives in HBM.  Names, paths, db_infos and the files stay on the host (btcdet_amd/gt_database.py).
 *
 * ---- the box rows: boxes (m, 8) f32, the row form of btc_augment_batch's rm_boxes (device_augmentor.removal_rows)
 *   [0..2] cx, cy, cz   [3] hx = dx/2 + 0.01   [4] hy = dy/2 + 0.01   [5] hz = dz/2   [6] c = cos(-heading)   [7] s = sin(-heading)
 * every value formed on the host in float32, by the expressions of database_sampler.points_in_boxes_mask.
 *
 * ---- the test, per row (x, y, z) = columns 0..2 and box row b; every product, sum and difference is rounded to float32 on its own
 *   sx = x - cx,  sy = y - cy
 *   lx = sx*c - sy*s,  ly = sx*s + sy*c
 *   inside = (|z - cz| <= hz) & (|lx| < hx) & (|ly| < hy)
 * A NaN compares false: a row with a NaN coordinate is in no object.  This is the test by which btc_augment_batch removes scan rows
 * under a pasted box (one device function serves both), and database_sampler.points_in_boxes_mask bit for bit.  The reference's
 * compiled op forms hx, hy in double and takes cos / sin from libm: its decisions are these for every point that is not within
 * rounding of a face.
 *
 * ---- btc_cut_objects
 *   points (n, ld) f32 raw scans, scenes contiguous, ld >= 3 ; scene_offsets (batch+1) i32 ascending, [0] = 0, [batch] = n
 *   boxes (m, 8) f32 ; centre (m, 3) f64 ; box_offsets (batch+1) i32 ascending: scene s owns boxes [box_offsets[s], box_offsets[s+1])
 *   max_boxes: a host scalar, the largest number of boxes any scene owns (it sizes the workspace); the boxes of a scene past its
 *              first max_boxes, and boxes no scene owns, get zero rows
 *   out (out_capacity, ld) f32 ; obj_offsets (m+1) i32 ; src_idx (out_capacity) i32 or NULL
 * out is box-major: object j owns rows [obj_offsets[j], obj_offsets[j+1]), the rows of ITS scene that pass the test against box j, in
 * scan order; a row inside two boxes appears in both objects.  Columns 0..2 are (float)((double)p - centre[j]) -- one rounding, which
 * is numpy's `gt_points[:, :3] -= gt_boxes[i, :3]` for a float64 and for a float32 centre alike -- and columns 3.. are copied bit for
 * bit.  src_idx[dst] = the source row.  obj_offsets always holds the true offsets and obj_offsets[m] the true total, whatever
 * out_capacity is: rows whose destination is >= out_capacity are not written (the caller sees total > out_capacity and calls again),
 * nothing at or past min(total, out_capacity) is written, and nothing past obj_offsets[m].  Every store is guarded by n, m,
 * max_boxes and out_capacity whatever the device arrays say.  ld == 4 with 16-byte aligned points and out moves a row as one 16-byte
 * load and store; any other ld, or an unaligned base, takes a scalar path with the same results.  Empty scenes, scenes without
 * boxes, n == 0 and m == 0 are legal; with m == 0, obj_offsets[0] = 0.
 * Five launches (tiles, count, per-box scan, offsets, scatter); tiles of 256 rows are aligned to scenes, so their number is at most
 * ceil(n / 256) + batch.  No atomics, no memset: ws contents are arbitrary on entry; results are the same from run to run.
 * Refused before any launch (BTC_EINVAL, nothing written): ld < 3, batch < 1, n < 0, m < 0, max_boxes < 0, out_capacity < 0, a NULL
 * scene_offsets / box_offsets / obj_offsets / ws, NULL points with n > 0, NULL boxes or centre with m > 0, NULL out with
 * out_capacity > 0, a workspace below btc_cut_objects_ws_bytes(n, batch, m, max_boxes) (which is 0 for refused arguments). */
#ifndef BTCDET_HIP_GTDB_H
#define BTCDET_HIP_GTDB_H

#include <stddef.h>
#include <stdint.h>

#include "btcdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t btc_cut_objects_ws_bytes(int n, int batch, int m, int max_boxes);
int btc_cut_objects(const float* points, int n, int ld, const int32_t* scene_offsets, int batch,
                    const float* boxes, const double* centre, const int32_t* box_offsets, int m, int max_boxes,
                    int out_capacity, float* out, int32_t* obj_offsets, int32_t* src_idx,
                    void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
