/* btcdet_hip_infos.h -- the point work of creating the KITTI infos: points per ground-truth box and coverage-rate cell counts, entry
 * points of libbtcdet_hip.so (gfx950); the eighth public header beside btcdet_hip.h, btcdet_hip_infer.h, btcdet_hip_augment.h,
 * btcdet_hip_bestmatch.h, btcdet_hip_frames.h, btcdet_hip_gtdb.h and btcdet_hip_templates.h (csrc/kitti_infos.hip).
 *
 * Same common rules as btcdet_hip.h: every pointer is a DEVICE pointer unless its name starts with h_; the caller allocates every
 * buffer; `stream` is a hipStream_t (NULL = the default stream) and every call only enqueues work on it; an entry point returns
 * BTC_OK or a BTC_E* code, with the text in btc_last_error(), and never exits the process.  ws contents are arbitrary on entry;
 * results are the same from run to run (the only atomics are integer adds and compare-and-swaps whose outcome is a set).
 *
 * What is replaced: the point work of the reference's KittiDataset.get_infos (btcdet/datasets/kitti/kitti_dataset.py:181-194:
 * lidar_to_rect, get_fov_flag, in_hull per box, flag.sum()) and of create_info_file_with_coverage (kitti_dataset.py:208-225, 246-251:
 * get_coords over a template and an object).  Labels, images, calibrations, dictionaries and files stay on the host
 * (btcdet_amd/kitti_infos.py).
 *
 * ==== btc_count_in_boxes: per box, the rows of its scene that the camera sees and that lie inside it
 *   points (n, ld) f32 raw scans, scenes contiguous, ld >= 3 ; scene_offsets (batch+1) i32 ascending, [0] = 0, [batch] = n
 *   calib (batch, 32) f32: btc_fov_crop's blocks (btcdet_hip_frames.h)
 *   boxes (m, 8) f32 in btc_cut_objects' layout, WITHOUT the 0.01 margin (the reference's in_hull tests the bare hull):
 *     [0..2] cx, cy, cz   [3] hx = dx/2   [4] hy = dy/2   [5] hz = dz/2   [6] c = cos(-heading)   [7] s = sin(-heading)
 *     every value formed on the host in float32 from the float32 box
 *   box_offsets (batch+1) i32 ascending: scene s owns boxes [box_offsets[s], box_offsets[s+1])
 *   counts (m) i32 ; fov_rows (batch) i32 or NULL
 * Per row (x, y, z) = columns 0..2 of scene s:
 *   seen   = btc_fov_crop's keep decision against calib[s], bit for bit (one device function serves both; btcdet_hip_frames.h
 *            states its arithmetic)
 *   inside = btc_cut_objects' test against box row b, bit for bit (one device function; btcdet_hip_gtdb.h states it):
 *            sx = x - cx, sy = y - cy, lx = sx*c - sy*s, ly = sx*s + sy*c, (|z - cz| <= hz) & (|lx| < hx) & (|ly| < hy), every
 *            operation rounded to float32 on its own
 *   counts[j]   = the rows of box j's scene with seen & inside
 *   fov_rows[s] = the rows of scene s with seen (what btc_fov_crop keeps of it)
 * A row inside two boxes counts in both; a row counts only for boxes of its own scene; a NaN coordinate counts nowhere; a box no
 * scene owns gets 0.  Empty scenes, scenes without boxes, n == 0 and m == 0 are legal.
 * One pass: every row is read once (16 B for ld == 4 with a 16-byte aligned base; a scalar path otherwise, with equal results) and
 * nothing is written per row.  Tiles of 256 rows are aligned to scenes; a workgroup stages its scene's calibration block and its box
 * rows, 64 at a time (no bound on the boxes of a scene), in LDS, counts with one ballot and popcount per (wave, box), sums its four
 * waves in LDS and adds once per (workgroup, box with a hit) to counts.  Three launches: tiles, zero, count.
 * The bound: 16 B per row.  At 8 TB/s a 120 K-row scan is 0.25 us, far below one launch: at a few frames per batch the call is
 * launch-bound (tools/infos_bench.py records the time).
 * Refused before any launch (BTC_EINVAL, nothing written): ld < 3, batch < 1, n < 0, m < 0, a NULL scene_offsets / calib /
 * box_offsets / ws, NULL points with n > 0, NULL boxes or counts with m > 0, a workspace below btc_count_in_boxes_ws_bytes(n, batch)
 * (which is 0 for refused arguments).
 *
 * ==== btc_coverage_cells: per job, the two unique-cell counts of get_coords
 *   tmpl_rows (T, 3) f32 box-local template rows ; obj_rows (R, ld) f32 centre-shifted database rows, ld >= 3
 *   jobs (J, 4) i32: [tmpl_first, tmpl_n, obj_first, obj_n]
 *   pose (J, 5) f64: [cx, cy, cz, cos(yaw), sin(yaw)], cos and sin taken on the host in double (the device calls neither)
 *   max_rows: a host scalar, at least every job's tmpl_n and obj_n (it sizes the workspace)
 *   cells (J, 2) i32: [unique_obj, unique_bm] ; status (J) i32
 * Arithmetic, in double, every operation rounded on its own (no fused multiply-add); tx, ty, tz, ox, oy, oz widened from float32:
 *   template point:  x = (tx*c - ty*s) + cx,  y = (tx*s + ty*c) + cy,  z = tz + cz
 *   object point:    x = ox + cx,  y = oy + cy,  z = oz + cz
 *   r  = sqrt((x*x + y*y) + z*z)
 *   az = (atan2(-y, x) * 180.0) / pi
 *   el = (atan2(z, sqrt(x*x + y*y)) * 180.0) / pi
 *   mn_k   = min(min over the template rows of coordinate k, 0)                       k = r, az, el
 *   cell_k = floor((s_k - mn_k) / res_k),  res = (0.32, 0.5184, 0.4203125)
 *   n_k    = max over the template rows of cell_k + 11     (floor((max s_k - mn_k) / res_k) + 11: every step is monotone in s_k)
 *   unique_bm  = the number of distinct template cells (cell_r, cell_az, cell_el)
 *   unique_obj = the number of distinct object cells among the object rows with 0 <= cell_k < n_k for all three k
 * tmpl_n == 0 gives (0, 0); obj_n == 0 gives unique_obj = 0.  Rows are finite (a NaN row is not defined here).
 * status[j]: BTC_COVERAGE_OK and cells[j] written; BTC_COVERAGE_WIDE: some n_k > 1024, so a kept cell may not fit the 10 bits per
 * coordinate of the 32-bit key (azimuth needs at most 705 and elevation 439 for any geometry, range stays below 1024 cells up to
 * 324 m): cells[j] is NOT written and the caller computes the job on the host; BTC_COVERAGE_BAD: a job's rows lie outside [0, T) or
 * [0, R) or exceed max_rows: cells[j] is not written and no row is read.
 * One workgroup of 256 threads per job; three passes that each recompute the spherical coordinates (nothing is stored per row): the
 * template's minima and maxima; the template's keys into an exact set; the table cleared, then the object's kept keys into the set.
 * The set is open addressing with linear probing, capacity the power of two >= 2 * max(tmpl_n, obj_n, 32), insertion by
 * compare-and-swap, the count going up on a successful insert, so the result does not depend on the order of arrival.  A table of
 * up to BTC_COVERAGE_LDS_KEYS = 8192 keys (jobs of up to 4096 rows) lives in 32 KB of static LDS: five workgroups fit the 160 KB of
 * a CU and no dynamic-LDS attribute is needed; a larger job uses its slice of ws through the same code.
 * btc_coverage_cells_ws_bytes(J, max_rows): J slices of the power of two >= 2 * max_rows keys when that exceeds
 * BTC_COVERAGE_LDS_KEYS, 256 otherwise; 0 for refused arguments (J < 0, max_rows < 0, max_rows >= 2^29).
 * Refused before any launch (BTC_EINVAL, nothing written): J < 0, T < 0, R < 0, ld < 3, max_rows < 0 or >= 2^29, a NULL ws, NULL
 * jobs / pose / cells / status with J > 0, a workspace below btc_coverage_cells_ws_bytes(J, max_rows).  NULL tmpl_rows with T == 0
 * and NULL obj_rows with R == 0 are legal.  J == 0 launches nothing. */
#ifndef BTCDET_HIP_INFOS_H
#define BTCDET_HIP_INFOS_H

#include <stddef.h>
#include <stdint.h>

#include "btcdet_hip.h"

#define BTC_COVERAGE_OK 0
#define BTC_COVERAGE_WIDE 1
#define BTC_COVERAGE_BAD 2
#define BTC_COVERAGE_LDS_KEYS 8192

#ifdef __cplusplus
extern "C" {
#endif

size_t btc_count_in_boxes_ws_bytes(int n, int batch);
int btc_count_in_boxes(const float* points, int n, int ld, const int32_t* scene_offsets, int batch, const float* calib,
                       const float* boxes, const int32_t* box_offsets, int m, int32_t* counts, int32_t* fov_rows,
                       void* ws, size_t ws_bytes, void* stream);

size_t btc_coverage_cells_ws_bytes(int J, int max_rows);
int btc_coverage_cells(const float* tmpl_rows, int T, const float* obj_rows, int R, int ld, const int32_t* jobs, const double* pose,
                       int J, int max_rows, int32_t* cells, int32_t* status, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
