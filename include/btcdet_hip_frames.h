/* btcdet_hip_frames.h -- the camera field-of-view crop of a resident batch of raw scans, entry points of libbtcdet_hip.so (gfx950);
 * the fifth public header beside btcdet_hip.h, btcdet_hip_infer.h, btcdet_hip_augment.h and btcdet_hip_bestmatch.h (csrc/fov_crop.hip).
 *
 * Same common rules as btcdet_hip.h: every pointer is a DEVICE pointer unless its name starts with h_; the caller allocates every
 * buffer; `stream` is a hipStream_t (NULL = the default stream) and every call only enqueues work on it; an entry point returns
 * BTC_OK or a BTC_E* code, with the text in btc_last_error(), and never exits the process.
 *
 * What is replaced: FOV_POINTS_ONLY of the reference's KittiDataset.__getitem__ (btcdet/datasets/kitti/kitti_dataset.py:426-429:
 * calib.lidar_to_rect, get_fov_flag, points[fov_flag]) for a whole batch of raw scans that already lives in HBM.  Reading the files and
 * the calibrations stays on the host (btcdet_amd/kitti_frames.py: KittiFrames.load_batch).
 *
 * ---- the calibration block: calib (batch, 32) f32, per scene
 *   [ 0..11]  M[4][3] row-major = np.dot(V2C.T, R0.T), formed on the host in float32 as Calibration.lidar_to_rect forms it
 *   [12..23]  P2[3][4] row-major
 *   [24], [25] W, H: the image's width and height as floats (exact: the host refuses a value of 2^24 or more)
 *   [26..31]  padding, never read
 *
 * ---- the arithmetic, per row (x, y, z) = columns 0..2; every product and every sum is rounded to float32 on its own (nothing fused)
 *   r_j   = ((x*M[0][j] + y*M[1][j]) + z*M[2][j]) + M[3][j]                 j = 0, 1, 2     (the rectified camera frame)
 *   h_i   = ((r_0*P2[i][0] + r_1*P2[i][1]) + r_2*P2[i][2]) + P2[i][3]       i = 0, 1, 2
 *   u     = h_0 / r_2,  v = h_1 / r_2,  depth = h_2 - P2[2][3]              (IEEE division, round to nearest)
 *   keep  = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (depth >= 0)
 * A NaN compares false, as in numpy: a row with a NaN coordinate is dropped.  r_2 == 0 gives +-inf or NaN for u and v: dropped without
 * a special case.  A point behind the camera can project inside the image; depth < 0 drops it.  The reference's np.dot goes through
 * BLAS, whose summation order is not defined, so these formulas -- not the reference's bits of u, v, depth -- are the contract; they
 * give the reference's decisions for every point that is not within rounding of an image edge (the decision margin).
 *
 * ---- btc_fov_crop: a stable compaction
 *   points (n, ld) f32 raw scans, scenes contiguous, ld >= 3 ; scene_offsets (batch+1) i32 ascending, [0] = 0, [batch] = n
 *   out (out_capacity, ld) f32, out_capacity >= n ; out_offsets (batch+1) i32 ; keep_idx (out_capacity) i32 or NULL
 * The kept rows of each scene appear in input order with all ld columns copied bit for bit; out_offsets[s] = kept rows in front of
 * scene s, out_offsets[batch] = n' the total; keep_idx[dst] = src.  Rows >= n' of out and keep_idx are not written, and no row
 * >= out_capacity whatever the device arrays say.  ld == 4 with 16-byte aligned points and out moves a row as one 16-byte load and
 * store; any other ld, or an unaligned base, takes a scalar path with the same results.  Empty scenes and n == 0 are legal.
 * Four launches (mark and count, scan, scatter, offsets); each row's decision is made once, in the first, and read by the others.
 * No atomics, no memset: ws contents are arbitrary on entry.
 * Refused before any launch (BTC_EINVAL, nothing written): ld < 3, batch < 1, n < 0, out_capacity < n, a NULL scene_offsets / calib /
 * out_offsets / ws, NULL points or out with n > 0, a workspace below btc_fov_crop_ws_bytes(n, batch) (which is 0 for refused n, batch). */
#ifndef BTCDET_HIP_FRAMES_H
#define BTCDET_HIP_FRAMES_H

#include <stddef.h>
#include <stdint.h>

#include "btcdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BTC_FOV_CALIB_FLOATS 32

size_t btc_fov_crop_ws_bytes(int n, int batch);
int btc_fov_crop(const float* points, int n, int ld, const int32_t* scene_offsets, int batch, const float* calib,
                 int out_capacity, float* out, int32_t* out_offsets, int32_t* keep_idx,
                 void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
