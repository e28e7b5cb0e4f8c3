/* btcdet_hip_augment.h -- training augmentation of a resident batch, entry points of libbtcdet_hip.so (gfx950); the third public
 * header beside btcdet_hip.h and btcdet_hip_infer.h (csrc/augment.hip).
 *
 * Same common rules as btcdet_hip.h: every pointer is a DEVICE pointer unless its name starts with h_; the caller allocates every
 * buffer; `stream` is a hipStream_t (NULL = the default stream) and every call only enqueues work on it; an entry point returns
 * BTC_OK or a BTC_E* code, with the text in btc_last_error(), and never exits the process.
 *
 * What is replaced: the point half of the reference's DataAugmentor.forward (btcdet/datasets/augmentor/data_augmentor.py:171-202) for
 * a whole batch of raw scans that already lives in HBM -- DataBaseSampler's paste (database_sampler.py:146-189: scene points inside the
 * pasted boxes are removed, the database objects appended), random_world_flip along x, random_world_scaling and
 * random_world_rotation with SAVE_PRE_ROT (augmentor_utils.py:5-20,44-82).  Everything that is O(boxes) -- the random draws, the
 * choice of database objects, the box arithmetic -- stays on the host (btcdet_amd/device_augmentor.py: DeviceAugmentor.plan) and
 * arrives here as a plan.  The results equal the host chain's bit for bit.
 *
 * ---- the plan, per scene b of `batch`
 *   removal boxes  rm_boxes rows [rm_offsets[b], rm_offsets[b+1]), 8 floats each:
 *                    cx, cy, cz, hx = dx/2 + margin, hy = dy/2 + margin, hz = dz/2, c = cos(-heading), s = sin(-heading)
 *                  all formed by the host in float32 with the expressions of database_sampler.points_in_boxes_mask.  A scan row
 *                  (x, y, z) is REMOVED iff for some box, every product and sum rounded to float32 on its own (nothing fused):
 *                    sx = x - cx, sy = y - cy, lx = sx*c - sy*s, ly = sx*s + sy*c
 *                    |z - cz| <= hz (inclusive)  and  |lx| < hx  and  |ly| < hy (strict)          -- a NaN compares false: kept
 *   pasted objects objects [obj_offsets[b], obj_offsets[b+1]) of the n_objects of the batch; object j is the rows
 *                  [obj_first[j], obj_first[j] + obj_rows[j]) of `bank` (bank_rows, ld), and obj_shift[4 j .. 4 j + 3] = centre x, y, z
 *                  and the road-plane lift (0 without one), as doubles.  A pasted row is
 *                    x = f32(f64(x) + cx), y = f32(f64(y) + cy), z = f32(f64(f32(f64(z) + cz)) - lift)
 *                  Why double: the host's `obj[:, :3] += box3d_lidar[:3]` on a float32 array is, with a float64 centre (a pickled
 *                  KITTI database), a float64 add rounded once to float32, and with a float32 centre a float32 add (measured with
 *                  numpy 2.2: 100000 random pairs, both forms, and `obj[:, 2] -= lift[i]` with a float64 / float32 numpy scalar
 *                  likewise).  One form serves both: the float64 sum of two float32 values rounded to float32 IS their
 *                  float32 sum (53 >= 2 * 24 + 2 bits: the second rounding cannot change the first).  A row of an object that
 *                  leaves [0, bank_rows) is written as zeros instead of being read.
 *   op program     ops rows [op_offsets[b], op_offsets[b+1]), at most BTC_AUG_MAX_OPS (rows past the 8th are ignored), 4 floats each
 *                  [kind, a, b, flag], applied in order to x, y, z of every emitted row; further columns are copied:
 *                    BTC_AUG_FLIP_X  y = -y
 *                    BTC_AUG_SCALE   x, y, z *= a                       (a = float32(noise_scale): numpy's f32 array *= Python float)
 *                    BTC_AUG_ROT     (x, y, z) . [[a, b, 0], [-b, a, 0], [0, 0, 1]],  a = cos, b = sin of the angle as float32, made
 *                                    on the host as data_side.rotate_points_along_z makes them (no device cosf).  Two roundings of the
 *                                    product, as that function has them:  column j = fma(z, r2j, fma(y, r1j, x * r0j)) for a set of
 *                                    >= 45 rows, ((0 + x r0j) + y r1j) + z r2j with every step rounded for a smaller set.
 *                                    btc_augment_batch chooses by the scene's emitted row count (known on the device only: removal
 *                                    is data dependent) and ignores `flag`; btc_world_transform takes flag != 0 as "small set".
 *
 * ---- btc_augment_batch
 *   points (n_rows, ld) f32 raw scans, scenes contiguous ; scene_offsets (batch+1) i32 ascending, [0] = 0, [batch] = n_rows
 *   n_objects, paste_rows : host copies of obj_offsets[batch] and of the sum of obj_rows -- they size the launch and the refusals
 *                  below; the kernels never write a row >= out_capacity nor read the bank outside [0, bank_rows) whatever they say
 *   out (out_capacity, ld) ; out_pre (out_capacity, ld) or NULL ; out_offsets (batch+1) i32
 * Output order per scene = np.concatenate([scene[keep]] + clouds): the kept scan rows in input order, then every pasted object in plan
 * order, its rows in file order.  out_offsets[batch] = n' is the total; rows >= n' are not written.  out_pre receives every row as
 * it stands when its scene's first BTC_AUG_ROT op is reached (`pre_rot_points`: scaled only if the scaling came first); without such
 * an op it equals out.  ld == 4 with 16-byte aligned arrays moves a row as one 16-byte load and store.
 * Refused before any launch (BTC_EINVAL, nothing written): ld < 3, batch < 1, a negative count, out_capacity < n_rows + paste_rows,
 * n_rows + paste_rows >= 2^31, a NULL scene_offsets / rm_offsets / op_offsets / out_offsets / ws, NULL points with n_rows > 0, NULL
 * bank / obj_* with n_objects > 0, NULL out with out_capacity > 0, a workspace below btc_augment_ws_bytes(n_rows, batch, n_objects).
 * rm_boxes and ops may be NULL: no removal / no op.  ws contents are arbitrary on entry.
 *
 * ---- btc_world_transform: the op program alone over `batch` stacked sets (the special point sets of a batch: flip, scale and
 * rotation, no removal, no paste); in / out (n_rows, ld), set_offsets (batch+1) i32; out may not alias in.  One launch. */
#ifndef BTCDET_HIP_AUGMENT_H
#define BTCDET_HIP_AUGMENT_H

#include <stddef.h>
#include <stdint.h>

#include "btcdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BTC_AUG_FLIP_X 1
#define BTC_AUG_SCALE 2
#define BTC_AUG_ROT 3
#define BTC_AUG_MAX_OPS 8

size_t btc_augment_ws_bytes(int n_rows, int batch, int n_objects);
int btc_augment_batch(const float* points, int n_rows, int ld, const int32_t* scene_offsets, int batch,
                      const float* rm_boxes, const int32_t* rm_offsets,
                      const float* bank, long long bank_rows,
                      const int32_t* obj_first, const int32_t* obj_rows, const double* obj_shift, const int32_t* obj_offsets,
                      int n_objects, long long paste_rows,
                      const float* ops, const int32_t* op_offsets,
                      long long out_capacity, float* out, float* out_pre, int32_t* out_offsets, void* ws, size_t ws_bytes, void* stream);
int btc_world_transform(const float* in, int n_rows, int ld, const int32_t* set_offsets, int batch, const float* ops,
                        const int32_t* op_offsets, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
