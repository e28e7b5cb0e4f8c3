// The per-row pieces the augmentation kernels share (augment.hip, best_match.hip, gt_database.hip): the in-box test, the z rotation with
// its two roundings and the op program of include/btcdet_hip_augment.h; the owner search over an ascending offsets array comes with
// compact.h.
#pragma once
#include "compact.h"

#include "../../include/btcdet_hip_augment.h"

// database_sampler.points_in_boxes_mask against one (8) box row of device_augmentor.removal_rows: unfused float32 arithmetic (numpy
// does not fuse, and a fused form moves a point that sits within an ulp of a face across it).  The removal of btc_augment_batch and
// the cut of btc_cut_objects (include/btcdet_hip_gtdb.h) are this one function.
static __device__ __forceinline__ bool aug_in_box(float x, float y, float z, const float* __restrict__ b) {
  const float sx = __fsub_rn(x, b[0]), sy = __fsub_rn(y, b[1]);
  const float c = b[6], s = b[7];
  const float lx = __fsub_rn(__fmul_rn(sx, c), __fmul_rn(sy, s));
  const float ly = __fadd_rn(__fmul_rn(sx, s), __fmul_rn(sy, c));
  return (fabsf(__fsub_rn(z, b[2])) <= b[5]) && (fabsf(lx) < b[3]) && (fabsf(ly) < b[4]);
}

// data_side.rotate_points_along_z: p . [[c, s, 0], [-s, c, 0], [0, 0, 1]] with its two roundings
static __device__ __forceinline__ void aug_rotate(float& x, float& y, float& z, float c, float s, bool small_set) {
  const float r0[3] = {c, s, 0.f}, r1[3] = {-s, c, 0.f}, r2[3] = {0.f, 0.f, 1.f};
  float o[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (small_set) o[j] = __fadd_rn(__fadd_rn(__fadd_rn(0.f, __fmul_rn(x, r0[j])), __fmul_rn(y, r1[j])), __fmul_rn(z, r2[j]));
    else o[j] = __fmaf_rn(z, r2[j], __fmaf_rn(y, r1[j], __fmul_rn(x, r0[j])));
  }
  x = o[0], y = o[1], z = o[2];
}

// runs set `s`'s op program on (x, y, z); (px, py, pz) = the point as it stood at the first ROT (the final point without one).
// USE_FLAG: the rotation form comes from the op's flag (sets of host-known size) instead of `small_set`
template <bool USE_FLAG>
static __device__ __forceinline__ void aug_run_ops(const float* __restrict__ ops, const int32_t* __restrict__ op_offsets, int s, bool small_set,
                                                   float& x, float& y, float& z, float& px, float& py, float& pz) {
  bool snapped = false;
  if (ops != nullptr) {
    const int o0 = op_offsets[s];
    const int cnt = min(max(op_offsets[s + 1] - o0, 0), BTC_AUG_MAX_OPS);
    for (int k = 0; k < cnt; ++k) {
      const float* op = ops + (size_t)(o0 + k) * 4;
      const int kind = (int)op[0];
      if (kind == BTC_AUG_FLIP_X) {
        y = -y;
      } else if (kind == BTC_AUG_SCALE) {
        const float a = op[1];
        x = __fmul_rn(x, a), y = __fmul_rn(y, a), z = __fmul_rn(z, a);
      } else if (kind == BTC_AUG_ROT) {
        if (!snapped) px = x, py = y, pz = z, snapped = true;
        aug_rotate(x, y, z, op[1], op[2], USE_FLAG ? (op[3] != 0.f) : small_set);
      }
    }
  }
  if (!snapped) px = x, py = y, pz = z;
}
