// The camera field-of-view decision for one scan row, stated once (fov_crop.hip: btc_fov_crop, kitti_infos.hip: btc_count_in_boxes), so
// that the rows the crop keeps and the rows the point counts look at cannot differ by a bit.
#pragma once
#include "btc_common.h"

#include "../../include/btcdet_hip_frames.h"

// the header's arithmetic; c = one scene's calibration block
static __device__ __forceinline__ bool fov_keep(float x, float y, float z, const float* __restrict__ c) {
  float r[3], h[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
    r[j] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(x, c[j]), __fmul_rn(y, c[3 + j])), __fmul_rn(z, c[6 + j])), c[9 + j]);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float* p = c + 12 + 4 * i;
    h[i] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(r[0], p[0]), __fmul_rn(r[1], p[1])), __fmul_rn(r[2], p[2])), p[3]);
  }
  const float u = __fdiv_rn(h[0], r[2]), v = __fdiv_rn(h[1], r[2]);
  const float depth = __fsub_rn(h[2], c[12 + 11]);
  return (u >= 0.f) & (u < c[24]) & (v >= 0.f) & (v < c[25]) & (depth >= 0.f);   // NaN compares false, as in numpy
}
