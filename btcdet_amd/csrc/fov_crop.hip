// The camera field-of-view crop of a resident batch of raw scans for gfx950 (include/btcdet_hip_frames.h: btc_fov_crop).
//
//   fov_mark     one thread per scan row, 256 per workgroup.  The workgroup finds the scenes its rows span (two searches of
//                scene_offsets, the same in every thread) and stages their 128-byte calibration blocks in LDS eight at a time (no cap on
//                the batch); each row is projected with unfused float32 arithmetic (__fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn: the
//                header's formulas are the contract, and a fused form moves a point that sits within an ulp of an image edge across it).
//                -> keep flag per row, kept count per workgroup.
//   (scan)       btc_scan_exclusive_i32 over the workgroup counts (csrc/scan.hip).
//   fov_scatter  the kept rows at their stable rank (compact.h).  It reads the flag fov_mark wrote, so the count and the scatter
//                cannot disagree.
//   fov_offsets  one wave per scene boundary: kept rows in front of it, from the same flags.
//
// A stream: 16 B read by fov_mark, 1 + 16 B read and at most 16 + 4 B written by fov_scatter per row of a (n, 4) scan.  No atomics, no
// memset, no ticket: every workspace word a kernel reads was written by an earlier launch of the same call.
#include "compact.h"   // the compaction's count, rank, boundary, row copy and workspace; aug_owner
#include "fov_keep.h"  // the per-row decision (the header's arithmetic), shared with kitti_infos.hip

#include "../../include/btcdet_hip_frames.h"

namespace {

constexpr int FOV_T = BTC_COMPACT_T;
constexpr int FOV_CAL = BTC_FOV_CALIB_FLOATS;
constexpr int FOV_CHUNK = FOV_T / FOV_CAL;   // calibration blocks staged per pass: one float per thread

template <bool VEC4>
__global__ __launch_bounds__(FOV_T) void fov_mark(const float* __restrict__ pts, int n, int ld, const int32_t* __restrict__ scene_offsets, int batch,
                                                  const float* __restrict__ calib, unsigned char* __restrict__ keep_flag,
                                                  int32_t* __restrict__ block_cnt) {
  __shared__ float s_cal[FOV_CHUNK * FOV_CAL];
  const int row0 = blockIdx.x * FOV_T;
  const int i = row0 + threadIdx.x;
  const bool live = i < n;
  float x = 0.f, y = 0.f, z = 0.f;
  int mine = -1;
  if (live) {
    const float* p = pts + (size_t)i * ld;
    if (VEC4) {
      const float4 v4 = *reinterpret_cast<const float4*>(p);
      x = v4.x, y = v4.y, z = v4.z;
    } else {
      x = p[0], y = p[1], z = p[2];
    }
    mine = aug_owner(scene_offsets, batch, i);
  }
  bool keep = false;
  if (row0 < n) {
    int s_lo, s_hi;
    btc_compact_scene_span(scene_offsets, batch, row0, n, s_lo, s_hi);
    for (int c0 = s_lo; c0 <= s_hi; c0 += FOV_CHUNK) {
      const int s = c0 + (int)threadIdx.x / FOV_CAL;
      __syncthreads();   // the previous chunk has been read
      if (s <= s_hi) s_cal[threadIdx.x] = calib[(size_t)s * FOV_CAL + threadIdx.x % FOV_CAL];
      __syncthreads();
      if (mine >= c0 && mine < c0 + FOV_CHUNK) keep = fov_keep(x, y, z, s_cal + (mine - c0) * FOV_CAL);
    }
  }
  if (live) keep_flag[i] = (unsigned char)keep;
  btc_compact_count(keep, block_cnt);
}

template <bool VEC4>
__global__ __launch_bounds__(FOV_T) void fov_scatter(const float* __restrict__ pts, int n, int ld, const unsigned char* __restrict__ keep_flag,
                                                     const int32_t* __restrict__ block_prefix, int out_capacity, float* __restrict__ out,
                                                     int32_t* __restrict__ keep_idx) {
  const int i = blockIdx.x * FOV_T + threadIdx.x;
  const bool keep = (i < n) && keep_flag[i] != 0;
  const int dst = btc_compact_rank(keep, block_prefix);
  if (!keep || dst < 0 || dst >= out_capacity) return;
  btc_copy_row<VEC4>(pts + (size_t)i * ld, out + (size_t)dst * ld, ld);
  if (keep_idx) keep_idx[dst] = i;
}

// out_offsets[s] = kept rows in front of scene s's first row; one wave per boundary
__global__ __launch_bounds__(64) void fov_offsets(const unsigned char* __restrict__ keep_flag, int n, const int32_t* __restrict__ scene_offsets,
                                                  int batch, const int32_t* __restrict__ block_prefix, const int32_t* __restrict__ total,
                                                  int32_t* __restrict__ out_offsets) {
  const int kept = btc_compact_boundary(blockIdx.x, scene_offsets, batch, n, block_prefix, total, [=](int j) -> int { return keep_flag[j]; });
  if (threadIdx.x == 0) out_offsets[blockIdx.x] = kept;
}

}  // namespace

extern "C" size_t btc_fov_crop_ws_bytes(int n, int batch) {
  if (n < 0 || batch < 1) return 0;
  return BtcCompactWs::bytes(n, true);
}

extern "C" int btc_fov_crop(const float* points, int n, int ld, const int32_t* scene_offsets, int batch, const float* calib, int out_capacity,
                            float* out, int32_t* out_offsets, int32_t* keep_idx, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(ld >= 3, "btc_fov_crop: need ld >= 3 (x, y, z columns), got %d", ld);
  BTC_CHECK_ARG(batch >= 1, "btc_fov_crop: need batch >= 1, got %d", batch);
  BTC_CHECK_ARG(n >= 0, "btc_fov_crop: negative count (n %d)", n);
  BTC_CHECK_ARG(out_capacity >= n, "btc_fov_crop: out_capacity %d below n = %d", out_capacity, n);
  BTC_CHECK_ARG(scene_offsets && calib && out_offsets && ws, "btc_fov_crop: missing pointer (scene_offsets, calib, out_offsets or ws)");
  BTC_CHECK_ARG((points && out) || n == 0, "btc_fov_crop: missing pointer (points or out)");
  BTC_CHECK_ARG(ws_bytes >= btc_fov_crop_ws_bytes(n, batch), "btc_fov_crop: workspace too small");
  const BtcCompactWs w(ws, n, true);
  const bool vec = ld == 4 && btc_aligned16(points) && btc_aligned16(out);
  if (vec) fov_mark<true><<<w.nb, FOV_T, 0, stream>>>(points, n, ld, scene_offsets, batch, calib, w.keep_flag, w.block_cnt);
  else fov_mark<false><<<w.nb, FOV_T, 0, stream>>>(points, n, ld, scene_offsets, batch, calib, w.keep_flag, w.block_cnt);
  BTC_LAUNCH_CHECK();
  int rc = w.scan(stream);
  if (rc != BTC_OK) return rc;
  if (n > 0) {
    if (vec) fov_scatter<true><<<w.nb, FOV_T, 0, stream>>>(points, n, ld, w.keep_flag, w.block_prefix, out_capacity, out, keep_idx);
    else fov_scatter<false><<<w.nb, FOV_T, 0, stream>>>(points, n, ld, w.keep_flag, w.block_prefix, out_capacity, out, keep_idx);
    BTC_LAUNCH_CHECK();
  }
  fov_offsets<<<batch + 1, 64, 0, stream>>>(w.keep_flag, n, scene_offsets, batch, w.block_prefix, w.total, out_offsets);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}
