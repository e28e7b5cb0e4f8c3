// The point work of creating the KITTI infos for gfx950 (include/btcdet_hip_infos.h: btc_count_in_boxes, btc_coverage_cells).
//
// btc_count_in_boxes -- num_points_in_gt of a resident batch of raw scans, one pass:
//   gtdb_tiles    (scene_tiles.h) one wave ranks the scenes' tile counts -> tile_first (batch + 1); tiles of 256 rows aligned to scenes.
//   infos_zero    counts (m) and fov_rows (batch) to 0.
//   infos_count   one workgroup per tile.  It stages its scene's calibration block and, 64 at a time, its scene's box rows in LDS;
//                 a row is read once, decided by fov_keep (fov_keep.h: btc_fov_crop's decision) and, when seen, tested against every
//                 staged box with aug_in_box (aug_ops.h: btc_cut_objects' decision) -- one ballot and popcount per (wave, box), lane k
//                 of a wave holding the wave's rows inside box k.  The four waves' counts meet in LDS and thread k adds the
//                 workgroup's count to counts[box k] once, when it is not 0.  Integer adds: the sum does not depend on their order.
//   A stream of 16 B per row; nothing is written per row.  Launch-bound at a few frames (three launches).
//
// btc_coverage_cells -- one workgroup per (template, object) job, three passes that recompute the spherical coordinates in double:
//   minima and maxima of the template -> mn, n ; the template's cells into an exact set ; the set cleared ; the object's kept cells
//   into the set.  The set: open addressing, linear probing, insertion by compare-and-swap, load <= 1/2; it lives in 32 KB of static
//   LDS for jobs of up to 4096 rows and in the job's slice of the workspace otherwise, through the same code.  A probe loop runs at
//   most `capacity` steps whatever the table holds.
// Every index formed from a device array is checked against n, m, T, R or max_rows before it addresses anything.
#include <limits.h>

#include "aug_ops.h"       // aug_in_box; compact.h: aug_owner, btc_aligned16
#include "fov_keep.h"      // fov_keep
#include "scene_tiles.h"   // GT_T, gtdb_tiles, GtTile, gtdb_tile, gtdb_load, gtdb_tmax

#include "../../include/btcdet_hip_infos.h"

namespace {

constexpr int IN_WAVES = GT_T / 64;
constexpr int IN_BOX_CHUNK = 64;   // boxes staged per pass: one per lane of a wave
constexpr int IN_CAL = BTC_FOV_CALIB_FLOATS;

__global__ __launch_bounds__(GT_T) void infos_zero(int32_t* __restrict__ counts, int m, int32_t* __restrict__ fov_rows, int batch) {
  const int i = blockIdx.x * GT_T + threadIdx.x;
  if (i < m) counts[i] = 0;
  if (fov_rows != nullptr && i < batch) fov_rows[i] = 0;
}

template <bool VEC4>
__global__ __launch_bounds__(GT_T) void infos_count(const float* __restrict__ pts, int n, int ld, const int32_t* __restrict__ scene_offsets, int batch,
                                                    const float* __restrict__ calib, const float* __restrict__ boxes,
                                                    const int32_t* __restrict__ box_offsets, int m, const int32_t* __restrict__ tile_first,
                                                    int32_t* __restrict__ counts, int32_t* __restrict__ fov_rows) {
  __shared__ float s_cal[IN_CAL];
  __shared__ float s_box[IN_BOX_CHUNK * 8];
  __shared__ int s_wcnt[IN_WAVES][64];
  GtTile t;
  if (!gtdb_tile(tile_first, scene_offsets, batch, n, box_offsets, m, INT_MAX, t)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if ((int)threadIdx.x < IN_CAL) s_cal[threadIdx.x] = calib[(size_t)t.s * IN_CAL + threadIdx.x];
  const long long i = t.row0 + threadIdx.x;
  const bool live = i < t.hi;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) p = gtdb_load<VEC4>(pts + (size_t)i * ld);
  __syncthreads();
  const bool seen = live && fov_keep(p.x, p.y, p.z, s_cal);
  if (fov_rows != nullptr) {   // the same in every thread
    const int c = __syncthreads_count(seen);
    if (threadIdx.x == 0 && c > 0) atomicAdd(fov_rows + t.s, c);
  }
  for (int c0 = 0; c0 < t.nbox; c0 += IN_BOX_CHUNK) {
    const int nb = min(IN_BOX_CHUNK, t.nbox - c0);
    const float* chunk = boxes + (size_t)(t.b0 + c0) * 8;
    __syncthreads();   // the previous chunk's LDS has been read
    for (int k = threadIdx.x; k < nb * 8; k += GT_T) s_box[k] = chunk[k];
    __syncthreads();
    int mine = 0;
    for (int k = 0; k < nb; ++k) {
      const bool hit = seen && aug_in_box(p.x, p.y, p.z, s_box + k * 8);
      const unsigned long long mk = __ballot(hit);
      if (lane == k) mine = __popcll(mk);
    }
    s_wcnt[wave][lane] = mine;
    __syncthreads();
    if ((int)threadIdx.x < nb) {
      int c = 0;
      for (int w = 0; w < IN_WAVES; ++w) c += s_wcnt[w][threadIdx.x];
      if (c > 0) atomicAdd(counts + t.b0 + c0 + threadIdx.x, c);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- coverage cells
constexpr int CV_T = 256;
constexpr int CV_WAVES = CV_T / 64;
constexpr unsigned CV_EMPTY = 0xFFFFFFFFu;   // no key: a key has 30 bits
constexpr int CV_MIN_ROWS = 32;
constexpr double CV_PI = 3.141592653589793;
constexpr double CV_LIMIT = 1024.0;          // cells per coordinate that fit a key

// the header's spherical coordinates of one point, every operation on its own (-ffp-contract=off: nothing is fused)
__device__ __forceinline__ void cv_sphere(double x, double y, double z, double s[3]) {
  const double xx = x * x, yy = y * y, zz = z * z;
  const double xy = xx + yy;
  s[0] = sqrt(xy + zz);
  s[1] = (atan2(-y, x) * 180.0) / CV_PI;
  s[2] = (atan2(z, sqrt(xy)) * 180.0) / CV_PI;
}

__device__ __forceinline__ void cv_template_point(const float* __restrict__ t, const double* __restrict__ pose, double s[3]) {
  const double tx = (double)t[0], ty = (double)t[1], tz = (double)t[2];
  const double c = pose[3], sn = pose[4];
  const double a = tx * c, b = ty * sn, d = tx * sn, e = ty * c;
  cv_sphere((a - b) + pose[0], (d + e) + pose[1], tz + pose[2], s);
}

__device__ __forceinline__ void cv_object_point(const float* __restrict__ o, const double* __restrict__ pose, double s[3]) {
  cv_sphere((double)o[0] + pose[0], (double)o[1] + pose[1], (double)o[2] + pose[2], s);
}

__device__ __forceinline__ double cv_cell(double s, double mn, int k) {
  const double res = k == 0 ? 0.32 : (k == 1 ? 0.5184 : 0.4203125);
  const double d = s - mn;
  return floor(d / res);
}

// -> 1 when `key` was not in the set; at most mask + 1 probes
__device__ __forceinline__ int cv_insert(unsigned* tab, unsigned mask, unsigned key) {
  unsigned slot = btc_hash32(key) & mask;
  for (unsigned it = 0; it <= mask; ++it) {
    const unsigned old = atomicCAS(tab + slot, CV_EMPTY, key);
    if (old == CV_EMPTY) return 1;
    if (old == key) return 0;
    slot = (slot + 1) & mask;
  }
  return 0;
}

__global__ __launch_bounds__(CV_T) void coverage_cells(const float* __restrict__ tmpl_rows, int T, const float* __restrict__ obj_rows, int R, int ld,
                                                       const int32_t* __restrict__ jobs, const double* __restrict__ pose_all, int max_rows,
                                                       unsigned cap_max, unsigned* __restrict__ ws_tab, int32_t* __restrict__ cells,
                                                       int32_t* __restrict__ status) {
  __shared__ unsigned s_tab[BTC_COVERAGE_LDS_KEYS];
  __shared__ double s_ext[CV_WAVES][6];
  __shared__ double s_mn[3], s_n[3];
  const int j = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t0 = jobs[j * 4 + 0], tn = jobs[j * 4 + 1], o0 = jobs[j * 4 + 2], on = jobs[j * 4 + 3];
  const bool bad = t0 < 0 || tn < 0 || o0 < 0 || on < 0 || (long long)t0 + tn > T || (long long)o0 + on > R || tn > max_rows || on > max_rows;
  if (bad) {   // the same in every thread
    if (threadIdx.x == 0) status[j] = BTC_COVERAGE_BAD;
    return;
  }
  if (tn == 0) {
    if (threadIdx.x == 0) cells[j * 2 + 0] = 0, cells[j * 2 + 1] = 0, status[j] = BTC_COVERAGE_OK;
    return;
  }
  const double* pose = pose_all + (size_t)j * 5;
  const float* tmpl = tmpl_rows + (size_t)t0 * 3;
  const float* obj = obj_rows + (size_t)o0 * ld;

  // pass 1: the template's minima and maxima (exact: min and max do not round, so the order does not matter)
  double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {-1e300, -1e300, -1e300};
  for (int i = threadIdx.x; i < tn; i += CV_T) {
    double s[3];
    cv_template_point(tmpl + (size_t)i * 3, pose, s);
#pragma unroll
    for (int k = 0; k < 3; ++k) lo[k] = fmin(lo[k], s[k]), hi[k] = fmax(hi[k], s[k]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = btc_wave_reduce(lo[k], [](double a, double b) { return fmin(a, b); });
    hi[k] = btc_wave_reduce(hi[k], [](double a, double b) { return fmax(a, b); });
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s_ext[wave][k] = lo[k], s_ext[wave][3 + k] = hi[k];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    double mn = s_ext[0][k], mx = s_ext[0][3 + k];
    for (int w = 1; w < CV_WAVES; ++w) mn = fmin(mn, s_ext[w][k]), mx = fmax(mx, s_ext[w][3 + k]);
    s_mn[k] = mn;
    s_n[k] = cv_cell(mx, mn, k) + 11.0;
  }
  __syncthreads();
  const double mn[3] = {s_mn[0], s_mn[1], s_mn[2]}, nk[3] = {s_n[0], s_n[1], s_n[2]};
  if (!(nk[0] <= CV_LIMIT && nk[1] <= CV_LIMIT && nk[2] <= CV_LIMIT)) {   // the same in every thread; a NaN lands here too
    if (threadIdx.x == 0) status[j] = BTC_COVERAGE_WIDE;
    return;
  }

  unsigned cap = 2u * CV_MIN_ROWS;   // the power of two >= 2 * max(tn, on, CV_MIN_ROWS); tn, on < 2^29
  while (cap < 2u * (unsigned)max(tn, on)) cap <<= 1;
  unsigned* tab = cap <= (unsigned)BTC_COVERAGE_LDS_KEYS ? s_tab : ws_tab + (size_t)j * cap_max;   // cap <= cap_max: tn, on <= max_rows
  const unsigned mask = cap - 1;

  // pass 2: the template's cells
  for (unsigned k = threadIdx.x; k < cap; k += CV_T) tab[k] = CV_EMPTY;
  __syncthreads();
  int fresh = 0;
  for (int i = threadIdx.x; i < tn; i += CV_T) {
    double s[3];
    cv_template_point(tmpl + (size_t)i * 3, pose, s);
    unsigned key = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double c = cv_cell(s[k], mn[k], k);   // 0 <= c <= n_k - 11 by the definition of mn and n
      key |= ((unsigned)(int)fmin(fmax(c, 0.0), CV_LIMIT - 1.0)) << (10 * k);
    }
    fresh += cv_insert(tab, mask, key);
  }
  const int unique_bm = btc_block_sum<CV_WAVES>(fresh);

  // pass 3: the object's kept cells, in the cleared table
  __syncthreads();   // every insert of pass 2 has been made
  for (unsigned k = threadIdx.x; k < cap; k += CV_T) tab[k] = CV_EMPTY;
  __syncthreads();
  fresh = 0;
  for (int i = threadIdx.x; i < on; i += CV_T) {
    double s[3];
    cv_object_point(obj + (size_t)i * ld, pose, s);
    unsigned key = 0;
    bool keep = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double c = cv_cell(s[k], mn[k], k);
      keep = keep && (c >= 0.0) && (c < nk[k]);   // a NaN is not kept
      key |= ((unsigned)(int)fmin(fmax(c, 0.0), CV_LIMIT - 1.0)) << (10 * k);
    }
    if (keep) fresh += cv_insert(tab, mask, key);
  }
  const int unique_obj = btc_block_sum<CV_WAVES>(fresh);
  if (threadIdx.x == 0) cells[j * 2 + 0] = unique_obj, cells[j * 2 + 1] = unique_bm, status[j] = BTC_COVERAGE_OK;
}

inline unsigned cv_cap_max(int max_rows) { return btc_pow2_ge(2ull * (unsigned long long)(max_rows > CV_MIN_ROWS ? max_rows : CV_MIN_ROWS)); }

}  // namespace

extern "C" size_t btc_count_in_boxes_ws_bytes(int n, int batch) {
  if (n < 0 || batch < 1) return 0;
  return btc_align((size_t)(batch + 1) * sizeof(int32_t));   // tile_first
}

extern "C" int btc_count_in_boxes(const float* points, int n, int ld, const int32_t* scene_offsets, int batch, const float* calib, const float* boxes,
                                  const int32_t* box_offsets, int m, int32_t* counts, int32_t* fov_rows, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(ld >= 3, "btc_count_in_boxes: need ld >= 3 (x, y, z columns), got %d", ld);
  BTC_CHECK_ARG(batch >= 1, "btc_count_in_boxes: need batch >= 1, got %d", batch);
  BTC_CHECK_ARG(n >= 0 && m >= 0, "btc_count_in_boxes: negative count (n %d, m %d)", n, m);
  BTC_CHECK_ARG(scene_offsets && calib && box_offsets && ws, "btc_count_in_boxes: missing pointer (scene_offsets, calib, box_offsets or ws)");
  BTC_CHECK_ARG(points || n == 0, "btc_count_in_boxes: missing pointer (points)");
  BTC_CHECK_ARG((boxes && counts) || m == 0, "btc_count_in_boxes: missing pointer (boxes or counts)");
  BTC_CHECK_ARG(ws_bytes >= btc_count_in_boxes_ws_bytes(n, batch), "btc_count_in_boxes: workspace too small");
  const long long tmax_ll = gtdb_tmax(n, batch);
  BTC_CHECK_ARG(tmax_ll < (1ll << 31), "btc_count_in_boxes: %lld tiles do not fit 31 bits", tmax_ll);
  const int tmax = (int)tmax_ll;
  BtcCarver c(ws);
  int32_t* tile_first = c.take<int32_t>(batch + 1);
  if (m > 0 || fov_rows != nullptr) {
    infos_zero<<<btc_cdiv(m > batch ? m : batch, GT_T), GT_T, 0, stream>>>(counts, m, fov_rows, batch);
    BTC_LAUNCH_CHECK();
  }
  if (n > 0 && (m > 0 || fov_rows != nullptr)) {
    gtdb_tiles<<<1, 64, 0, stream>>>(scene_offsets, batch, n, tmax, tile_first);
    BTC_LAUNCH_CHECK();
    if (ld == 4 && btc_aligned16(points))
      infos_count<true><<<tmax, GT_T, 0, stream>>>(points, n, ld, scene_offsets, batch, calib, boxes, box_offsets, m, tile_first, counts, fov_rows);
    else
      infos_count<false><<<tmax, GT_T, 0, stream>>>(points, n, ld, scene_offsets, batch, calib, boxes, box_offsets, m, tile_first, counts, fov_rows);
    BTC_LAUNCH_CHECK();
  }
  return BTC_OK;
}

extern "C" size_t btc_coverage_cells_ws_bytes(int J, int max_rows) {
  if (J < 0 || max_rows < 0 || max_rows >= (1 << 29)) return 0;
  const unsigned cap_max = cv_cap_max(max_rows);
  if (cap_max <= (unsigned)BTC_COVERAGE_LDS_KEYS || J == 0) return 256;
  return btc_align((size_t)J * (size_t)cap_max * sizeof(unsigned));
}

extern "C" int btc_coverage_cells(const float* tmpl_rows, int T, const float* obj_rows, int R, int ld, const int32_t* jobs, const double* pose, int J,
                                  int max_rows, int32_t* cells, int32_t* status, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(J >= 0 && T >= 0 && R >= 0, "btc_coverage_cells: negative count (J %d, T %d, R %d)", J, T, R);
  BTC_CHECK_ARG(ld >= 3, "btc_coverage_cells: need ld >= 3 (x, y, z columns), got %d", ld);
  BTC_CHECK_ARG(max_rows >= 0 && max_rows < (1 << 29), "btc_coverage_cells: max_rows %d outside [0, 2^29)", max_rows);
  BTC_CHECK_ARG(ws, "btc_coverage_cells: missing pointer (ws)");
  BTC_CHECK_ARG((jobs && pose && cells && status) || J == 0, "btc_coverage_cells: missing pointer (jobs, pose, cells or status)");
  BTC_CHECK_ARG(tmpl_rows || T == 0, "btc_coverage_cells: missing pointer (tmpl_rows)");
  BTC_CHECK_ARG(obj_rows || R == 0, "btc_coverage_cells: missing pointer (obj_rows)");
  BTC_CHECK_ARG(ws_bytes >= btc_coverage_cells_ws_bytes(J, max_rows), "btc_coverage_cells: workspace too small");
  if (J == 0) return BTC_OK;
  coverage_cells<<<J, CV_T, 0, stream>>>(tmpl_rows, T, obj_rows, R, ld, jobs, pose, max_rows, cv_cap_max(max_rows), (unsigned*)ws, cells, status);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}
