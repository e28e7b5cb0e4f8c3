// Tiles of 256 rows aligned to scenes, stated once (gt_database.hip: btc_cut_objects, kitti_infos.hip: btc_count_in_boxes): tile t of
// scene s covers rows scene_offsets[s] + 256 t .., so a tile meets the boxes (and the calibration) of one scene only and the number of
// tiles is at most ceil(n / 256) + batch, a bound the host knows.  Every index formed from a device array is clamped before use.
// gtdb_tiles is one wave over the scenes: wave_ops.h's chunked exclusive scan in 64 bits, clamped to tmax as it stores.
#pragma once
#include "compact.h"   // aug_owner, BTC_COMPACT_T; btc_wave_excl_scan_chunks through btc_common.h

namespace {

constexpr int GT_T = BTC_COMPACT_T;

// set s of an offsets array as [lo, hi), clamped to [0, limit] and to ascending order
__device__ __forceinline__ void gtdb_span(const int32_t* __restrict__ offs, int s, int limit, int& lo, int& hi) {
  lo = min(max(offs[s], 0), limit);
  hi = min(max(offs[s + 1], lo), limit);
}

// tile_first[s] = tiles in front of scene s, tile_first[batch] = all of them; never above tmax
__global__ __launch_bounds__(64) void gtdb_tiles(const int32_t* __restrict__ scene_offsets, int batch, int n, int tmax,
                                                 int32_t* __restrict__ tile_first) {
  const long long all = btc_wave_excl_scan_chunks<long long>(
      batch,
      [=](int s) {
        int lo, hi;
        gtdb_span(scene_offsets, s, n, lo, hi);
        return ((long long)hi - lo + GT_T - 1) / GT_T;
      },
      [=](int s, long long prefix) { tile_first[s] = (int32_t)min(prefix, (long long)tmax); });
  if (threadIdx.x == 0) tile_first[batch] = (int32_t)min(all, (long long)tmax);
}

// what a workgroup knows of its tile, the same in every thread
struct GtTile {
  int s;           // the scene
  long long row0;  // the tile's first row
  int hi;          // the scene's end: row i of the tile is live while i < hi
  int b0, nbox;    // the scene's boxes [b0, b0 + nbox), nbox <= max_boxes
};

__device__ __forceinline__ bool gtdb_tile(const int32_t* __restrict__ tile_first, const int32_t* __restrict__ scene_offsets, int batch, int n,
                                          const int32_t* __restrict__ box_offsets, int m, int max_boxes, GtTile& t) {
  const int tile = blockIdx.x;
  if (tile >= tile_first[batch]) return false;
  t.s = aug_owner(tile_first, batch, tile);
  int lo, b1;
  gtdb_span(scene_offsets, t.s, n, lo, t.hi);
  t.row0 = (long long)lo + (long long)(tile - tile_first[t.s]) * GT_T;
  gtdb_span(box_offsets, t.s, m, t.b0, b1);
  t.nbox = min(b1 - t.b0, max_boxes);
  return true;
}

template <bool VEC4>
__device__ __forceinline__ float4 gtdb_load(const float* __restrict__ p) {
  if (VEC4) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], 0.f);
}

// tiles aligned to scenes: every scene adds at most one partly filled tile
inline long long gtdb_tmax(int n, int batch) { return ((long long)n + GT_T - 1) / GT_T + batch; }

}  // namespace
