// The objects of a ground-truth database cut from a resident batch of raw scans for gfx950 (include/btcdet_hip_gtdb.h: btc_cut_objects).
//
// A compaction per box instead of one per batch: row i of scene s goes to every object of s whose box it is inside.  Tiles of 256 rows
// are aligned to scenes (tile t of scene s covers rows scene_offsets[s] + 256 t ..), so a tile meets the boxes of one scene only and
// their number is at most ceil(n / 256) + batch, a bound the host knows.
//
//   gtdb_tiles    one wave ranks the scenes' tile counts -> tile_first (batch + 1).
//   gtdb_count    one workgroup per tile.  It stages its scene's box rows in LDS 64 at a time (as aug_mark does; no cap on their number
//                 but max_boxes), tests its rows with aug_in_box (aug_ops.h: the removal test of btc_augment_batch, unfused float32) and
//                 counts with one ballot per box: lane k of a wave holds the wave's rows inside box k -> cnt[tile][k].
//   gtdb_box_scan one wave per box walks its scene's tiles: its column of cnt becomes the exclusive prefix in place -> obj_total[j].
//   gtdb_offsets  one wave ranks the totals -> obj_offsets (m + 1), true whatever out_capacity is.
//   gtdb_scatter  one workgroup per tile makes the same decisions through the same function on the same bits, so count and scatter
//                 cannot disagree: dst = obj_offsets[j] + cnt[tile][k] + the rows of the earlier waves + of the lower lanes.  The row
//                 goes out with columns 0..2 shifted in double (one rounding) and the rest copied.
//
// A stream: gtdb_count reads 16 B per row, gtdb_scatter reads them again and writes 16 (+ 4) B per row that is inside a box; the box
// rows come from LDS at one broadcast read per (row, box).  Measured (tools/gt_database_bench.py): 19.9 us for the five launches at
// 2 KITTI-sized frames -- launch latency -- and 142 us at 64 frames (7.8 M rows), 1.78 TB/s of those bytes.  No atomics, no memset, no ticket: every workspace word a kernel reads was
// written by an earlier launch of the same call.  Every index formed from a device array is clamped to n, m, max_boxes, the tile
// bound or out_capacity before it addresses anything.
#include "aug_ops.h"   // aug_in_box; compact.h: aug_owner, btc_aligned16, BTC_COMPACT_T
#include "scene_tiles.h"   // GT_T, gtdb_span, gtdb_tiles, GtTile, gtdb_tile, gtdb_load, gtdb_tmax: shared with kitti_infos.hip

#include "../../include/btcdet_hip_gtdb.h"

namespace {

constexpr int GT_WAVES = GT_T / 64;
constexpr int GT_BOX_CHUNK = 64;   // boxes staged per pass: one per lane of a wave, one bit of a 64-bit mask

// One chunk of nb <= 64 boxes (rows `chunk` of the box array) against the workgroup's rows; every thread calls it (three barriers).
// -> bit k: this thread's row is inside box k of the chunk.  s_wcnt[w][k] = rows of wave w inside box k (0 for k >= nb);
// wave_boxes: bit k = some row of this thread's wave is inside box k.
__device__ __forceinline__ unsigned long long gtdb_chunk(const float* __restrict__ chunk, int nb, bool live, float x, float y, float z,
                                                         float* __restrict__ s_box, int (*__restrict__ s_wcnt)[64],
                                                         unsigned long long& wave_boxes) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();   // the previous chunk's LDS has been read
  for (int k = threadIdx.x; k < nb * 8; k += GT_T) s_box[k] = chunk[k];
  __syncthreads();
  unsigned long long in = 0;
  int mine = 0;
  for (int k = 0; k < nb; ++k) {
    const bool hit = live && aug_in_box(x, y, z, s_box + k * 8);
    const unsigned long long mk = __ballot(hit);
    if (lane == k) mine = __popcll(mk);
    if (hit) in |= 1ull << k;
  }
  s_wcnt[wave][lane] = mine;
  wave_boxes = __ballot(mine > 0);
  __syncthreads();
  return in;
}

template <bool VEC4>
__global__ __launch_bounds__(GT_T) void gtdb_count(const float* __restrict__ pts, int n, int ld, const int32_t* __restrict__ scene_offsets, int batch,
                                                   const float* __restrict__ boxes, const int32_t* __restrict__ box_offsets, int m, int max_boxes,
                                                   const int32_t* __restrict__ tile_first, int32_t* __restrict__ cnt) {
  __shared__ float s_box[GT_BOX_CHUNK * 8];
  __shared__ int s_wcnt[GT_WAVES][64];
  GtTile t;
  if (!gtdb_tile(tile_first, scene_offsets, batch, n, box_offsets, m, max_boxes, t)) return;
  const long long i = t.row0 + threadIdx.x;
  const bool live = i < t.hi;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) p = gtdb_load<VEC4>(pts + (size_t)i * ld);
  int32_t* mine = cnt + (size_t)blockIdx.x * max_boxes;
  for (int c0 = 0; c0 < t.nbox; c0 += GT_BOX_CHUNK) {
    const int nb = min(GT_BOX_CHUNK, t.nbox - c0);
    unsigned long long wave_boxes;
    gtdb_chunk(boxes + (size_t)(t.b0 + c0) * 8, nb, live, p.x, p.y, p.z, s_box, s_wcnt, wave_boxes);
    if ((int)threadIdx.x < nb) {
      int c = 0;
      for (int w = 0; w < GT_WAVES; ++w) c += s_wcnt[w][threadIdx.x];
      mine[c0 + threadIdx.x] = c;
    }
  }
}

// one wave per box j: cnt[tile][k] over the tiles of its scene -> the exclusive prefix in place, obj_total[j] = the sum
__global__ __launch_bounds__(64) void gtdb_box_scan(const int32_t* __restrict__ box_offsets, int batch, int m, int max_boxes,
                                                    const int32_t* __restrict__ tile_first, int32_t* __restrict__ cnt,
                                                    int32_t* __restrict__ obj_total) {
  const int j = blockIdx.x;
  const int s = aug_owner(box_offsets, batch, j);
  int b0, b1;
  gtdb_span(box_offsets, s, m, b0, b1);
  const int k = j - b0;
  int run = 0;
  if (j >= b0 && j < b1 && k < max_boxes) {
    const int t0 = tile_first[s], t1 = tile_first[s + 1];
    int32_t* c = cnt + (size_t)t0 * max_boxes + k;   // box k's cell of the scene's first tile; the next tile's is max_boxes further on
    run = btc_wave_excl_scan_chunks<int>(t1 - t0, [=](int t) { return c[(size_t)t * max_boxes]; },
                                         [=](int t, int prefix) { c[(size_t)t * max_boxes] = prefix; });
  }
  if (threadIdx.x == 0) obj_total[j] = run;
}

// obj_offsets[j] = rows of the objects in front of object j, obj_offsets[m] = all
__global__ __launch_bounds__(64) void gtdb_offsets(const int32_t* __restrict__ obj_total, int m, int32_t* __restrict__ obj_offsets) {
  btc_wave_offsets_of_counts(obj_total, m, obj_offsets);
}

template <bool VEC4>
__global__ __launch_bounds__(GT_T) void gtdb_scatter(const float* __restrict__ pts, int n, int ld, const int32_t* __restrict__ scene_offsets, int batch,
                                                     const float* __restrict__ boxes, const double* __restrict__ centre,
                                                     const int32_t* __restrict__ box_offsets, int m, int max_boxes,
                                                     const int32_t* __restrict__ tile_first, const int32_t* __restrict__ cnt,
                                                     const int32_t* __restrict__ obj_offsets, int out_capacity, float* __restrict__ out,
                                                     int32_t* __restrict__ src_idx) {
  __shared__ float s_box[GT_BOX_CHUNK * 8];
  __shared__ int s_wcnt[GT_WAVES][64];
  __shared__ int s_base[GT_WAVES][64];   // [w][k]: the destination of wave w's first row inside box k
  GtTile t;
  if (!gtdb_tile(tile_first, scene_offsets, batch, n, box_offsets, m, max_boxes, t)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long i = t.row0 + threadIdx.x;
  const bool live = i < t.hi;
  const float* src = pts + (size_t)(live ? i : 0) * ld;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) p = gtdb_load<VEC4>(src);
  const int32_t* prefix = cnt + (size_t)blockIdx.x * max_boxes;
  for (int c0 = 0; c0 < t.nbox; c0 += GT_BOX_CHUNK) {
    const int nb = min(GT_BOX_CHUNK, t.nbox - c0);
    unsigned long long wave_boxes;
    const unsigned long long in = gtdb_chunk(boxes + (size_t)(t.b0 + c0) * 8, nb, live, p.x, p.y, p.z, s_box, s_wcnt, wave_boxes);
    if (lane < nb) {
      int base = obj_offsets[t.b0 + c0 + lane] + prefix[c0 + lane];
      for (int w = 0; w < wave; ++w) base += s_wcnt[w][lane];
      s_base[wave][lane] = base;
    }
    __syncthreads();
    while (wave_boxes != 0) {   // the boxes that hold a row of this wave; the same in every lane
      const int k = __ffsll((long long)wave_boxes) - 1;
      wave_boxes &= wave_boxes - 1;
      const bool hit = (in >> k) & 1ull;
      const unsigned long long mk = __ballot(hit);
      const long long dst = (long long)s_base[wave][k] + __popcll(mk & ((1ull << lane) - 1ull));
      if (hit && dst >= 0 && dst < out_capacity) {
        const double* c = centre + (size_t)(t.b0 + c0 + k) * 3;
        const float x = (float)((double)p.x - c[0]), y = (float)((double)p.y - c[1]), z = (float)((double)p.z - c[2]);
        float* o = out + (size_t)dst * ld;
        if (VEC4) {
          *reinterpret_cast<float4*>(o) = make_float4(x, y, z, p.w);
        } else {
          o[0] = x, o[1] = y, o[2] = z;
          for (int col = 3; col < ld; ++col) o[col] = src[col];
        }
        if (src_idx) src_idx[dst] = (int32_t)i;
      }
    }
  }
}

}  // namespace

extern "C" size_t btc_cut_objects_ws_bytes(int n, int batch, int m, int max_boxes) {
  if (n < 0 || batch < 1 || m < 0 || max_boxes < 0) return 0;
  const size_t cells = (size_t)gtdb_tmax(n, batch) * (size_t)max_boxes;
  return btc_align((size_t)(batch + 1) * sizeof(int32_t)) + btc_align((cells > 0 ? cells : 1) * sizeof(int32_t)) +
         btc_align((size_t)(m > 0 ? m : 1) * sizeof(int32_t));   // tile_first, cnt, obj_total
}

extern "C" int btc_cut_objects(const float* points, int n, int ld, const int32_t* scene_offsets, int batch, const float* boxes, const double* centre,
                               const int32_t* box_offsets, int m, int max_boxes, int out_capacity, float* out, int32_t* obj_offsets,
                               int32_t* src_idx, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(ld >= 3, "btc_cut_objects: need ld >= 3 (x, y, z columns), got %d", ld);
  BTC_CHECK_ARG(batch >= 1, "btc_cut_objects: need batch >= 1, got %d", batch);
  BTC_CHECK_ARG(n >= 0 && m >= 0 && max_boxes >= 0 && out_capacity >= 0, "btc_cut_objects: negative count (n %d, m %d, max_boxes %d, out_capacity %d)",
                n, m, max_boxes, out_capacity);
  BTC_CHECK_ARG(scene_offsets && box_offsets && obj_offsets && ws, "btc_cut_objects: missing pointer (scene_offsets, box_offsets, obj_offsets or ws)");
  BTC_CHECK_ARG(points || n == 0, "btc_cut_objects: missing pointer (points)");
  BTC_CHECK_ARG((boxes && centre) || m == 0, "btc_cut_objects: missing pointer (boxes or centre)");
  BTC_CHECK_ARG(out || out_capacity == 0, "btc_cut_objects: missing pointer (out)");
  BTC_CHECK_ARG(ws_bytes >= btc_cut_objects_ws_bytes(n, batch, m, max_boxes), "btc_cut_objects: workspace too small");
  const long long tmax_ll = gtdb_tmax(n, batch);
  BTC_CHECK_ARG(tmax_ll < (1ll << 31), "btc_cut_objects: %lld tiles do not fit 31 bits", tmax_ll);
  const int tmax = (int)tmax_ll;
  BtcCarver c(ws);
  int32_t* tile_first = c.take<int32_t>(batch + 1);
  const size_t cells = (size_t)tmax * (size_t)max_boxes;
  int32_t* cnt = c.take<int32_t>(cells > 0 ? cells : 1);
  int32_t* obj_total = c.take<int32_t>(m > 0 ? m : 1);
  const bool rows = n > 0 && m > 0 && max_boxes > 0;   // otherwise every object is empty
  const bool vec = ld == 4 && btc_aligned16(points) && btc_aligned16(out);
  gtdb_tiles<<<1, 64, 0, stream>>>(scene_offsets, batch, n, tmax, tile_first);
  BTC_LAUNCH_CHECK();
  if (rows) {
    if (vec) gtdb_count<true><<<tmax, GT_T, 0, stream>>>(points, n, ld, scene_offsets, batch, boxes, box_offsets, m, max_boxes, tile_first, cnt);
    else gtdb_count<false><<<tmax, GT_T, 0, stream>>>(points, n, ld, scene_offsets, batch, boxes, box_offsets, m, max_boxes, tile_first, cnt);
    BTC_LAUNCH_CHECK();
  }
  if (m > 0) {
    gtdb_box_scan<<<m, 64, 0, stream>>>(box_offsets, batch, m, rows ? max_boxes : 0, tile_first, cnt, obj_total);
    BTC_LAUNCH_CHECK();
  }
  gtdb_offsets<<<1, 64, 0, stream>>>(obj_total, m, obj_offsets);
  BTC_LAUNCH_CHECK();
  if (rows && out_capacity > 0) {
    if (vec)
      gtdb_scatter<true><<<tmax, GT_T, 0, stream>>>(points, n, ld, scene_offsets, batch, boxes, centre, box_offsets, m, max_boxes, tile_first, cnt,
                                                    obj_offsets, out_capacity, out, src_idx);
    else
      gtdb_scatter<false><<<tmax, GT_T, 0, stream>>>(points, n, ld, scene_offsets, batch, boxes, centre, box_offsets, m, max_boxes, tile_first, cnt,
                                                     obj_offsets, out_capacity, out, src_idx);
    BTC_LAUNCH_CHECK();
  }
  return BTC_OK;
}
