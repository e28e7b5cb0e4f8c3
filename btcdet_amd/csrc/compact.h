// Stable row compaction, stated once (prestep.hip: btc_range_mask_compact, augment.hip: btc_augment_batch, fov_crop.hip: btc_fov_crop):
// drop rows of a resident batch, keep the survivors in input order, give the new scene offsets.  Four launches, no atomics:
//
//   count    btc_compact_count: kept rows per workgroup of BTC_COMPACT_T rows -> block_cnt
//   scan     btc_scan_exclusive_i32 over block_cnt -> block_prefix, total (scan.hip)
//   scatter  btc_compact_rank: a kept row's destination = its workgroup's prefix + the kept rows of the earlier waves + of the lower lanes
//   offsets  btc_compact_boundary: one wave per scene boundary -> kept rows in front of it
//
// The helpers take a `bool keep` and do not know the predicate: the caller decides once and stores a flag byte per row (augment, fov
// crop), or decides again in every stage (range mask: four comparisons are cheaper than a byte written and read).
// The boundary stage's wave sum is wave_ops.h's (as are the scans of aug_offsets' object block, gtdb_offsets and tsel_offsets behind
// the same batches); the rank stage is a ballot and a popcount and stays here.
#pragma once
#include "btc_common.h"   // (wave_ops.h comes with it)

constexpr int BTC_COMPACT_T = 256;   // rows (threads) per workgroup of the count and scatter stages

// largest s in [0, count) with offs[s] <= i (offs ascending, offs[0] <= i): the set that owns row i, empty sets skipped
static __device__ __forceinline__ int aug_owner(const int32_t* __restrict__ offs, int count, int i) {
  int lo = 0, hi = count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offs[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// the scenes [s_lo, s_hi] that own the rows [row0, min(row0 + BTC_COMPACT_T, n)) of one workgroup (row0 < n); uniform in the workgroup
static __device__ __forceinline__ void btc_compact_scene_span(const int32_t* __restrict__ scene_offsets, int batch, int row0, int n, int& s_lo,
                                                              int& s_hi) {
  s_lo = aug_owner(scene_offsets, batch, row0);
  s_hi = aug_owner(scene_offsets, batch, min(row0 + BTC_COMPACT_T, n) - 1);
}

// count stage; every thread of the workgroup calls it
static __device__ __forceinline__ void btc_compact_count(bool keep, int32_t* __restrict__ block_cnt) {
  const int c = __syncthreads_count(keep);
  if (threadIdx.x == 0) block_cnt[blockIdx.x] = c;
}

// scatter stage; every thread of the workgroup calls it (it holds a __syncthreads).  -> the stable destination rank of a kept row.
// A thread with keep == false gets a value it must not use.
static __device__ __forceinline__ int btc_compact_rank(bool keep, const int32_t* __restrict__ block_prefix) {
  __shared__ int s_wave[BTC_COMPACT_T / 64];
  const unsigned long long m = __ballot(keep);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave[wave] = __popcll(m);
  __syncthreads();
  if (!keep) return -1;
  int rank = block_prefix[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) rank += s_wave[w];
  return rank;
}

// offsets stage, one wave: the kept rows in front of boundary s (s == batch: all of them), in every lane.  kept(j) -> 0 / 1 for row j.
// A scene offset outside [0, n] is clamped, so block_prefix is never read out of range.
template <class Kept>
static __device__ __forceinline__ int btc_compact_boundary(int s, const int32_t* __restrict__ scene_offsets, int batch, int n,
                                                           const int32_t* __restrict__ block_prefix, const int32_t* __restrict__ total,
                                                           Kept kept) {
  const int pos = s == batch ? n : min(max(scene_offsets[s], 0), n);
  if (pos >= n) return *total;
  const int blk = pos / BTC_COMPACT_T;
  int cnt = 0;
  for (int j = blk * BTC_COMPACT_T + (int)threadIdx.x; j < pos; j += 64) cnt += kept(j);
  return block_prefix[blk] + btc_wave_all_sum(cnt);
}

// one row of ld floats; VEC4: ld == 4 and both ends 16-byte aligned, one load and one store
template <bool VEC4>
static __device__ __forceinline__ void btc_copy_row(const float* __restrict__ src, float* __restrict__ dst, int ld) {
  if (VEC4) {
    *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
  } else {
    for (int c = 0; c < ld; ++c) dst[c] = src[c];
  }
}

static inline bool btc_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static inline int btc_compact_blocks(int n) { return btc_cdiv(n > 0 ? n : 1, BTC_COMPACT_T); }   // n == 0: one workgroup, it counts nothing

// The workspace of one compaction of n rows: [flag byte per row] block_cnt, block_prefix, total, whatever the caller takes from `c`,
// and the scan's workspace last.
struct BtcCompactWs {
  BtcCarver c;
  int nb;
  unsigned char* keep_flag;   // NULL without flags
  int32_t *block_cnt, *block_prefix, *total;
  BtcCompactWs(void* ws, int n, bool flags) : c(ws), nb(btc_compact_blocks(n)) {
    keep_flag = flags ? c.take<unsigned char>(n > 0 ? n : 1) : nullptr;
    block_cnt = c.take<int32_t>(nb + 1);
    block_prefix = c.take<int32_t>(nb + 1);
    total = c.take<int32_t>(1);
  }
  void* scan_ws() const { return c.base + c.off; }
  int scan(hipStream_t stream) const { return btc_scan_exclusive_i32(block_cnt, block_prefix, nb, total, scan_ws(), stream); }
  static size_t bytes(int n, bool flags) {
    const long long nb = btc_compact_blocks(n);
    return (flags ? btc_align((size_t)(n > 0 ? n : 1)) : 0) + btc_align((size_t)(nb + 1) * sizeof(int32_t)) * 2 + 256 + btc_scan_ws_bytes(nb);
  }
};
