// What the weight-gradient kernels share on the device: conv_wgrad_partial / _partial_p / _rows / _rows_p (conv_wgrad.hip) are callers of
// the five pieces below, each stated once; conv_wgrad_x (conv_wgrad_x.hip) of the tile decode and the tile count (its map ring and its
// slab store, the same statements, stay in the kernel: one instance lost a wave per SIMD through the shared ones):
//   1. register-batched staging: all of a thread's global loads into registers (wg_stage_load), then registers -> LDS (wg_stage_store);
//   2. the accumulator-tile decode (wg_tile) and the slab stores (wg_store_slab_rows, wg_store_slab_offset);
//   3. the map ring of the persistent walks (wg_tiles_of_workgroup, wg_load_map, wg_store_map);
//   4. the 4-row MFMA step loop with both fragments from LDS (wg_mfma_steps);
//   5. the block decode of the offset-major pair (wg_offset_block).
// A piece is shared only where every instance keeps its scratch (none), its LDS and its occupancy: profiles/wgrad_tile_resource_usage.txt.
// Kernels of 256 threads (4 waves) throughout.
#pragma once
#include "btc_common.h"

// ---- 1. staging.  A tile of rows x CPR units (a unit: V = float4 -> 4 channels, V = float -> 1) is dealt to the 256 threads unit by
// unit: e = i * 256 + tid -> row e / CPR, unit e % CPR.  row(r) names the source row of tile row r, or -1: zeros.  Channels [c0, C) of
// the source's C are read.  Load and store are separate calls: the pipelined kernels keep v[] in flight across a barrier and their MFMAs.
// (A KB-deep gather is the same walk over KB * TM rows: (kb * TM + r) * pitch == (e / CPR) * pitch.)
// Where CPR divides 256 a thread keeps its unit and its rows are 256 / CPR apart: said so, the addresses of its loads and of its LDS
// stores differ by constants (derived from e, conv_wgrad_rows<1, 1, 8, 4> kept one address per store: 120 -> 154 VGPRs).  The element
// index is one unsigned 32 x 32 -> 64-bit product plus the channel: rows and channel counts are not negative, and the signed 64-bit
// product's cross terms made the scalar loads of conv_wgrad_partial wait for one another.
template <int CPR>
__device__ __forceinline__ int wg_stage_row(int i, int tid) {
  return 256 % CPR == 0 ? i * (256 / CPR) + tid / CPR : (i * 256 + tid) / CPR;
}
template <int CPR>
__device__ __forceinline__ int wg_stage_unit(int i, int tid) {
  return 256 % CPR == 0 ? tid % CPR : (i * 256 + tid) % CPR;
}
template <bool BF, int CPR, typename V, int NV, typename Row>
__device__ __forceinline__ void wg_stage_load(V (&v)[NV], const float* __restrict__ src, int tid, Row row, int C, int c0) {
  constexpr int W = sizeof(V) / sizeof(float);
  static_assert(W == 4 || W == 1, "float4 or float units");
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int r = wg_stage_row<CPR>(i, tid), c = c0 + wg_stage_unit<CPR>(i, tid) * W;
    const int j = row(r);
    if constexpr (W == 4) v[i] = (j >= 0 && c < C) ? btc_ld4<BF>(src, (size_t)(unsigned)j * (unsigned)C + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    else v[i] = (j >= 0 && c < C) ? btc_ld1<BF>(src, (size_t)(unsigned)j * (unsigned)C + c) : 0.f;
  }
}
// rows: only tile rows below it are written (conv_wgrad_partial_p's packed tiles)
template <int CPR, typename V, int NV>
__device__ __forceinline__ void wg_stage_store(const V (&v)[NV], float* dst, int pitch, int tid, int rows = 1 << 30) {
  constexpr int W = sizeof(V) / sizeof(float);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int r = wg_stage_row<CPR>(i, tid);
    if (r >= rows) continue;
    float* d = dst + r * pitch + wg_stage_unit<CPR>(i, tid) * W;
    if constexpr (W == 4) {
      d[0] = v[i].x; d[1] = v[i].y; d[2] = v[i].z; d[3] = v[i].w;
    } else {
      d[0] = v[i];
    }
  }
}

// ---- 2. accumulator tiles.  Row-stationary kernels: a phase has KB * MT * NT 16 x 16 tiles, wave w owns tiles l = q * 4 + w
struct WgTile {
  int nt, mt, kb;
};
template <int MT, int NT>
__device__ __forceinline__ WgTile wg_tile(int q, int wave) {
  const int l = q * 4 + wave;
  return {l % NT, (l / NT) % MT, l / (NT * MT)};
}

// the slab of a row-stationary workgroup: P[k][cg][cc] (swap: P[k][cc][cg], so that dW keeps its [K][Cin][Cout] layout) for the offsets
// kg0 .. kg0 + PH * KB; value(p, q, r) is row r of the lane's tile q of phase p.  D layout of a
// 16 x 16 tile: column = lane & 15 (the contiguous operand's channel), row = (lane >> 4) * 4 + r (the gathered operand's)
template <int MT, int NT, int KB, int PH, typename Value>
__device__ __forceinline__ void wg_store_slab_rows(float* __restrict__ P, int K, int Cg_all, int Cc_all, int kg0, int swap, Value value) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int p = 0; p < PH; ++p)
#pragma unroll
    for (int q = 0; q < KB * MT * NT / 4; ++q) {
      const WgTile t = wg_tile<MT, NT>(q, wave);
      const int k = kg0 + p * KB + t.kb;
      const int co = t.nt * 16 + (lane & 15);
      if (k >= K || co >= Cc_all) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ci = t.mt * 16 + (lane >> 4) * 4 + r;
        if (ci >= Cg_all) continue;
        const float v = value(p, q, r);
        if (!swap) P[((size_t)k * Cg_all + ci) * Cc_all + co] = v;
        else P[((size_t)k * Cc_all + co) * Cg_all + ci] = v;
      }
    }
}

// the slab of an offset-major workgroup: P[ci][co], the lane's rows ci0 .. ci0 + 4 of NT tiles whose first column for this lane is co0
template <int NT>
__device__ __forceinline__ void wg_store_slab_offset(float* __restrict__ P, int Cin, int Cout, int ci0, int co0, const f32x4 (&acc)[NT]) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int col = co0 + nt * 16;
    if (col >= Cout) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (ci0 + r < Cin) P[(size_t)(ci0 + r) * Cout + col] = acc[nt][r];
  }
}

// ---- 3. the map ring.  A persistent workgroup takes every gridDim.x-th tile of TMROWS rows; its tile i goes to LDS ring slot i % RING:
// the rows through `order` (s_row, RROW slots) and, per row, the NOFF offsets of the workgroup's group (s_nbr[RING][TMROWS][NOFF]).
__device__ __forceinline__ int wg_tiles_of_workgroup(int n_tiles) {
  return ((int)blockIdx.x < n_tiles) ? (n_tiles - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
}
template <int TMROWS, int NOFF>
__device__ __forceinline__ void wg_load_map(int (&nv)[(TMROWS * NOFF + 255) / 256], int& nrow, int i, const int32_t* __restrict__ nbr,
                                            const int32_t* __restrict__ order, int n_rows, int K, int kg0) {
  const int tid = threadIdx.x;
  const int row0 = (blockIdx.x + i * gridDim.x) * TMROWS;
  if (tid < TMROWS) nrow = (row0 + tid < n_rows) ? (order ? order[row0 + tid] : row0 + tid) : -1;
#pragma unroll
  for (int u = 0; u < (TMROWS * NOFF + 255) / 256; ++u) {
    const int e = u * 256 + tid, r = e / NOFF, o = e - r * NOFF;
    int v = -1;
    if (e < TMROWS * NOFF && row0 + r < n_rows && kg0 + o < K) {
      const int gr = order ? order[row0 + r] : row0 + r;
      v = nbr[(long long)gr * K + kg0 + o];
    }
    nv[u] = v;
  }
}
template <int TMROWS, int NOFF, int RING, int RROW>
__device__ __forceinline__ void wg_store_map(const int (&nv)[(TMROWS * NOFF + 255) / 256], int nrow, int i, int32_t* s_nbr, int32_t* s_row) {
  const int tid = threadIdx.x;
  int32_t* dn = s_nbr + (i % RING) * TMROWS * NOFF;
#pragma unroll
  for (int u = 0; u < (TMROWS * NOFF + 255) / 256; ++u) {
    const int e = u * 256 + tid;
    if (e < TMROWS * NOFF) dn[e] = nv[u];
  }
  if (tid < TMROWS) s_row[(i % RROW) * TMROWS + tid] = nrow;
}

// ---- 4. `steps` 4-row MFMA steps of NT tiles that share the A fragment: ap / bp point at the lane's element of row lane >> 4
template <int NT>
__device__ __forceinline__ void wg_mfma_steps(f32x4 (&acc)[NT], const float* ap, int lda, const float* bp, int ldb, int steps) {
#pragma unroll 4
  for (int q = 0; q < steps; ++q) {
    const float a = ap[q * 4 * lda];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[q * 4 * ldb + nt * 16], acc[nt], 0, 0, 0);
  }
}

// ---- 5. offset-major kernels: block = (offset k, row split, tile of 64 Cin x NT * 16 Cout); wave w owns dW rows [m0 + 16 w, m0 + 16 w + 16)
struct WgOffsetBlock {
  int k, split, m0, n0, t_begin, t_end;
  bool wave_live;
};
template <int NT>
__device__ __forceinline__ WgOffsetBlock wg_offset_block(int n_out, int Cin, int tiles_per_split, int n_cblk) {
  WgOffsetBlock b;
  b.k = blockIdx.x, b.split = blockIdx.y;
  b.m0 = (blockIdx.z / n_cblk) * 64;
  b.n0 = (blockIdx.z % n_cblk) * (NT * 16);
  b.t_begin = b.split * tiles_per_split;
  b.t_end = min((n_out + TM - 1) / TM, b.t_begin + tiles_per_split);
  b.wave_live = (b.m0 + (int)(threadIdx.x >> 6) * 16) < Cin;
  return b;
}
