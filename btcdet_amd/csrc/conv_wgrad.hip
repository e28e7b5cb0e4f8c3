// Sparse convolution weight gradient for gfx950: the fp32-matrix-pipe kernels (offset-major conv_wgrad_partial / _partial_p, row-stationary
// conv_wgrad_rows / _rows_p), the slab reductions, and the ONE planner that picks a kernel family and its slab count for every
// weight-gradient call -- the families of conv_wgrad_x.hip (bf16 matrix pipe) and conv_wgrad_n.hip (narrow layers) included.
//
// Every family writes S partial sums ("slabs") of K * Cin * Cout floats into the caller's workspace; wgrad_reduce adds them up in slab
// order (deterministic).  A family's plan function fills the launch record of conv_wgrad.h (instance, grid, LDS bytes, S) or refuses the
// shape; btc_conv_wgrad_ws_bytes asks the same plan functions (wgrad_max_slabs), and the launch is the record's: L.fn(L, a).
//
// The four kernels here are callers of wgrad_tile.h for what they share on the device: the register-batched staging of both operands,
// the accumulator-tile decode and the slab stores, the map ring of conv_wgrad_rows_p, the LDS / LDS MFMA step loop and the block decode
// of the offset-major pair.  What is written out in a kernel is what only that kernel has.
#include "conv_wgrad.h"
#include "wgrad_tile.h"

namespace {

// dW partial: part[s][k][ci][co] = sum over the split's rows of feat[nbr[i][k]][ci] * dout[i][co]
// block = (k, split, tile of 64 Cin x NT*16 Cout); wave w owns dW rows [m0 + 16w, m0 + 16w + 16)
constexpr int WG_LDA = 64 + 16;
template <int NT, bool BF>
__global__ __launch_bounds__(256) void conv_wgrad_partial(const float* __restrict__ feat, const float* __restrict__ dout,
                                                          const int32_t* __restrict__ nbr, int n_out, int K, int Cin,
                                                          int Cout, int tiles_per_split, int n_cblk, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int LDB = ldb_of(NT);
  float* As = (float*)smem;       // [TM][WG_LDA]  gathered input rows, 64 channels
  float* Ds = As + TM * WG_LDA;   // [TM][LDB]     dout rows, NT*16 channels
  int32_t* s_j = (int32_t*)(Ds + TM * LDB);  // [TM] (kept inside the one dynamic LDS array)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4;
  const WgOffsetBlock B = wg_offset_block<NT>(n_out, Cin, tiles_per_split, n_cblk);
  const int k = B.k, m0 = B.m0, n0 = B.n0;

  f32x4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int t = B.t_begin; t < B.t_end; ++t) {
    const int row0 = t * TM;
    int j = -1;
    if (tid < TM && row0 + tid < n_out) j = nbr[(size_t)(row0 + tid) * K + k];
    if (tid < TM) s_j[tid] = j;
    if (!__syncthreads_or(j >= 0)) continue;
    // all loads of a thread are issued before the first LDS store (one memory latency per tile)
    auto arow = [&](int r) { return s_j[r]; };
    auto drow = [&](int r) { return s_j[r] >= 0 ? row0 + r : -1; };
    if (((Cin | Cout) & 3) == 0) {
      float4 va[4], vd[NT];
      wg_stage_load<BF, 16>(va, feat, tid, arow, Cin, m0);
      wg_stage_load<BF, NT * 4>(vd, dout, tid, drow, Cout, n0);
      wg_stage_store<16>(va, As, WG_LDA, tid);
      wg_stage_store<NT * 4>(vd, Ds, LDB, tid);
    } else {
      float va[16], vd[NT * 4];
      wg_stage_load<BF, 64>(va, feat, tid, arow, Cin, m0);
      wg_stage_load<BF, NT * 16>(vd, dout, tid, drow, Cout, n0);
      wg_stage_store<64>(va, As, WG_LDA, tid);
      wg_stage_store<NT * 16>(vd, Ds, LDB, tid);
    }
    __syncthreads();
    if (B.wave_live) wg_mfma_steps<NT>(acc, As + kq * WG_LDA + wave * 16 + (lane & 15), WG_LDA, Ds + kq * LDB + (lane & 15), LDB, TM / 4);
    __syncthreads();
  }
  wg_store_slab_offset<NT>(part + ((size_t)B.split * K + k) * Cin * Cout, Cin, Cout, m0 + wave * 16 + kq * 4, n0 + (lane & 15), acc);
}

// conv_wgrad_partial for channel counts that are multiples of 4, with
//  * the next tile's loads in flight during this tile's MFMAs: the map column entry of tile t + 1 is read while tile t is being
//    staged, its gathered rows and dOut rows are requested right after tile t's tiles are visible in LDS and sit in registers
//    until tile t's MFMAs are done (same LDS footprint, same two barriers per tile);
//  * per-tile packing: only the rows of the tile that HAVE the offset are staged, packed to the front of the LDS tiles (a wave
//    ballot over the column gives every live row its slot), and the reduction runs over ceil(m / 4) 4-row steps instead of 16.
//    Both operands are gathered per offset here anyway, so packing costs no indirection in the MFMA loop.  At the wide layers
//    that land on this kernel (128 -> 128, 256 -> 128 on the 8x-downsampled level) 55 % of the (row, offset) slots are live.
// Skipped terms are exact zeros; dW differs from the unpacked sum only in how rows group into 4-row MFMA steps.
template <int NT, bool BF>
__global__ __launch_bounds__(256) void conv_wgrad_partial_p(const float* __restrict__ feat, const float* __restrict__ dout,
                                                            const int32_t* __restrict__ nbr, int n_out, int K, int Cin, int Cout,
                                                            int tiles_per_split, int n_cblk, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int LDB = ldb_of(NT);
  float* As = (float*)smem;       // [TM][WG_LDA]  gathered input rows (packed), 64 channels
  float* Ds = As + TM * WG_LDA;   // [TM][LDB]     dout rows (packed), NT*16 channels
  int32_t* s_src = (int32_t*)(Ds + TM * LDB);  // [2][TM] input row of packed slot t (-1: padding of the last 4-row step)
  int32_t* s_dst = s_src + 2 * TM;             // [2][TM] output row of packed slot t
  int32_t* s_m = s_dst + 2 * TM;               // [2] live rows of the tile

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4;
  const WgOffsetBlock B = wg_offset_block<NT>(n_out, Cin, tiles_per_split, n_cblk);
  const int k = B.k, m0 = B.m0, n0 = B.n0, t_begin = B.t_begin, t_end = B.t_end;

  f32x4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  float4 va[4], vd[NT];
  auto load_j = [&](int t) {   // wave 0: map column entry of row `lane` of tile t
    const int row = t * TM + lane;
    return (wave == 0 && t < t_end && row < n_out) ? nbr[(size_t)row * K + k] : -1;
  };
  auto pack = [&](int t, int j, int b) {   // wave 0: packed slots of tile t into buffer b
    if (wave != 0) return;
    const unsigned long long live = __ballot(j >= 0);
    const int m = __popcll(live);
    if (j >= 0) {
      const int slot = __popcll(live & ((1ull << lane) - 1ull));
      s_src[b * TM + slot] = j;
      s_dst[b * TM + slot] = t * TM + lane;
    }
    if (lane >= m && lane < ((m + 3) & ~3)) {
      s_src[b * TM + lane] = -1;
      s_dst[b * TM + lane] = -1;
    }
    if (lane == 0) s_m[b] = m;
  };
  auto load_tile = [&](int b) {
    const int m4 = (s_m[b] + 3) & ~3;
    wg_stage_load<BF, 16>(va, feat, tid, [&](int r) { return r < m4 ? s_src[b * TM + r] : -1; }, Cin, m0);
    wg_stage_load<BF, NT * 4>(vd, dout, tid, [&](int r) { return r < m4 ? s_dst[b * TM + r] : -1; }, Cout, n0);
  };
  auto store_tile = [&](int m4) {
    wg_stage_store<16>(va, As, WG_LDA, tid, m4);
    wg_stage_store<NT * 4>(vd, Ds, LDB, tid, m4);
  };

  // prologue: the first tile's column and loads, the second tile's column
  int m4 = 0, jn = -1;
  if (t_begin < t_end) {
    pack(t_begin, load_j(t_begin), 0);
    __syncthreads();
    m4 = (s_m[0] + 3) & ~3;
    if (m4) load_tile(0);
    jn = load_j(t_begin + 1);
  }
  for (int t = t_begin; t < t_end; ++t) {
    const int cur = (t - t_begin) & 1;
    if (m4) store_tile(m4);            // tile t: registers -> LDS (the previous tile's MFMAs ended at the barrier below)
    pack(t + 1, jn, cur ^ 1);          // tile t + 1's packed slots
    __syncthreads();                   // tile t in LDS; everyone sees tile t + 1's slots
    const int m4_next = (s_m[cur ^ 1] + 3) & ~3;
    if (m4_next) load_tile(cur ^ 1);   // in flight during the MFMAs below
    jn = load_j(t + 2);
    if (m4 && B.wave_live) wg_mfma_steps<NT>(acc, As + kq * WG_LDA + wave * 16 + (lane & 15), WG_LDA, Ds + kq * LDB + (lane & 15), LDB, m4 >> 2);
    __syncthreads();   // MFMAs of tile t done: the LDS tiles may be overwritten
    m4 = m4_next;
  }
  wg_store_slab_offset<NT>(part + ((size_t)B.split * K + k) * Cin * Cout, Cin, Cout, m0 + wave * 16 + kq * 4, n0 + (lane & 15), acc);
}

// ------------------------------------------------------------------------------------------------------------
// Row-stationary weight gradient for the large-N / small-C layers (the occupancy branch: up to 210 K rows at 32
// channels).  A persistent workgroup walks row tiles; per tile the dOut rows and the neighbour-map rows are loaded
// ONCE (coalesced, row-major) and the K offsets are processed in phases of KB gathered input tiles; the whole
// dW slab of the workgroup's offset group (PH*KB offsets x Cin x Cout) lives in MFMA accumulators for the entire
// walk and is written out once.  (The offset-major kernel below re-reads dOut K times and reads the map column-wise.)
//   MT, NT : 16-wide tiles of Cin / Cout;  KB : offsets per LDS phase;  PH : phases per offset group
// ------------------------------------------------------------------------------------------------------------
template <int MT, int NT, int KB, int PH, bool BF>
__global__ __launch_bounds__(256) void conv_wgrad_rows(const float* __restrict__ feat, const float* __restrict__ dout,
                                                       const int32_t* __restrict__ nbr, const int32_t* __restrict__ order, int n_out, int K,
                                                       int Cin, int Cout, float* __restrict__ part, int swap, int dbg) {
  // order (optional, row_order.hip): tile slot t works on map row order[t]; rows with the same offsets share tiles, so fewer
  // offset phases per tile are live.  dW is the fp32 sum over rows in walk order.
  // Naming follows the un-swapped case: `feat` = gathered operand (Cin channels, via the map), `dout` = contiguous
  // operand (Cout channels), one tile per 64 map rows.  swap = 1: the walk is over the INPUT rows instead (map =
  // nbr_in, gathered = dOut, contiguous = features) -- used when the layer has far fewer input than output rows
  // (transposed / dilating convs) -- and the slab is written transposed so that dW keeps the [K][Cin][Cout] layout.
  constexpr int TPP = KB * MT * NT / 4;  // accumulator tiles per wave per phase
  static_assert(KB * MT * NT % 4 == 0, "phase tiles must split evenly over the 4 waves");
  constexpr int LDA = ldb_of(MT), LDB = ldb_of(NT);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* As = (float*)smem;                       // [KB][TM][LDA]
  float* Ds = As + KB * TM * LDA;                 // [TM][LDB]
  int32_t* s_nbr = (int32_t*)(Ds + TM * LDB);     // [TM][K]
  int32_t* s_kact = s_nbr + TM * K;               // [K]
  int32_t* s_row = s_kact + K;                    // [TM] map row of each tile slot, -1 past the end

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4;
  const int kg0 = blockIdx.y * (PH * KB);         // first offset of this workgroup's group
  const int n_tiles = (n_out + TM - 1) / TM;

  f32x4 acc[PH * TPP];
#pragma unroll
  for (int t = 0; t < PH * TPP; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int row0 = tile * TM;
    for (int e = tid; e < K; e += 256) s_kact[e] = 0;
    if (tid < TM) s_row[tid] = (row0 + tid < n_out) ? (order ? order[row0 + tid] : row0 + tid) : -1;
    __syncthreads();
    for (int e = tid; e < TM * K; e += 256) {
      const int rloc = e / K, kk = e - rloc * K;
      const int gr = s_row[rloc];
      const int v = gr >= 0 ? nbr[(long long)gr * K + kk] : -1;
      s_nbr[e] = v;
      if (v >= 0) s_kact[kk] = 1;
    }
    // dOut tile: all loads of a thread are issued before the first LDS store (one latency, not one per element)
    auto drow = [&](int r) { return s_row[r]; };
    if ((Cout & 3) == 0) {
      float4 v[NT];
      wg_stage_load<BF, NT * 4>(v, dout, tid, drow, Cout, 0);
      wg_stage_store<NT * 4>(v, Ds, LDB, tid);
    } else {
      float v[NT * 4];
      wg_stage_load<BF, NT * 16>(v, dout, tid, drow, Cout, 0);
      wg_stage_store<NT * 16>(v, Ds, LDB, tid);
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < PH; ++p) {
      const int k0 = kg0 + p * KB;
      int any = 0;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) any |= (k0 + kb < K) ? s_kact[k0 + kb] : 0;
      if (!any) continue;  // block-uniform
      // gather KB input tiles (As row kb * TM + r: offset k0 + kb of tile row r); loads batched in registers as above
      auto grow = [&](unsigned ra) {   // (unsigned: the divisions by TM are shifts)
        const int r = ra % TM, kb = ra / TM;
        return (k0 + kb < K) ? s_nbr[r * K + k0 + kb] : -1;
      };
      if ((Cin & 3) == 0) {
        float4 v[KB * MT];
        // dbg & 8: timing experiments only (BTC_TUNE_APPLY_DEBUG, tools/wgrad_bench.py): no gathers
        wg_stage_load<BF, MT * 4>(v, feat, tid, [&](unsigned ra) { const int j = grow(ra); return (dbg & 8) ? -1 : j; }, Cin, 0);
        wg_stage_store<MT * 4>(v, As, LDA, tid);
      } else {
        float v[KB * MT * 4];
        wg_stage_load<BF, MT * 16>(v, feat, tid, grow, Cin, 0);
        wg_stage_store<MT * 16>(v, As, LDA, tid);
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < TPP; ++q) {
        if (dbg & 4) continue;       // timing experiments only: no MFMA phase
        const WgTile t = wg_tile<MT, NT>(q, wave);  // phase-local tile: (kb, mt, nt)
        f32x4 a4[1] = {acc[p * TPP + q]};
        wg_mfma_steps<1>(a4, As + (size_t)t.kb * TM * LDA + t.mt * 16 + (lane & 15) + kq * LDA, LDA, Ds + t.nt * 16 + (lane & 15) + kq * LDB, LDB, TM / 4);
        acc[p * TPP + q] = a4[0];
      }
      __syncthreads();
    }
  }
  // write this workgroup's slab: part[blockIdx.x][k][ci][co] (swap: ci indexes dOut channels, co feature channels)
  wg_store_slab_rows<MT, NT, KB, PH>(part + (size_t)blockIdx.x * K * Cin * Cout, K, Cin, Cout, kg0, swap,
                                     [&](int p, int q, int r) { return acc[p * TPP + q][r]; });
}

// ------------------------------------------------------------------------------------------------------------
// conv_wgrad_rows, software-pipelined (gathered-operand channel counts that are multiples of 4).  tools/wgrad_bench.py on the
// kernel above: removing the MFMA phase halves its time, removing the gathers changes nothing -- a workgroup alternates
// between a staging round (issue the loads, wait one L2 / HBM latency, store to LDS, barrier: ~1.8 us) and an MFMA phase of
// about the same length, and only the other workgroup of the CU fills the holes.  Here
//  * the loads of item g + 1 (the gathered rows of the next phase; the map rows of the tile after next) are issued right
//    after item g's barrier and land in registers while item g's MFMAs run; they are stored to the OTHER LDS buffer at the
//    top of item g + 1: one barrier per item, no exposed load latency;
//  * the contiguous operand never goes through LDS: 4 % NT == 0, so a wave's accumulator tiles all share ONE 16-column block
//    (nt = wave % NT), and its MFMA B fragments for the 16 4-row steps of a tile are 16 registers, loaded once per tile
//    (prefetched during the previous tile's last phase) and reused by every offset of the group.  Half the LDS reads of the
//    MFMA loop, and the LDS footprint drops to the double-buffered gather tile: 41-64 KB, two to three workgroups per CU.
// Same tiles, same 4-row MFMA steps, same order over rows as the kernel above.  Items are all (tile, phase) pairs: a phase
// none of whose offsets occurs in the tile costs zeros -- at 64-row tiles that is < 10 % of the phases of the layers this
// kernel takes.
//   LDS: As[2][KB][TM][LDA] | s_nbr[3][TM][NOFF] (the group's offsets only) | s_row[3][TM]
// ------------------------------------------------------------------------------------------------------------
template <int MT, int NT, int KB, int PH, bool BF>
__global__ __launch_bounds__(256) void conv_wgrad_rows_p(const float* __restrict__ feat, const float* __restrict__ dout,
                                                         const int32_t* __restrict__ nbr, const int32_t* __restrict__ order, int n_out, int K,
                                                         int Cin, int Cout, float* __restrict__ part, int swap) {
  constexpr int TPP = KB * MT * NT / 4;
  static_assert(KB * MT * NT % 4 == 0, "phase tiles must split evenly over the 4 waves");
  static_assert(4 % NT == 0, "a wave's tiles must share one column block");
  constexpr int LDA = ldb_of(MT);
  constexpr int NOFF = PH * KB;
  constexpr int NV = (TM * NOFF + 255) / 256;   // map entries per thread and tile
  constexpr int NS = TM / 4;                    // 4-row MFMA steps per tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* As = (float*)smem;                              // [2][KB][TM][LDA]
  int32_t* s_nbr = (int32_t*)(As + 2 * KB * TM * LDA);   // [3][TM][NOFF]
  int32_t* s_row = s_nbr + 3 * TM * NOFF;                // [3][TM]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4;
  const int kg0 = blockIdx.y * NOFF;
  const int nt_wg = wg_tiles_of_workgroup((n_out + TM - 1) / TM);
  const int bcol = (wave % NT) * 16 + (lane & 15);   // this lane's column of the contiguous operand

  f32x4 acc[PH * TPP];
#pragma unroll
  for (int t = 0; t < PH * TPP; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  int nv[NV], nrow = -1;            // the map rows (this group's offsets) and row ids of a tile, in flight
  float4 gv[KB * MT];               // the gathered rows of an item, in flight
  float bcur[NS], bnext[NS];        // B fragments of the tile / of the next tile (in flight)

  auto load_map = [&](int i) { wg_load_map<TM, NOFF>(nv, nrow, i, nbr, order, n_out, K, kg0); };   // tile i of this workgroup -> registers
  auto store_map = [&](int i) { wg_store_map<TM, NOFF, 3, 3>(nv, nrow, i, s_nbr, s_row); };
  auto load_b = [&](int i) {        // B fragments of tile i (its row ids are in LDS): row 4 s + kq, column bcol
    const int32_t* rows = s_row + (i % 3) * TM + kq;
#pragma unroll
    for (int s2 = 0; s2 < NS; ++s2) {
      const int gr = rows[s2 * 4];
      bnext[s2] = (gr >= 0 && bcol < Cout) ? btc_ld1<BF>(dout, (size_t)gr * Cout + bcol) : 0.f;
    }
  };
  // bf16 activations (the launcher guarantees Cin % 8 == 0 for these instances): 16-byte loads of 8 channels -- half the load
  // instructions of the 4-channel walk and half its staging registers (216 -> 152 VGPRs for the 64 x 64 shape: a third workgroup
  // per CU) -- widened to fp32 on the way into LDS
  constexpr int UPR8 = MT * 2;                             // 8-channel units per gathered row
  constexpr int NU8 = BF ? (KB * TM * UPR8 + 255) / 256 : 1;   // units per thread and item
  uint4 gq[NU8];
  constexpr bool wide = BF;
  auto load_g = [&](int i, int p) { // the gathered rows of phase p of tile i
    const int32_t* mp = s_nbr + (i % 3) * TM * NOFF + p * KB;
    if (wide) {
#pragma unroll
      for (int u = 0; u < NU8; ++u) {
        const int e = u * 256 + tid, c8 = e % UPR8, r = (e / UPR8) % TM, kb = e / (UPR8 * TM);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (e < KB * TM * UPR8) {
          const int j = mp[r * NOFF + kb];
          if (j >= 0 && c8 * 8 < Cin) v = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(feat) + (size_t)j * Cin + c8 * 8);
        }
        gq[u] = v;
      }
      return;
    }
    wg_stage_load<BF, MT * 4>(gv, feat, tid, [&](unsigned ra) { return mp[(ra % TM) * NOFF + ra / TM]; }, Cin, 0);   // As row kb * TM + r
  };
  auto store_g = [&](int buf) {
    float* A = As + buf * KB * TM * LDA;
    if (wide) {
#pragma unroll
      for (int u = 0; u < NU8; ++u) {
        const int e = u * 256 + tid, c8 = e % UPR8, r = (e / UPR8) % TM, kb = e / (UPR8 * TM);
        if (e < KB * TM * UPR8) {
          float* d = A + (kb * TM + r) * LDA + c8 * 8;
          const unsigned w[4] = {gq[u].x, gq[u].y, gq[u].z, gq[u].w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            d[2 * q] = __uint_as_float(w[q] << 16);
            d[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u);
          }
        }
      }
      return;
    }
    wg_stage_store<MT * 4>(gv, A, LDA, tid);
  };

  if (nt_wg > 0) {
    load_map(0);
    store_map(0);
    if (nt_wg > 1) {
      load_map(1);
      store_map(1);
    }
    __syncthreads();
    load_b(0);
    load_g(0, 0);
  }
  int buf = 0;
  for (int i = 0; i < nt_wg; ++i) {
#pragma unroll
    for (int p = 0; p < PH; ++p) {
      store_g(buf);
      if (p == 0) {
#pragma unroll
        for (int s2 = 0; s2 < NS; ++s2) bcur[s2] = bnext[s2];
      }
      // the map rows that were loaded during the previous item: tile i + 2 (PH > 1: loaded at this tile's phase 0) or
      // tile i + 1 (PH == 1: loaded during tile i - 1); tiles 0 and 1 come from the prologue
      if (PH > 1 ? (p == 1 && i + 2 < nt_wg) : (i >= 1 && i + 1 < nt_wg)) store_map(PH > 1 ? i + 2 : i + 1);
      __syncthreads();
      // ---- loads for the next item, in flight during this item's MFMAs
      if (p + 1 < PH) {
        load_g(i, p + 1);
      } else if (i + 1 < nt_wg) {
        load_b(i + 1);
        load_g(i + 1, 0);
      }
      if (PH > 1 ? (p == 0 && i + 2 < nt_wg) : (i + 2 < nt_wg)) load_map(i + 2);
      // ---- MFMAs of item (i, p)
      const float* A = As + buf * KB * TM * LDA;
#pragma unroll
      for (int q = 0; q < TPP; ++q) {
        const WgTile t = wg_tile<MT, NT>(q, wave);  // phase-local tile: (kb, mt, nt), nt == wave % NT
        const float* ap = A + (size_t)t.kb * TM * LDA + t.mt * 16 + (lane & 15) + kq * LDA;
        f32x4 a4 = acc[p * TPP + q];
#pragma unroll
        for (int s2 = 0; s2 < NS; ++s2) a4 = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[s2 * 4 * LDA], bcur[s2], a4, 0, 0, 0);
        acc[p * TPP + q] = a4;
      }
      buf ^= 1;
    }
  }
  wg_store_slab_rows<MT, NT, KB, PH>(part + (size_t)blockIdx.x * K * Cin * Cout, K, Cin, Cout, kg0, swap,
                                     [&](int p, int q, int r) { return acc[p * TPP + q][r]; });
}

// sum_s part[s][e] in slab order (deterministic): a chain of S dependent additions per element, bound by the round trips of its loads --
// 16 in flight, then 8, then single terms; the order of the additions is the slab order either way
__device__ __forceinline__ float wgrad_slab_sum(const float* __restrict__ part, int S, long long count, long long e) {
  float s = 0.f;
  int q = 0;
  for (; q + 16 <= S; q += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = part[(size_t)(q + u) * count + e];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += v[u];
  }
  for (; q + 8 <= S; q += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(q + u) * count + e];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; q < S; ++q) s += part[(size_t)q * count + e];
  return s;
}

// dW[e] = sum_s part[s][e]
__global__ __launch_bounds__(256) void wgrad_reduce(const float* __restrict__ part, int S, long long count,
                                                    float* __restrict__ dW) {
  long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  dW[e] = wgrad_slab_sum(part, S, count, e);
}

// the slab reductions of MANY layers in one launch (btc_wgrad_reduce_multi: every weight gradient of a backward pass whose dW nobody
// reads before the side stream's join): block b works on job j with block0[j] <= b < block0[j + 1]; same sums, same order as wgrad_reduce
struct ReduceJobs {
  const float* part[BTC_WGRAD_MULTI_MAX];
  float* dW[BTC_WGRAD_MULTI_MAX];
  long long count[BTC_WGRAD_MULTI_MAX];
  int S[BTC_WGRAD_MULTI_MAX];
  int block0[BTC_WGRAD_MULTI_MAX + 1];
  int n;
};

__global__ __launch_bounds__(256) void wgrad_reduce_multi(const ReduceJobs jobs) {
  int j = 0;
  while (j + 1 < jobs.n && (int)blockIdx.x >= jobs.block0[j + 1]) ++j;   // (uniform: scalar loop over <= 64 entries)
  const long long e = (long long)((int)blockIdx.x - jobs.block0[j]) * 256 + threadIdx.x;
  const long long count = jobs.count[j];
  if (e >= count) return;
  jobs.dW[j][e] = wgrad_slab_sum(jobs.part[j], jobs.S[j], count, e);
}

// ---- host side: one planner (wgrad_choose) decides everything about a call; btc_conv_wgrad_ws_bytes asks the same per-family plans ----

template <int MT, int NT, int KB, int PH, bool BF>
void launch_wgrad_rows_p(const WgradLaunch& L, const WgradArgs& a) {
  static BtcPerDeviceOnce once;   // launches come from the training thread, the autograd thread and the prefetch thread
  btc_once_per_device(once, [] {
    (void)hipFuncSetAttribute((const void*)conv_wgrad_rows_p<MT, NT, KB, PH, BF>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  });
  conv_wgrad_rows_p<MT, NT, KB, PH, BF><<<dim3(L.S, L.groups), 256, L.lds, a.stream>>>(a.g, a.c, a.map, a.ord, L.walk.rows, a.K, L.walk.Cg, L.walk.Cc,
                                                                                    a.part, L.walk.swap);
}

template <int MT, int NT, int KB, int PH, bool BF>
void launch_wgrad_rows(const WgradLaunch& L, const WgradArgs& a) {
  conv_wgrad_rows<MT, NT, KB, PH, BF><<<dim3(L.S, L.groups), 256, L.lds, a.stream>>>(a.g, a.c, a.map, a.ord, L.walk.rows, a.K, L.walk.Cg, L.walk.Cc, a.part,
                                                                                  L.walk.swap, btc_tune_get(BTC_TUNE_APPLY_DEBUG));
}

template <int NT, bool BF, bool PIPE>
void launch_wgrad_partial(const WgradLaunch& L, const WgradArgs& a) {
  const dim3 grid(a.K, L.S, L.blocks);
  const WgradWalk& w = L.walk;   // (the output rows: Cg = Cin, Cc = Cout)
  if (PIPE) conv_wgrad_partial_p<NT, BF><<<grid, 256, L.lds, a.stream>>>(a.g, a.c, a.map, w.rows, a.K, w.Cg, w.Cc, L.tiles_per_split, L.n_cblk, a.part);
  else conv_wgrad_partial<NT, BF><<<grid, 256, L.lds, a.stream>>>(a.g, a.c, a.map, w.rows, a.K, w.Cg, w.Cc, L.tiles_per_split, L.n_cblk, a.part);
}

// ---- the instance tables (each macro spells the template instances of one table row, nothing else) ----
// rows_p / rows: (MT, NT) 16-wide tiles of the gathered / walked channels -> KB offsets per LDS phase, PH phases per offset group
struct RowsTile {
  int mt, nt, kb;
  int n_auto;      // the work split picks among ph[0 .. n_auto); a variant after those is reached through BTC_TUNE_WGRAD_PH only
  int ph[4];       // the PH of each variant, 0: none
  WgradFn fn[2][4];   // [bf16 activations][PH variant]
};
// conv_wgrad_rows_p: variants PH = ph, ph / 2 (its own (KB, PH) per tile shape: the B fragments live in registers, LDS holds the
// double-buffered gather tile only)
#define ROWS_P_TILE(MT, NT, KB, PH)                                                                                                  \
  {MT, NT, KB, 2, {PH, PH / 2}, {{launch_wgrad_rows_p<MT, NT, KB, PH, false>, launch_wgrad_rows_p<MT, NT, KB, PH / 2, false>},      \
                                 {launch_wgrad_rows_p<MT, NT, KB, PH, true>, launch_wgrad_rows_p<MT, NT, KB, PH / 2, true>}}}
const RowsTile ROWS_P_TILES[] = {ROWS_P_TILE(1, 1, 4, 4), ROWS_P_TILE(2, 1, 2, 8), ROWS_P_TILE(1, 2, 4, 4), ROWS_P_TILE(2, 2, 2, 8),
                                 ROWS_P_TILE(3, 2, 2, 4), ROWS_P_TILE(2, 4, 2, 4), ROWS_P_TILE(4, 2, 1, 8), ROWS_P_TILE(4, 4, 1, 4)};
#undef ROWS_P_TILE
// conv_wgrad_rows: variants PH = 4, 2, 1 for the work split and PH = 7 (it no longer fits two workgroups per CU) for the key; the
// 16 -> 16 shape has the one PH named
#define ROWS_TILE(MT, NT, KB)                                                                                                                \
  {MT, NT, KB, 3, {4, 2, 1, 7},                                                                                                              \
   {{launch_wgrad_rows<MT, NT, KB, 4, false>, launch_wgrad_rows<MT, NT, KB, 2, false>, launch_wgrad_rows<MT, NT, KB, 1, false>,             \
     launch_wgrad_rows<MT, NT, KB, 7, false>},                                                                                              \
    {launch_wgrad_rows<MT, NT, KB, 4, true>, launch_wgrad_rows<MT, NT, KB, 2, true>, launch_wgrad_rows<MT, NT, KB, 1, true>,                \
     launch_wgrad_rows<MT, NT, KB, 7, true>}}}
const RowsTile ROWS_TILES[] = {{1, 1, 8, 1, {4}, {{launch_wgrad_rows<1, 1, 8, 4, false>}, {launch_wgrad_rows<1, 1, 8, 4, true>}}},
                               ROWS_TILE(2, 1, 4), ROWS_TILE(1, 2, 4), ROWS_TILE(2, 2, 4), ROWS_TILE(3, 2, 2), ROWS_TILE(2, 4, 2), ROWS_TILE(4, 2, 2),
                               ROWS_TILE(4, 4, 1)};
#undef ROWS_TILE
constexpr int N_ROWS_TILES = sizeof(ROWS_TILES) / sizeof(ROWS_TILES[0]);
static_assert(sizeof(ROWS_P_TILES) == sizeof(ROWS_TILES), "the two row-stationary kernels take the same tile shapes, in the same order");
// partial_p / partial: NT = 1, 2, 4, 8 16-column tiles of Cout per workgroup
#define PARTIAL_NT(BF, PIPE) \
  {launch_wgrad_partial<1, BF, PIPE>, launch_wgrad_partial<2, BF, PIPE>, launch_wgrad_partial<4, BF, PIPE>, launch_wgrad_partial<8, BF, PIPE>}
const WgradFn PARTIAL_FN[2][2][4] = {{PARTIAL_NT(false, false), PARTIAL_NT(false, true)}, {PARTIAL_NT(true, false), PARTIAL_NT(true, true)}};   // [bf16][pipe][log2 NT]
#undef PARTIAL_NT

// ---- the walks ----
WgradWalk wgrad_walk(const WgradCall& c, int swap, int rows) { return {swap, rows, swap ? c.Cout : c.Cin, swap ? c.Cin : c.Cout}; }

// the walk of the row-stationary families: the smaller side of the rulebook where the input side is under half the output side
WgradWalk wgrad_short_walk(const WgradCall& c) {
  const int swap = c.n_in > 0 && 2LL * c.n_in < c.n_out;
  return wgrad_walk(c, swap, swap ? c.n_in : c.n_out);
}

// an operand of `rows` rows x C elements of esz bytes that a kernel reaches through 32-bit byte offsets (4 GB)
bool wgrad_fits32(long long rows, long long C, long long esz) { return rows * C * esz < 0xFFFFFF00LL; }

// ---- per-family plans (conv_wgrad.h): false = the family does not take this shape; true = *L describes its launch ----

// row-stationary kernels: supported (MT, NT) tile shapes and enough rows to amortise the persistent walk
bool wgrad_plan_rows(bool bf, const WgradCall& c, const WgradWalk& w, WgradLaunch* L) {
  const int mt = btc_cdiv(w.Cg, 16), nt = btc_cdiv(w.Cc, 16);
  int tile = -1;
  for (int i = 0; i < N_ROWS_TILES; ++i)
    if (ROWS_TILES[i].mt == mt && ROWS_TILES[i].nt == nt) tile = i;
  if (tile < 0 || w.rows < 4096 || c.K > 64) return false;
  // software-pipelined variant (conv_wgrad_rows_p) when the gathered operand's channel count is a multiple of 4
  const bool pipe = (w.Cg & (bf ? 7 : 3)) == 0 && btc_tune_get(BTC_TUNE_WGRAD_PIPE) != 1;   // bf16: 8-channel gathers
  const RowsTile& t = pipe ? ROWS_P_TILES[tile] : ROWS_TILES[tile];
  // the PH variants the work split chooses from -- or, in tuning runs, the one variant of this tile row that BTC_TUNE_WGRAD_PH names
  const int t_ph = btc_tune_get(BTC_TUNE_WGRAD_PH);
  int v0 = 0, n_ph = t.n_auto;
  for (int i = 0; i < 4; ++i)
    if (t_ph && t.ph[i] == t_ph) v0 = i, n_ph = 1;
  const WgradSplit s = wgrad_split(btc_cdiv(w.rows, TM), c.K, t.kb, t.ph + v0, n_ph, 1);
  *L = WgradLaunch{};
  L->family = pipe ? WG_ROWS_P : WG_ROWS;
  L->S = s.S;
  L->walk = w;
  L->fn = t.fn[bf][v0 + s.i];
  // rows_p: As[2][KB][TM][LDA] | s_nbr[3][TM][KB * PH] | s_row[3][TM];  rows: As[KB][TM][LDA] | Ds[TM][LDB] | s_nbr[TM][K] | s_kact[K] | s_row[TM]
  L->lds = pipe ? (size_t)(2 * t.kb * TM * ldb_of(mt)) * sizeof(float) + (size_t)(3 * TM * t.kb * s.ph + 3 * TM) * sizeof(int32_t)
                : (size_t)(t.kb * TM * ldb_of(mt) + TM * ldb_of(nt)) * sizeof(float) + (size_t)(TM * c.K + c.K + TM) * sizeof(int32_t);
  L->groups = s.groups;
  return true;
}

// offset-major kernels: everything else, over the output rows
void wgrad_plan_partial(bool bf, const WgradCall& c, WgradLaunch* L) {
  const bool pipe = ((c.Cin | c.Cout) & 3) == 0 && btc_tune_get(BTC_TUNE_WGRAD_PIPE) != 1;
  const int lnt = c.Cout <= 16 ? 0 : (c.Cout <= 32 ? 1 : (c.Cout <= 64 ? 2 : 3)), nt = 1 << lnt;
  *L = WgradLaunch{};
  L->family = pipe ? WG_PARTIAL_P : WG_PARTIAL;
  L->walk = wgrad_walk(c, 0, c.n_out);
  L->fn = PARTIAL_FN[bf][pipe][lnt];
  L->lds = (size_t)(TM * WG_LDA + TM * ldb_of(nt)) * sizeof(float) + (4 * TM + 2) * sizeof(int32_t);
  L->n_cblk = btc_cdiv(c.Cout, nt * 16);
  L->blocks = btc_cdiv(c.Cin, 64) * L->n_cblk;
  const int n_tiles = btc_cdiv(c.n_out > 0 ? c.n_out : 1, TM);
  int S = 1536 / (c.K * L->blocks);
  if (S > 32) S = 32;
  if (S < 1) S = 1;
  if (S > n_tiles) S = n_tiles;
  L->tiles_per_split = btc_cdiv(n_tiles, S);
  L->S = btc_cdiv(n_tiles, L->tiles_per_split);
}

// the most slabs any launch of this call can write: every family that takes the shape, for both activation types and both walk sides --
// whatever BTC_TUNE_WGRAD_X, _NARROW and BTC_TUNE_SPLIT say and whatever the 4 GB bounds allow, so that a switch flipped between sizing and
// launch cannot leave the buffer short (the keys that shape a split, _WGS, _PH, _PIPE, enter here as they enter the launch)
int wgrad_max_slabs(const WgradCall& c) {
  const WgradWalk out = wgrad_walk(c, 0, c.n_out), w = wgrad_short_walk(c);
  WgradLaunch L = {};
  int S = 1;
  for (int bf = 0; bf < 2; ++bf) {
    // (the bf16 instances of the pipelined kernel want 8-channel gathers, so the two plans can differ)
    if (!wgrad_plan_rows(bf, c, w, &L)) wgrad_plan_partial(bf, c, &L);
    if (L.S > S) S = L.S;
    if (btc_wgrad_x_plan(bf, c.K, out, &L) && L.S > S) S = L.S;
    if (w.swap && btc_wgrad_x_plan(bf, c.K, w, &L) && L.S > S) S = L.S;
  }
  // narrow layers: either walk side at either row count (kind 1 walks n_out rows where the map is mirrored)
  for (int swap = 0; swap < 2; ++swap) {
    if (btc_wgrad_n_plan(c, wgrad_walk(c, swap, c.n_out), false, &L) && L.S > S) S = L.S;
    if (c.n_in > 0 && btc_wgrad_n_plan(c, wgrad_walk(c, swap, c.n_in), false, &L) && L.S > S) S = L.S;
  }
  return S;
}

// the launch of one call: the first family, in this order, that takes the shape and that the tuning keys and the 4 GB bounds allow
WgradLaunch wgrad_choose(bool bf, const WgradCall& c) {
  WgradLaunch L = {};
  // the n and x families gather through 32-bit byte offsets: both operands under 4 GB, so the row count of `feat` must be known
  const long long esz = bf ? 2 : 4;
  const bool fits = c.n_feat >= 0 && wgrad_fits32(c.n_feat, c.Cin, esz) && wgrad_fits32(c.n_out, c.Cout, esz);
  if (btc_tune_get(BTC_TUNE_WGRAD_NARROW) != 1) {
    // (n reaches its map through 32-bit offsets as well)
    const WgradWalk in = wgrad_walk(c, 1, c.mirror ? c.n_out : c.n_in), out = wgrad_walk(c, 0, c.n_out);
    if ((c.mirror || c.n_in >= 0) && in.rows >= 2048 && fits && wgrad_fits32(in.rows, c.K, 4) && btc_wgrad_n_plan(c, in, bf, &L)) return L;
    // (not where the rulebook's input side is less than half the output side: the kernels below walk that side -- 4 -> 16 from 8.4 K to
    // 40 K rows: 13.6 us there, 23.8 here)
    if (!(c.n_in >= 0 && 2LL * c.n_in < c.n_out) && out.rows >= 2048 && fits && wgrad_fits32(out.rows, c.K, 4) && btc_wgrad_n_plan(c, out, bf, &L)) return L;
  }
  const WgradWalk w = wgrad_short_walk(c);
  if (btc_tune_get(BTC_TUNE_WGRAD_X) != 1 && (bf || btc_tune_get(BTC_TUNE_SPLIT) != 1) && fits && btc_wgrad_x_plan(bf, c.K, w, &L)) return L;
  if (!wgrad_plan_rows(bf, c, w, &L)) wgrad_plan_partial(bf, c, &L);
  return L;
}

// every family ends the same way: the check of its launch, then the slabs
int wgrad_finish(const float* part, int S, long long count, float* dW, int* slabs_out, hipStream_t stream) {
  BTC_LAUNCH_CHECK();
  if (slabs_out) {
    *slabs_out = S;
    return BTC_OK;
  }
  wgrad_reduce<<<btc_cdiv(count, 256), 256, 0, stream>>>(part, S, count, dW);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}

int wgrad_impl(bool bf, const void* feat_, const void* dout_, const int32_t* nbr_out, int n_out, const int32_t* nbr_in, int n_in, int K, int Cin, int Cout,
               float* dW, void* ws, size_t ws_bytes, void* stream_, const int32_t* order_out = nullptr, const int32_t* order_in = nullptr,
               int* slabs_out = nullptr) {
  // slabs_out: the caller adds the slabs up itself, later (btc_wgrad_reduce_multi): *slabs_out = S > 0 slabs of K Cin Cout floats
  // in `ws`, dW untouched -- or 0: dW is complete (no rows: zeros)
  hipStream_t stream = (hipStream_t)stream_;
  const float *feat = (const float*)feat_, *dout = (const float*)dout_;
  BTC_CHECK_ARG(K >= 1 && Cin >= 1 && Cout >= 1 && n_out >= 0, "btc_conv_wgrad: bad sizes");
  BTC_CHECK_ARG(K <= BTC_CONV_K_MAX, "btc_conv_wgrad: K=%d offsets, more than BTC_CONV_K_MAX = %d", K, BTC_CONV_K_MAX);
  // rows of `feat`: n_in when the backward map comes with it, or when a caller without one states a positive count; a legacy call that
  // passes NULL and 0 (the argument used to be ignored without a map) leaves it unknown -> the fp32-pipe kernels, which need no bound
  // nbr_in == nbr_out (the same pointer, n_in == n_out): a submanifold layer -- its backward map is the forward map with the offset index
  // mirrored, nothing else is stored (rulebook.hip); the kernels that walk the output rows take it as "no backward map"
  WgradCall c = {n_out, K, Cin, Cout, n_in, n_in, nbr_in != nullptr && nbr_in == nbr_out && n_in == n_out};
  const bool have_bwd = nbr_in != nullptr && !c.mirror;
  if (!have_bwd && n_in <= 0) c.n_feat = -1;
  if (!have_bwd) c.n_in = -1;
  BTC_CHECK_ARG(ws_bytes >= btc_conv_wgrad_ws_bytes(n_out, K, Cin, Cout, c.n_in), "btc_conv_wgrad: workspace too small");
  const long long count = (long long)K * Cin * Cout;
  if (slabs_out) *slabs_out = 0;
  if (n_out <= 0) {
    BTC_HIP(hipMemsetAsync(dW, 0, (size_t)count * sizeof(float), stream));
    return BTC_OK;
  }
  const WgradLaunch L = wgrad_choose(bf, c);
  BTC_CHECK_ARG((size_t)L.S * count * sizeof(float) <= ws_bytes, "btc_conv_wgrad: the chosen kernel (family %d) writes %d slabs, more than the workspace holds",
                (int)L.family, L.S);
  const int swap = L.walk.swap;
  const WgradArgs a = {swap ? dout : feat, swap ? feat : dout, swap && !c.mirror ? nbr_in : nbr_out, swap ? order_in : order_out, K, (float*)ws, stream};
  L.fn(L, a);
  return wgrad_finish(a.part, L.S, count, dW, slabs_out, stream);
}

}  // namespace

extern "C" size_t btc_conv_wgrad_ws_bytes(int n_out, int K, int Cin, int Cout, int n_in) {
  const WgradCall c = {n_out, K, Cin, Cout, n_in, n_in, false};
  return btc_align((size_t)wgrad_max_slabs(c) * K * Cin * Cout * sizeof(float));
}

extern "C" int btc_conv_wgrad(const float* feat, const float* dout, const int32_t* nbr_out, int n_out, const int32_t* nbr_in,
                              int n_in, int K, int Cin, int Cout, float* dW, void* ws, size_t ws_bytes, void* stream) {
  return wgrad_impl(false, feat, dout, nbr_out, n_out, nbr_in, n_in, K, Cin, Cout, dW, ws, ws_bytes, stream);
}

extern "C" int btc_conv_wgrad_bf16(const void* feat, const void* dout, const int32_t* nbr_out, int n_out, const int32_t* nbr_in,
                                   int n_in, int K, int Cin, int Cout, float* dW, void* ws, size_t ws_bytes, void* stream) {
  return wgrad_impl(true, feat, dout, nbr_out, n_out, nbr_in, n_in, K, Cin, Cout, dW, ws, ws_bytes, stream);
}

extern "C" int btc_conv_wgrad_ordered(int bf16_act, const void* feat, const void* dout, const int32_t* nbr_out, int n_out, const int32_t* nbr_in,
                                      int n_in, const int32_t* order_out, const int32_t* order_in, int K, int Cin, int Cout, float* dW, void* ws,
                                      size_t ws_bytes, void* stream) {
  return wgrad_impl(bf16_act != 0, feat, dout, nbr_out, n_out, nbr_in, n_in, K, Cin, Cout, dW, ws, ws_bytes, stream, order_out, order_in);
}

extern "C" int btc_conv_wgrad_slabs(int bf16_act, const void* feat, const void* dout, const int32_t* nbr_out, int n_out, const int32_t* nbr_in,
                                    int n_in, const int32_t* order_out, const int32_t* order_in, int K, int Cin, int Cout, float* dW, void* ws,
                                    size_t ws_bytes, int* n_slabs, void* stream) {
  BTC_CHECK_ARG(n_slabs != nullptr, "btc_conv_wgrad_slabs: n_slabs is NULL");
  return wgrad_impl(bf16_act != 0, feat, dout, nbr_out, n_out, nbr_in, n_in, K, Cin, Cout, dW, ws, ws_bytes, stream, order_out, order_in, n_slabs);
}

extern "C" int btc_wgrad_reduce_multi(const float* const* parts, float* const* dWs, const int* n_slabs, const long long* counts, int n_jobs,
                                      void* stream) {
  BTC_CHECK_ARG(n_jobs >= 0 && (n_jobs == 0 || (parts && dWs && n_slabs && counts)), "btc_wgrad_reduce_multi: bad arguments");
  for (int base = 0; base < n_jobs; base += BTC_WGRAD_MULTI_MAX) {
    ReduceJobs jobs;
    jobs.n = n_jobs - base < BTC_WGRAD_MULTI_MAX ? n_jobs - base : BTC_WGRAD_MULTI_MAX;
    long long blocks = 0;
    for (int j = 0; j < jobs.n; ++j) {
      BTC_CHECK_ARG(n_slabs[base + j] >= 1 && counts[base + j] >= 1 && parts[base + j] && dWs[base + j], "btc_wgrad_reduce_multi: bad job %d", base + j);
      jobs.part[j] = parts[base + j];
      jobs.dW[j] = dWs[base + j];
      jobs.S[j] = n_slabs[base + j];
      jobs.count[j] = counts[base + j];
      jobs.block0[j] = (int)blocks;
      blocks += (counts[base + j] + 255) / 256;
    }
    jobs.block0[jobs.n] = (int)blocks;
    BTC_CHECK_ARG(blocks < (1LL << 31), "btc_wgrad_reduce_multi: too many elements");
    wgrad_reduce_multi<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(jobs);
    BTC_LAUNCH_CHECK();
  }
  return BTC_OK;
}
