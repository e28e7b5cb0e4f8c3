// The weight gradient's launch record: what the planner of conv_wgrad.hip (wgrad_choose / wgrad_max_slabs) decides about a call, for
// every kernel family -- the four fp32-pipe families of conv_wgrad.hip, the bf16 matrix pipe (conv_wgrad_x.hip) and the narrow layers
// (conv_wgrad_n.hip).  A family's plan function fills a WgradLaunch or refuses the shape; the launch is `L.fn(L, a)`, nothing is decided
// after the plan: the instance, its grid, its LDS bytes and the slab count S the workspace is checked against are the ones launched.
// (The device side has its counterpart in wgrad_tile.h: the staging, tile decode, slab stores, map ring and MFMA step loop the kernels share.)
#pragma once
#include "btc_common.h"

// what the caller has
struct WgradCall {
  int n_out, K, Cin, Cout;
  int n_in;      // rows of the backward map, < 0: there is none (a submanifold layer's mirrored forward map counts as none: the kernels
                 // that walk the output rows take nothing from it)
  int n_feat;    // rows of `feat`, < 0: unknown
  bool mirror;   // nbr_in == nbr_out: the backward map is the forward map with the offset index mirrored (rulebook.hip)
};

// One side of the rulebook as a row walk: the walked operand's rows are read once, in order, the other operand's rows are gathered
// through the map.  swap = 0: the OUTPUT rows (walked dout, gathered feat, nbr_out, order_out); swap = 1: the INPUT rows (walked feat,
// gathered dout, nbr_in or the mirrored nbr_out, order_in) and the slab is written transposed, so dW keeps its [K][Cin][Cout] layout.
struct WgradWalk {
  int swap, rows;
  int Cg, Cc;    // channels of the gathered / the walked (contiguous) operand
};

struct WgradArgs {   // the operands of the chosen walk
  const float *g, *c;
  const int32_t *map, *ord;
  int K;
  float* part;
  hipStream_t stream;
};

enum WgradFamily { WG_N, WG_X, WG_ROWS_P, WG_ROWS, WG_PARTIAL_P, WG_PARTIAL };

struct WgradLaunch {
  WgradFamily family;
  int S;                                                 // slabs the launch writes
  WgradWalk walk;
  void (*fn)(const WgradLaunch&, const WgradArgs&);      // the template instance; a launch error is left for the caller's check
  size_t lds;                                            // its dynamic LDS bytes
  int groups;                                            // rows_p / rows / x: offset groups
  int blocks;                                            // x / n / partial_p / partial: channel blocks
  int n_cblk, tiles_per_split;                           // partial_p / partial: blocks of Cout, row tiles per slab
  int flags;                                             // n: 1 mirrored map, 2 narrow input (slab written [k][narrow][walked])
};
typedef void (*WgradFn)(const WgradLaunch&, const WgradArgs&);

// ---- per-family plans: false = the family does not take this shape; true = *L describes its launch ----
// conv_wgrad_x.hip: the row-stationary walk on the bf16 matrix pipe (bf16 activations as they are, fp32 activations as three exact bf16
// pieces): >= 2048 rows, K <= 64, gathered channels a multiple of 16 (a workgroup owns a <= 64 x 64 block of every dW[k])
bool btc_wgrad_x_plan(bool bf, int K, const WgradWalk& w, WgradLaunch* L);
// conv_wgrad_n.hip: narrow layers on the fp32 matrix pipe.  A narrow RESULT (<= 8 channels: the 5-channel occupancy head) is walked over
// the layer's INPUT rows (w.swap = 1) -- x read once, dy gathered through the backward map (c.mirror: a submanifold layer's forward map,
// column k' = offset K-1-k'); a narrow INPUT (the 4- / 6-channel first layers) over its OUTPUT rows, the features gathered through nbr_out
bool btc_wgrad_n_plan(const WgradCall& c, const WgradWalk& w, bool bf, WgradLaunch* L);

// The work split of the row-stationary families (rows_p, rows, x): a persistent workgroup owns an offset group (PH phases of kb
// offsets), a channel block and every S-th 64-row tile.  Measured (tools/conv_bench.py, MI355X): two workgroups per CU (512 in all)
// = row splits x offset groups x blocks.  More phases per group = fewer groups re-reading the walked tile but a larger accumulator
// slab per workgroup and more slab traffic; the largest PH that still leaves >= 3 row tiles per workgroup measured best from 12 K
// to 210 K rows (e.g. 32->32 at 210 K rows 307 -> 219 us, at 12 K rows 63 -> 30 us).
//   ph[0 .. n_ph): the PH values the caller has instances for, largest first -> i = the first that leaves tiles x groups x blocks
//   >= 3 x workgroups, else the last; S = workgroups / (groups x blocks), at least two row tiles per workgroup, at least 1
struct WgradSplit {
  int i, ph, groups, S;
};
static inline WgradSplit wgrad_split(int n_tiles, int K, int kb, const int* ph, int n_ph, int blocks) {
  const int t_wgs = btc_tune_get(BTC_TUNE_WGRAD_WGS);
  const int wgs = t_wgs ? t_wgs : 512;
  int i = 0;
  while (i + 1 < n_ph && (long long)n_tiles * btc_cdiv(K, kb * ph[i]) * blocks < 3LL * wgs) ++i;
  WgradSplit s = {i, ph[i], btc_cdiv(K, kb * ph[i]), 1};
  s.S = wgs / (s.groups * blocks);
  if (s.S > n_tiles / 2) s.S = n_tiles / 2;
  if (s.S < 1) s.S = 1;
  return s;
}
