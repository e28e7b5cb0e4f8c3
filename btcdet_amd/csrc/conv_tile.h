// What the sparse-conv apply kernels share below the dispatcher (sparse_conv.hip btc_apply): the flags word, the map tile a workgroup
// keeps in LDS and the prologue that fills it (conv_apply_g / conv_apply_b / conv_apply_s), the epilogue of a wave's 16-row x NTW x
// 16-column tile (conv_apply_g / conv_apply_b / conv_apply), the LDS-DMA helpers, the exact three-piece bf16 split (also conv_wgrad_x.hip)
// and the launch with a raised dynamic-LDS limit.  A kernel shares a part only where every instance keeps its register allocation,
// scratch and occupancy (profiles/apply_tile_resource_usage.txt): conv_apply_s and conv_apply_ws keep their own epilogues for that reason.
// The bar is "unchanged", in both directions: in those two families the shared epilogue allocated FEWER registers (conv_apply_ws<2, ...> 3
// VGPRs, one conv_apply_s instance 12 AGPRs) at the same occupancy, and a different allocation is a different schedule that nobody has timed.
#pragma once
#include <type_traits>

#include "btc_common.h"
#include "bn_fuse.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- the flags word of conv_apply_g / conv_apply_b / conv_apply_s
constexpr int APPLY_XCD = 1;             // workgroups are dealt round-robin to the 8 XCDs: give XCD x the contiguous tile range x
constexpr int APPLY_MIRROR = 2;          // the map is a submanifold layer's FORWARD map read as its backward map -- column K-1-k of nbr is
                                         // offset k of the transposed map (rulebook.hip: the two are mirror images, nbr_in is never materialised)
constexpr int APPLY_STAGES_SHIFT = 4;    // bits 4..7: ring depth (conv_apply_g; 0 = its default)
constexpr int APPLY_DEBUG_SHIFT = 8;     // bits 8..: timing experiments (BTC_TUNE_APPLY_DEBUG, wrong results; conv_apply_s)
inline int apply_flags(int mirror) { return (btc_tune_get(BTC_TUNE_APPLY_XCD) == 2 ? APPLY_XCD : 0) | (mirror ? APPLY_MIRROR : 0); }

// ---- the map tile, behind a kernel's ring: [TM][K] nbr | [K] kact | [1] nact | [TM] row, int32 each
//   s_nbr  [TM][K] the tile's rows of the neighbour map
//   s_kact [K]     flags, then the compact ascending list of the tile's active offsets
//   s_nact [1]     their number
//   s_row  [TM]    the row each tile slot works on (order[] or identity), -1 past the end
inline size_t apply_tail_bytes(int tm, int K) { return (size_t)(tm * K + K + 1 + tm) * sizeof(int32_t); }
// the kernel's four pointers into it, as a statement.  (A macro, and plain pointers: taken from a function or kept in a struct, conv_apply_g
// and conv_apply_s come out with 1-6 more vector registers in most instances, and some lose a wave per SIMD.)
#define APPLY_TAIL(base, TM_, K_)              \
  int32_t* s_nbr = (int32_t*)(base);           \
  int32_t* s_kact = s_nbr + (TM_) * (K_);      \
  int32_t* s_nact = s_kact + (K_);             \
  int32_t* s_row = s_nact + 1

struct ApplyTile {
  int bx, row0, n_act;            // tile index after the XCD remap, its first slot, active offsets of the workgroup
  unsigned long long wave_act;    // bit k: one of the 16 rows of this wave's row group `wr` has a neighbour at offset k (K <= 64)
};

template <int TM, int THREADS>
__device__ __forceinline__ ApplyTile apply_tile_prologue(int32_t* s_nbr, int32_t* s_kact, int32_t* s_nact, int32_t* s_row, const int32_t* __restrict__ nbr,
                                                         const int32_t* __restrict__ order, int n_rows, int K, int flags, int wr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mirror = (flags & APPLY_MIRROR) ? 1 : 0;
  int bx = blockIdx.x;
  if (flags & APPLY_XCD) {
    const int nb = gridDim.x, per = nb >> 3, main = per << 3;
    if (bx < main) bx = (bx & 7) * per + (bx >> 3);
  }
  const int row0 = bx * TM;
  for (int e = tid; e < K; e += THREADS) s_kact[e] = 0;
  for (int e = tid; e < TM; e += THREADS) s_row[e] = (row0 + e < n_rows) ? (order ? order[row0 + e] : row0 + e) : -1;
  __syncthreads();
  for (int e = tid; e < TM * K; e += THREADS) {
    const int rloc = e / K, kk = e - rloc * K;
    const int gr = s_row[rloc];
    const int v = gr >= 0 ? nbr[(long long)gr * K + (mirror ? K - 1 - kk : kk)] : -1;
    s_nbr[e] = v;
    if (v >= 0) s_kact[kk] = 1;
  }
  __syncthreads();
  unsigned long long wave_act;   // lane k scans its column of the map
  {
    bool any = false;
    if (lane < K)
      for (int r = 0; r < 16; ++r) any |= s_nbr[(wr * 16 + r) * K + lane] >= 0;
    wave_act = __ballot(any);
  }
  const int kflag = (lane < K) ? s_kact[lane] : 0;
  __syncthreads();
  if (wave == 0) {
    const unsigned long long m = __ballot(kflag != 0);
    if (kflag) s_kact[__popcll(m & ((1ull << lane) - 1ull))] = lane;
    if (lane == 0) *s_nact = __popcll(m);
  }
  __syncthreads();
  return {bx, row0, *s_nact, wave_act};
}

// ---- epilogue of a wave's 16 x (NTW x 16) tile.  C/D layout of a 16x16 MFMA: col = lane & 15, row = (lane >> 4) * 4 + reg.
// sum: the accumulated tile; rows[r]: the result row of register r, < 0 = none; col0: the first column of the wave's tile.
// v = sum + bias -> (OUT 16-bit: rounded to bf16 as stored) -> ev: the eval-mode BatchNorm (+ ReLU) of bn_fuse.h's second mode, of x as it
// would have been stored: y -> store.  vals / valid: the tensor as STORED, for bn_fuse_wave.  COLS: columns >= Cres exist (no store).
template <int NTW, bool COLS = false, typename OUT>
__device__ __forceinline__ void apply_tile_epilogue(const f32x4 (&sum)[NTW], const int (&rows)[4], int col0, const float* __restrict__ bias, int Cres,
                                                    OUT* __restrict__ out, const BnFuse& bn, bool ev, float (&vals)[NTW][4], bool (&valid)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) valid[r] = rows[r] >= 0;
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) {
    const int col = col0 + nt * 16 + (threadIdx.x & 15);
    const float bv0 = (bias && (!COLS || col < Cres)) ? bias[col] : 0.f;
    BnEvalCol ec = {0.f, 0.f, 1.f, 0.f};
    if (ev) ec = bn_eval_col(bn, col);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = bias ? (sum[nt][r] + bv0) : sum[nt][r];
      if (sizeof(OUT) == 2) {
        unsigned short h = btc_f32_to_bf16(v);
        if (ev) h = btc_f32_to_bf16(bn_affine(btc_bf16_to_f32(h), ec.m, ec.rs, ec.g, ec.b, bn.ev_relu));
        if (rows[r] >= 0) ((unsigned short*)out)[(size_t)rows[r] * Cres + col] = h;
        v = btc_bf16_to_f32(h);
      } else {
        if (ev) v = bn_affine(v, ec.m, ec.rs, ec.g, ec.b, bn.ev_relu);
        if ((!COLS || col < Cres) && rows[r] >= 0) ((float*)out)[(size_t)rows[r] * Cres + col] = v;
      }
      vals[nt][r] = v;
    }
  }
}

// ---- LDS-DMA: 16 bytes per lane from global memory to wave-uniform base + lane * 16 in LDS, and the counted wait on its queue
__device__ __forceinline__ void glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- x = hi + mid + lo, three bfloat16 pieces by truncation (8 + 8 + 8 significant bits): the split is EXACT, both subtractions are.
// Each piece is the high half of its word.
__device__ __forceinline__ float btc_split_rest(float x) { return x - __uint_as_float(__float_as_uint(x) & 0xFFFF0000u); }   // x - its piece
struct BtcSplit3 { unsigned hi, mid, lo; };
__device__ __forceinline__ BtcSplit3 btc_split3(float x) {
  const float x1 = btc_split_rest(x), x2 = btc_split_rest(x1);
  return {__float_as_uint(x), __float_as_uint(x1), __float_as_uint(x2)};
}
// two values -> one dword of each plane (low half = a's piece, high half = b's piece)
__device__ __forceinline__ void btc_split3(float a, float b, unsigned& hi, unsigned& mid, unsigned& lo) {
  hi = __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
  const float a1 = btc_split_rest(a), b1 = btc_split_rest(b);
  mid = __builtin_amdgcn_perm(__float_as_uint(b1), __float_as_uint(a1), 0x07060302u);
  const float a2 = btc_split_rest(a1), b2 = btc_split_rest(b1);
  lo = __builtin_amdgcn_perm(__float_as_uint(b2), __float_as_uint(a2), 0x07060302u);
}

// ---- launch with up to the whole 160 KB of a CU's LDS: the limit of KERNEL is raised once per device (btc_once_per_device; launches
// come from the training thread, the autograd thread and the prefetch thread), a tile that cannot fit is refused
constexpr size_t APPLY_LDS_MAX = 160 * 1024;
template <auto KERNEL, class... A>
int apply_launch(const char* who, dim3 grid, int threads, size_t lds, hipStream_t stream, A... args) {
  BTC_CHECK_ARG(lds <= APPLY_LDS_MAX, "%s: tile does not fit the LDS", who);
  static BtcPerDeviceOnce once;
  btc_once_per_device(once, [] { (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)APPLY_LDS_MAX); });
  hipLaunchKernelGGL(KERNEL, grid, dim3(threads), lds, stream, args...);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}
