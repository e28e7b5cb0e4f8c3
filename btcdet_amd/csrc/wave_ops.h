// Wave and workgroup reductions and scans, stated once (device only, gfx950, wave = 64; included through btc_common.h).
//
//   btc_wave_incl_scan(v)                  inclusive prefix sum over the wave's lanes (int, long long)
//   btc_wave_reduce(v, op)                 the shuffle-down tree: lane 0 holds op over the wave, the other lanes hold partial values
//   btc_wave_allreduce(v, op)              the xor butterfly: every lane holds op over the wave
//   btc_wave_sum / btc_wave_max            reduce with + / max;  btc_wave_all_sum / btc_wave_all_max / btc_wave_all_or: the butterflies
//   btc_block_excl_scan<WAVES>(v, &total)  exclusive prefix sum of int over the workgroup's threads, total in every thread
//   btc_block_sum<WAVES>(v)                sum of int over the workgroup, in every thread
//   btc_wave_excl_scan_chunks<Acc>(n, value, put)   one wave: exclusive prefix over j = 0 .. n-1, 64 at a time with a running carry
//   btc_wave_offsets_of_counts(counts, n, out)      one wave: counts -> offsets, out[n] = all
//
// Both trees combine lanes l and l + 32 first, then 16, ... 1, always as op(mine, the other lane's): lane 0 of the down tree and of the
// butterfly see the same pairs in the same order, so for float and double they give the same bits.  Which tree a site uses, and the order
// in which it combines its waves' results, is part of that site's result and stays there (glue.hip, det_post.hip, occ_metrics.hip, ...);
// only integer sums cross the waves in here.  An `op` that treats NaN in a way of its own (det_post.hip: fmaxf) is passed by its site.
//
// The two workgroup helpers own their LDS words, are called by EVERY thread of a workgroup of WAVES * 64 threads, and hold two
// barriers: one in front of the store of the wave totals (the readers of the call before have left: back-to-back calls are safe) and
// one behind it.  Nothing is required of the caller's own LDS.
//
// Left where they are, on purpose:
//   reductions that carry a payload (pointnet2.hip FpsBest, roi_targets.hip's masked max, template_match.hip TselBest);
//   partial ladders that stop early or start late (anchor_loss.hip and occ_loss.hip: o >= 4; bn_fuse.h and conv_apply_split.hip: 16, 32);
//   __ballot / __popcll ranking (compact.h, conv_tile.h, row_order.hip);
//   the exactness helpers of roi_targets.hip.
// The shuffles are shuffles: nothing here is a DPP or a performance change.
#pragma once
#include <hip/hip_runtime.h>

struct BtcSum {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct BtcMax {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return max(a, b); }
};
struct BtcOr {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a | b; }
};

template <class T>
__device__ __forceinline__ T btc_wave_incl_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

template <class T, class Op>
__device__ __forceinline__ T btc_wave_reduce(T v, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_down(v, o, 64));
  return v;
}
template <class T, class Op>
__device__ __forceinline__ T btc_wave_allreduce(T v, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  return v;
}
template <class T>
__device__ __forceinline__ T btc_wave_sum(T v) { return btc_wave_reduce(v, BtcSum()); }
template <class T>
__device__ __forceinline__ T btc_wave_max(T v) { return btc_wave_reduce(v, BtcMax()); }
template <class T>
__device__ __forceinline__ T btc_wave_all_sum(T v) { return btc_wave_allreduce(v, BtcSum()); }
template <class T>
__device__ __forceinline__ T btc_wave_all_max(T v) { return btc_wave_allreduce(v, BtcMax()); }
template <class T>
__device__ __forceinline__ T btc_wave_all_or(T v) { return btc_wave_allreduce(v, BtcOr()); }

template <int WAVES>
__device__ __forceinline__ int btc_block_excl_scan(int v, int* total) {
  __shared__ int s_wave[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int inc = btc_wave_incl_scan(v);
  __syncthreads();   // the call before has read s_wave
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll 4   // (not 16: at 1024 threads sixteen totals in flight cost the callers in pass_occ.hip 10 VGPRs and up to 50 SGPRs)
  for (int w = 0; w < WAVES; ++w) {
    const int t = s_wave[w];
    if (w < wave) base += t;
    sum += t;
  }
  *total = sum;
  return base + inc - v;
}

template <int WAVES>
__device__ __forceinline__ int btc_block_sum(int v) {
  __shared__ int s_wave[WAVES];
  v = btc_wave_sum(v);
  __syncthreads();   // the call before has read s_wave
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  int sum = 0;
#pragma unroll 4
  for (int w = 0; w < WAVES; ++w) sum += s_wave[w];
  return sum;
}

// value(j) -> the addend of j, put(j, prefix) stores the sum of the addends in front of j; -> the sum of all, in every lane
template <class Acc, class Value, class Put>
__device__ __forceinline__ Acc btc_wave_excl_scan_chunks(int n, Value value, Put put) {
  const int lane = threadIdx.x & 63;
  Acc run = 0;
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    const Acc v = j < n ? (Acc)value(j) : (Acc)0;
    const Acc inc = btc_wave_incl_scan(v);
    if (j < n) put(j, run + inc - v);
    run += __shfl(inc, 63, 64);
  }
  return run;
}

// out[j] = sum of max(counts[i], 0) over i < j, for j = 0 .. n
__device__ __forceinline__ void btc_wave_offsets_of_counts(const int32_t* __restrict__ counts, int n, int32_t* __restrict__ out) {
  const int total = btc_wave_excl_scan_chunks<int>(n, [=](int j) { return max(counts[j], 0); }, [=](int j, int prefix) { out[j] = prefix; });
  if ((threadIdx.x & 63) == 0) out[n] = total;
}
