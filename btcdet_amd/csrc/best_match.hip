// Best-match templates placed into the boxes of a resident batch for gfx950 (include/btcdet_hip_bestmatch.h: btc_place_templates).
//
// The host plan (btcdet_amd/device_augmentor.py) names, per box, a template's rows in the resident bank and the box's rotation and
// centre; the prefix of the row counts is made on the host too, so every output row's position is known before the launch:
//
//   bm_place_rows  one thread per output row, 256 per workgroup.  The workgroup finds the placements its rows span (two searches of
//                  bm_row_offsets, the same in every thread) and stages up to 64 of them in LDS: row range, bank range, scene (one
//                  search of bm_offsets per placement), rotation and centre.  A row finds its placement among the staged ones (a
//                  workgroup spans more only through runs of empty or tiny templates: those rows search the global arrays), reads
//                  its 12 bytes of the bank, is rotated and moved with unfused float32 arithmetic in np.einsum's order, runs its
//                  scene's op program in registers (aug_ops.h, shared with augment.hip) and is stored once.
//
// A stream: 12 B read and 12 or 16 B written per row.  No workspace, no atomics, no memset.
#include "aug_ops.h"

#include "../../include/btcdet_hip_bestmatch.h"

namespace {

constexpr int BM_T = 256;
constexpr int BM_STAGE = 64;

template <bool VEC4>
__global__ __launch_bounds__(BM_T) void bm_place_rows(const float* __restrict__ bank, long long bank_rows, const int32_t* __restrict__ bm_first,
                                                      const int32_t* __restrict__ bm_rows, const float* __restrict__ bm_place,
                                                      const int32_t* __restrict__ bm_offsets, const int32_t* __restrict__ bm_row_offsets,
                                                      int n_placements, int batch, const float* __restrict__ ops,
                                                      const int32_t* __restrict__ op_offsets, int n_out, int out_ld, float* __restrict__ out) {
  __shared__ int32_t s_start[BM_STAGE], s_end[BM_STAGE], s_first[BM_STAGE], s_rows[BM_STAGE], s_scene[BM_STAGE];
  __shared__ float s_place[BM_STAGE * 6];
  const long long row0 = (long long)blockIdx.x * BM_T;   // n_out may end within 256 rows of 2^31
  int p_lo = 0, staged = 0;
  if (n_placements > 0) {   // uniform in the workgroup
    const int last = (int)min(row0 + BM_T, (long long)n_out) - 1;
    p_lo = aug_owner(bm_row_offsets, n_placements, (int)row0);
    staged = min(aug_owner(bm_row_offsets, n_placements, last) - p_lo + 1, BM_STAGE);
    for (int k = threadIdx.x; k < staged; k += BM_T) {
      const int p = p_lo + k;
      s_start[k] = bm_row_offsets[p], s_end[k] = bm_row_offsets[p + 1];
      s_first[k] = bm_first[p], s_rows[k] = bm_rows[p];
      s_scene[k] = aug_owner(bm_offsets, batch, p);
#pragma unroll
      for (int q = 0; q < 6; ++q) s_place[k * 6 + q] = bm_place[(size_t)p * 8 + q];
    }
  }
  __syncthreads();
  if (row0 + threadIdx.x >= n_out) return;
  const int i = (int)(row0 + threadIdx.x);
  int scene = 0;
  float x = 0.f, y = 0.f, z = 0.f;
  if (staged > 0) {
    const int k = aug_owner(s_start, staged, i);
    int start = s_start[k], first = s_first[k], rows = s_rows[k];
    const float* pl = s_place + k * 6;
    float place[6];
    scene = s_scene[k];
    if (k == staged - 1 && i >= s_end[k]) {   // past the staged placements
      const int p = aug_owner(bm_row_offsets, n_placements, i);
      start = bm_row_offsets[p], first = bm_first[p], rows = bm_rows[p];
      scene = aug_owner(bm_offsets, batch, p);
#pragma unroll
      for (int q = 0; q < 6; ++q) place[q] = bm_place[(size_t)p * 8 + q];
    } else {
#pragma unroll
      for (int q = 0; q < 6; ++q) place[q] = pl[q];
    }
    const long long t = (long long)i - start;
    const long long src = (long long)first + t;
    if (t >= 0 && t < rows && first >= 0 && src < bank_rows) {
      const float* r = bank + (size_t)src * 3;
      const float tx = r[0], ty = r[1], tz = r[2];
      const float c = place[0], ms = place[1], s = place[2];
      x = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(0.f, __fmul_rn(tx, c)), __fmul_rn(ty, ms)), __fmul_rn(tz, 0.f)), place[3]);
      y = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(0.f, __fmul_rn(tx, s)), __fmul_rn(ty, c)), __fmul_rn(tz, 0.f)), place[4]);
      z = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(0.f, __fmul_rn(tx, 0.f)), __fmul_rn(ty, 0.f)), __fmul_rn(tz, 1.f)), place[5]);
      float px, py, pz;
      aug_run_ops<true>(ops, op_offsets, scene, false, x, y, z, px, py, pz);
    }
  }
  float* o = out + (size_t)i * out_ld;
  if (VEC4) {
    *reinterpret_cast<float4*>(o) = make_float4((float)scene, x, y, z);
  } else if (out_ld == 4) {
    o[0] = (float)scene, o[1] = x, o[2] = y, o[3] = z;
  } else {
    o[0] = x, o[1] = y, o[2] = z;
  }
}

}  // namespace

extern "C" int btc_place_templates(const float* bank, long long bank_rows, const int32_t* bm_first, const int32_t* bm_rows, const float* bm_place,
                                   const int32_t* bm_offsets, const int32_t* bm_row_offsets, int n_placements, int batch, const float* ops,
                                   const int32_t* op_offsets, long long n_out, int out_ld, float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(out_ld == 3 || out_ld == 4, "btc_place_templates: need out_ld 3 (x, y, z) or 4 (scene, x, y, z), got %d", out_ld);
  BTC_CHECK_ARG(batch >= 1, "btc_place_templates: need batch >= 1, got %d", batch);
  BTC_CHECK_ARG(n_placements >= 0 && bank_rows >= 0 && n_out >= 0, "btc_place_templates: negative count (n_placements %d, bank_rows %lld, n_out %lld)",
                n_placements, bank_rows, n_out);
  BTC_CHECK_ARG(n_out < (1ll << 31), "btc_place_templates: n_out = %lld does not fit 31 bits", n_out);
  BTC_CHECK_ARG(bm_offsets && bm_row_offsets && op_offsets, "btc_place_templates: missing pointer (bm_offsets, bm_row_offsets or op_offsets)");
  BTC_CHECK_ARG(n_placements == 0 || (bank && bm_first && bm_rows && bm_place), "btc_place_templates: missing pointer (bank or bm_*)");
  BTC_CHECK_ARG(out || n_out == 0, "btc_place_templates: missing pointer (out)");
  if (n_out == 0) return BTC_OK;
  const int nb = btc_cdiv(n_out, BM_T);
  if (out_ld == 4 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0)
    bm_place_rows<true><<<nb, BM_T, 0, stream>>>(bank, bank_rows, bm_first, bm_rows, bm_place, bm_offsets, bm_row_offsets, n_placements, batch, ops,
                                                 op_offsets, (int)n_out, out_ld, out);
  else
    bm_place_rows<false><<<nb, BM_T, 0, stream>>>(bank, bank_rows, bm_first, bm_rows, bm_place, bm_offsets, bm_row_offsets, n_placements, batch, ops,
                                                  op_offsets, (int)n_out, out_ld, out);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}
