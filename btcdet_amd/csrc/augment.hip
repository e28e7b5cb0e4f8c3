// Training augmentation of a resident batch for gfx950 (include/btcdet_hip_augment.h: btc_augment_batch, btc_world_transform).
//
// The host plan (btcdet_amd/device_augmentor.py) carries everything that is O(boxes); these kernels touch the points:
//
//   aug_mark     one thread per scan row, 256 per workgroup.  The workgroup finds the scenes its rows span (two searches of
//                scene_offsets, the same in every thread), stages each such scene's removal boxes in LDS 64 at a time (no cap on
//                their number) and tests its rows against them with unfused float32 arithmetic (__fmul_rn / __fsub_rn / __fadd_rn:
//                numpy does not fuse, and a fused form moves a point that sits within an ulp of a face across it).
//                -> keep flag per row, kept count per workgroup.
//   (scan)       btc_scan_exclusive_i32 over the workgroup counts (csrc/scan.hip).
//   aug_offsets  one wave per scene boundary: kept rows and pasted rows in front of it -> out_offsets; one more wave ranks the
//                objects' row counts (exclusive prefix) for aug_emit's row -> object search.
//   aug_emit     workgroups [0, nb): the kept scan rows at their stable rank (compact.h); workgroups [nb, ..): one thread per pasted
//                row, bank[first + i] shifted in double.
//                Every emitted row runs its scene's op program and is stored to `out`, and to `out_pre` as it stood at the first ROT.
//   aug_world    the op program alone over stacked sets.
//
// All of it is a stream: a KITTI-shaped batch (2 x ~28 k rows of 16 bytes) is bound by its launches (mark, scan, offsets, emit:
// 18.5 us in all, tools/augment_bench.py), a Waymo-shaped batch (2 x ~160 k rows) by HBM: 16 B read by aug_mark, 1 + 16 B read and 16 or 32 B written by aug_emit per row.  No atomics, no memset, no ticket: every
// workspace word a kernel reads was written by an earlier launch of the same call.
#include "aug_ops.h"   // aug_in_box (shared with gt_database.hip), aug_rotate, aug_run_ops (with best_match.hip); compact.h: the compaction's stages, aug_owner

namespace {

constexpr int AUG_T = BTC_COMPACT_T;
constexpr int AUG_BOX_CHUNK = 64;
constexpr int AUG_SMALL_SET = 45;   // rotate_points_along_z: sets below 45 rows (9 n < 400) take the rounded chain

__global__ __launch_bounds__(AUG_T) void aug_mark(const float* __restrict__ pts, int n, int ld, const int32_t* __restrict__ scene_offsets,
                                                  int batch, const float* __restrict__ rm_boxes, const int32_t* __restrict__ rm_offsets,
                                                  unsigned char* __restrict__ keep_flag, int32_t* __restrict__ block_cnt) {
  __shared__ float s_box[AUG_BOX_CHUNK * 8];
  const int row0 = blockIdx.x * AUG_T;
  const int i = row0 + threadIdx.x;
  const bool live = i < n;
  float x = 0.f, y = 0.f, z = 0.f;
  int mine = -1;
  if (live) {
    const float* p = pts + (size_t)i * ld;
    x = p[0], y = p[1], z = p[2];
    mine = aug_owner(scene_offsets, batch, i);
  }
  bool removed = false;
  if (row0 < n && rm_boxes != nullptr) {
    int s_lo, s_hi;
    btc_compact_scene_span(scene_offsets, batch, row0, n, s_lo, s_hi);
    for (int s = s_lo; s <= s_hi; ++s) {
      const int b0 = rm_offsets[s], b1 = rm_offsets[s + 1];
      for (int c0 = b0; c0 < b1; c0 += AUG_BOX_CHUNK) {
        const int nbox = min(AUG_BOX_CHUNK, b1 - c0);
        __syncthreads();   // the previous chunk has been read
        for (int k = threadIdx.x; k < nbox * 8; k += AUG_T) s_box[k] = rm_boxes[(size_t)c0 * 8 + k];
        __syncthreads();
        if (mine == s && !removed) {
          for (int k = 0; k < nbox; ++k) {
            if (aug_in_box(x, y, z, s_box + k * 8)) {
              removed = true;
              break;
            }
          }
        }
      }
    }
  }
  const bool keep = live && !removed;
  if (live) keep_flag[i] = (unsigned char)keep;
  btc_compact_count(keep, block_cnt);
}

// blocks [0, batch]: boundary s -> kept_off[s] = kept scan rows in front of scene s, paste_off[s] = pasted rows in front of it,
// out_offsets[s] = their sum.  block batch + 1: obj_prefix[j] = rows of the objects in front of object j, obj_prefix[n_objects] = all.
__global__ __launch_bounds__(64) void aug_offsets(const unsigned char* __restrict__ keep_flag, int n, const int32_t* __restrict__ scene_offsets,
                                                  int batch, const int32_t* __restrict__ block_prefix, const int32_t* __restrict__ total,
                                                  const int32_t* __restrict__ obj_rows, const int32_t* __restrict__ obj_offsets, int n_objects,
                                                  int32_t* __restrict__ kept_off, int32_t* __restrict__ paste_off,
                                                  int32_t* __restrict__ obj_prefix, int32_t* __restrict__ out_offsets) {
  const int lane = threadIdx.x;
  if ((int)blockIdx.x == batch + 1) {
    btc_wave_offsets_of_counts(obj_rows, n_objects, obj_prefix);
    return;
  }
  const int s = blockIdx.x;
  const int kept = btc_compact_boundary(s, scene_offsets, batch, n, block_prefix, total, [=](int j) -> int { return keep_flag[j]; });
  int pasted = 0;
  if (n_objects > 0) {
    const int j1 = min(max(obj_offsets[s], 0), n_objects);
    for (int j = lane; j < j1; j += 64) pasted += max(obj_rows[j], 0);
    pasted = btc_wave_all_sum(pasted);
  }
  if (lane == 0) {
    kept_off[s] = kept;
    paste_off[s] = pasted;
    out_offsets[s] = kept + pasted;
  }
}

template <bool VEC4>
__device__ __forceinline__ void aug_store_row(float* __restrict__ dst, int ld, float x, float y, float z, const float* __restrict__ rest) {
  if (VEC4) {
    *reinterpret_cast<float4*>(dst) = make_float4(x, y, z, rest[0]);
  } else {
    dst[0] = x, dst[1] = y, dst[2] = z;
    for (int c = 3; c < ld; ++c) dst[c] = rest[c - 3];
  }
}

template <bool VEC4>
__global__ __launch_bounds__(AUG_T) void aug_emit(const float* __restrict__ pts, int n, int ld, const int32_t* __restrict__ scene_offsets, int batch,
                                                  const unsigned char* __restrict__ keep_flag, const int32_t* __restrict__ block_prefix, int nb,
                                                  const float* __restrict__ bank, long long bank_rows, const int32_t* __restrict__ obj_first,
                                                  const double* __restrict__ obj_shift, const int32_t* __restrict__ obj_offsets, int n_objects,
                                                  long long paste_rows, const int32_t* __restrict__ obj_prefix, const int32_t* __restrict__ kept_off,
                                                  const int32_t* __restrict__ paste_off, const float* __restrict__ ops,
                                                  const int32_t* __restrict__ op_offsets, const int32_t* __restrict__ out_offsets,
                                                  long long out_capacity, float* __restrict__ out, float* __restrict__ out_pre) {
  float x, y, z;
  float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const float* rest = nullptr;   // columns 3.. of the source row (scalar path)
  long long dst;
  int s;
  if ((int)blockIdx.x < nb) {
    const int i = blockIdx.x * AUG_T + threadIdx.x;
    const bool keep = (i < n) && keep_flag[i] != 0;
    const int rank = btc_compact_rank(keep, block_prefix);
    if (!keep) return;
    s = aug_owner(scene_offsets, batch, i);
    dst = (long long)rank + paste_off[s];
    const float* p = pts + (size_t)i * ld;
    if (VEC4) {
      v4 = *reinterpret_cast<const float4*>(p);
      x = v4.x, y = v4.y, z = v4.z;
    } else {
      x = p[0], y = p[1], z = p[2];
      rest = p + 3;
    }
  } else {
    const long long t = (long long)(blockIdx.x - nb) * AUG_T + threadIdx.x;
    if (t >= paste_rows || t >= (long long)obj_prefix[n_objects]) return;
    const int j = aug_owner(obj_prefix, n_objects, (int)t);
    s = aug_owner(obj_offsets, batch, j);
    dst = (long long)kept_off[s + 1] + t;
    const long long src = (long long)obj_first[j] + (t - obj_prefix[j]);
    const bool ok = src >= 0 && src < bank_rows && obj_first[j] >= 0;
    if (!ok) {
      x = y = z = 0.f;
    } else {
      const float* p = bank + (size_t)src * ld;
      if (VEC4) {
        v4 = *reinterpret_cast<const float4*>(p);
        x = v4.x, y = v4.y, z = v4.z;
      } else {
        x = p[0], y = p[1], z = p[2];
        rest = p + 3;
      }
      const double* sh = obj_shift + (size_t)j * 4;
      x = (float)((double)x + sh[0]);
      y = (float)((double)y + sh[1]);
      z = (float)((double)z + sh[2]);
      z = (float)((double)z - sh[3]);
    }
  }
  if (dst < 0 || dst >= out_capacity) return;
  const bool small_set = out_offsets[s + 1] - out_offsets[s] < AUG_SMALL_SET;
  float px, py, pz;
  aug_run_ops<false>(ops, op_offsets, s, small_set, x, y, z, px, py, pz);
  float* o = out + (size_t)dst * ld;
  float* op = out_pre ? out_pre + (size_t)dst * ld : nullptr;
  if (VEC4) {
    *reinterpret_cast<float4*>(o) = make_float4(x, y, z, v4.w);
    if (op) *reinterpret_cast<float4*>(op) = make_float4(px, py, pz, v4.w);
  } else if (rest != nullptr) {
    aug_store_row<false>(o, ld, x, y, z, rest);
    if (op) aug_store_row<false>(op, ld, px, py, pz, rest);
  } else {   // a zero row in place of one outside the bank
    for (int c = 0; c < ld; ++c) o[c] = 0.f;
    if (op)
      for (int c = 0; c < ld; ++c) op[c] = 0.f;
  }
}

template <bool VEC4>
__global__ __launch_bounds__(AUG_T) void aug_world(const float* __restrict__ in, int n, int ld, const int32_t* __restrict__ set_offsets, int batch,
                                                   const float* __restrict__ ops, const int32_t* __restrict__ op_offsets, float* __restrict__ out) {
  const int i = blockIdx.x * AUG_T + threadIdx.x;
  if (i >= n) return;
  const int s = aug_owner(set_offsets, batch, i);
  const float* p = in + (size_t)i * ld;
  float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float x, y, z;
  if (VEC4) {
    v4 = *reinterpret_cast<const float4*>(p);
    x = v4.x, y = v4.y, z = v4.z;
  } else {
    x = p[0], y = p[1], z = p[2];
  }
  float px, py, pz;
  aug_run_ops<true>(ops, op_offsets, s, false, x, y, z, px, py, pz);
  float* o = out + (size_t)i * ld;
  if (VEC4) *reinterpret_cast<float4*>(o) = make_float4(x, y, z, v4.w);
  else aug_store_row<false>(o, ld, x, y, z, p + 3);
}

}  // namespace

extern "C" size_t btc_augment_ws_bytes(int n_rows, int batch, int n_objects) {
  if (n_rows < 0 || batch < 1 || n_objects < 0) return 0;
  return BtcCompactWs::bytes(n_rows, true) + btc_align((size_t)(batch + 1) * sizeof(int32_t)) * 2 +
         btc_align((size_t)(n_objects + 1) * sizeof(int32_t));   // kept_off, paste_off, obj_prefix
}

extern "C" int btc_augment_batch(const float* points, int n_rows, int ld, const int32_t* scene_offsets, int batch, const float* rm_boxes,
                                 const int32_t* rm_offsets, const float* bank, long long bank_rows, const int32_t* obj_first,
                                 const int32_t* obj_rows, const double* obj_shift, const int32_t* obj_offsets, int n_objects, long long paste_rows,
                                 const float* ops, const int32_t* op_offsets, long long out_capacity, float* out, float* out_pre,
                                 int32_t* out_offsets, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(ld >= 3, "btc_augment_batch: need ld >= 3 (x, y, z columns), got %d", ld);
  BTC_CHECK_ARG(batch >= 1, "btc_augment_batch: need batch >= 1, got %d", batch);
  BTC_CHECK_ARG(n_rows >= 0 && n_objects >= 0 && paste_rows >= 0 && bank_rows >= 0 && out_capacity >= 0,
                "btc_augment_batch: negative count (n_rows %d, n_objects %d, paste_rows %lld, bank_rows %lld, out_capacity %lld)", n_rows, n_objects,
                paste_rows, bank_rows, out_capacity);
  BTC_CHECK_ARG((long long)n_rows + paste_rows < (1ll << 31), "btc_augment_batch: n_rows + paste_rows = %lld does not fit 31 bits",
                (long long)n_rows + paste_rows);
  BTC_CHECK_ARG(n_objects > 0 || paste_rows == 0, "btc_augment_batch: paste_rows without objects");
  BTC_CHECK_ARG(out_capacity >= (long long)n_rows + paste_rows, "btc_augment_batch: out_capacity %lld below n_rows + paste_rows = %lld", out_capacity,
                (long long)n_rows + paste_rows);
  BTC_CHECK_ARG(scene_offsets && rm_offsets && op_offsets && out_offsets && ws, "btc_augment_batch: missing pointer (offsets, out_offsets or ws)");
  BTC_CHECK_ARG(points || n_rows == 0, "btc_augment_batch: missing pointer (points)");
  BTC_CHECK_ARG(n_objects == 0 || (bank && obj_first && obj_rows && obj_shift && obj_offsets), "btc_augment_batch: missing pointer (bank or obj_*)");
  BTC_CHECK_ARG(out || out_capacity == 0, "btc_augment_batch: missing pointer (out)");
  BTC_CHECK_ARG(ws_bytes >= btc_augment_ws_bytes(n_rows, batch, n_objects), "btc_augment_batch: workspace too small");
  BtcCompactWs w(ws, n_rows, true);
  int32_t* kept_off = w.c.take<int32_t>(batch + 1);
  int32_t* paste_off = w.c.take<int32_t>(batch + 1);
  int32_t* obj_prefix = w.c.take<int32_t>(n_objects + 1);
  const int nb = w.nb;
  aug_mark<<<nb, AUG_T, 0, stream>>>(points, n_rows, ld, scene_offsets, batch, rm_boxes, rm_offsets, w.keep_flag, w.block_cnt);
  BTC_LAUNCH_CHECK();
  int rc = w.scan(stream);
  if (rc != BTC_OK) return rc;
  aug_offsets<<<batch + 2, 64, 0, stream>>>(w.keep_flag, n_rows, scene_offsets, batch, w.block_prefix, w.total, obj_rows, obj_offsets, n_objects,
                                           kept_off, paste_off, obj_prefix, out_offsets);
  BTC_LAUNCH_CHECK();
  const int grid = (n_rows > 0 ? nb : 0) + btc_cdiv(paste_rows, AUG_T);
  if (grid > 0) {
    const int nb_scan = n_rows > 0 ? nb : 0;
    const bool vec = ld == 4 && btc_aligned16(points) && btc_aligned16(bank) && btc_aligned16(out) && btc_aligned16(out_pre);
    if (vec)
      aug_emit<true><<<grid, AUG_T, 0, stream>>>(points, n_rows, ld, scene_offsets, batch, w.keep_flag, w.block_prefix, nb_scan, bank, bank_rows, obj_first,
                                                 obj_shift, obj_offsets, n_objects, paste_rows, obj_prefix, kept_off, paste_off, ops, op_offsets,
                                                 out_offsets, out_capacity, out, out_pre);
    else
      aug_emit<false><<<grid, AUG_T, 0, stream>>>(points, n_rows, ld, scene_offsets, batch, w.keep_flag, w.block_prefix, nb_scan, bank, bank_rows, obj_first,
                                                  obj_shift, obj_offsets, n_objects, paste_rows, obj_prefix, kept_off, paste_off, ops, op_offsets,
                                                  out_offsets, out_capacity, out, out_pre);
    BTC_LAUNCH_CHECK();
  }
  return BTC_OK;
}

extern "C" int btc_world_transform(const float* in, int n_rows, int ld, const int32_t* set_offsets, int batch, const float* ops,
                                   const int32_t* op_offsets, float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(ld >= 3, "btc_world_transform: need ld >= 3 (x, y, z columns), got %d", ld);
  BTC_CHECK_ARG(batch >= 1, "btc_world_transform: need batch >= 1, got %d", batch);
  BTC_CHECK_ARG(n_rows >= 0, "btc_world_transform: negative count (n_rows %d)", n_rows);
  BTC_CHECK_ARG(set_offsets && op_offsets, "btc_world_transform: missing pointer (offsets)");
  BTC_CHECK_ARG((in && out) || n_rows == 0, "btc_world_transform: missing pointer (in or out)");
  BTC_CHECK_ARG(in != out || n_rows == 0, "btc_world_transform: out may not alias in");
  if (n_rows == 0) return BTC_OK;
  const int nb = btc_cdiv(n_rows, AUG_T);
  if (ld == 4 && btc_aligned16(in) && btc_aligned16(out)) aug_world<true><<<nb, AUG_T, 0, stream>>>(in, n_rows, ld, set_offsets, batch, ops, op_offsets, out);
  else aug_world<false><<<nb, AUG_T, 0, stream>>>(in, n_rows, ld, set_offsets, batch, ops, op_offsets, out);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}
