// Rotated BEV overlap / IoU and NMS for gfx950 (the first component next to the hot path).
//
// Replaces /root/reference/btcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu (box_overlap :107-233, iou_bev :235-243,
// nms_kernel :268-309, nms_normal_kernel :325-362) and the host side of iou3d_nms.cpp:90-188, which for every NMS call
// cudaMallocs the N x N/64 suppression mask, copies it to the host (10 MB at 9 000 proposals), walks it on one CPU core
// and frees it again.  Here the mask never leaves the device: one kernel builds its upper triangle, one 256-thread
// workgroup resolves the greedy chain 64 boxes at a time (the in-block dependency with v_readlane on the diagonal word,
// the kept rows OR-ed into the remaining removal words by all threads) and writes the kept positions and their count;
// no allocation, no copy, no host loop, one optional 4-byte read-back of the count.
// Per pair the arithmetic follows the reference's fp32 formulation (edge intersections + corners inside the other box
// with its 1 cm margin, ordered by atan2 about their centroid, fan area) so that IoU values -- and with them the NMS
// decisions -- agree with it up to the last-ulp differences of cosf / sinf / atan2f.
#include "btc_common.h"
#include "iou3d_dev.h"   // box_overlap, iou_bev, iou_normal: shared with det_post.hip

namespace {

// one thread per (a, b) pair; a 16 x 16 workgroup shares 16 + 16 boxes through LDS
__global__ __launch_bounds__(256) void pairwise_bev(const float* __restrict__ boxes_a, int na, const float* __restrict__ boxes_b, int nb,
                                                    int mode, float* __restrict__ out) {
  __shared__ float sa[16 * 7], sb[16 * 7];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int a0 = blockIdx.y * 16, b0 = blockIdx.x * 16;
  if (threadIdx.x < 112) {
    const int r = threadIdx.x / 7, c = threadIdx.x % 7;
    sa[threadIdx.x] = (a0 + r < na) ? boxes_a[(size_t)(a0 + r) * 7 + c] : 0.f;
    sb[threadIdx.x] = (b0 + r < nb) ? boxes_b[(size_t)(b0 + r) * 7 + c] : 0.f;
  }
  __syncthreads();
  const int ia = a0 + ty, ib = b0 + tx;
  if (ia >= na || ib >= nb) return;
  out[(size_t)ia * nb + ib] = mode ? iou_bev(sa + ty * 7, sb + tx * 7) : box_overlap(sa + ty * 7, sb + tx * 7);
}

// mask[i][cb] bit j: box 64 cb + j (> i) overlaps box i above the threshold; upper triangle of 64 x 64 blocks only
__global__ __launch_bounds__(64) void nms_mask(const float* __restrict__ boxes, int n, float thresh, int rotated,
                                               unsigned long long* __restrict__ mask) {
  const int rb = blockIdx.y, cb = blockIdx.x;
  if (cb < rb) return;
  __shared__ float sbox[64 * 7];
  const int col_blocks = (n + 63) / 64;
  const int col_size = min(n - cb * 64, 64), row_size = min(n - rb * 64, 64);
  for (int e = threadIdx.x; e < col_size * 7; e += 64) sbox[e] = boxes[(size_t)cb * 64 * 7 + e];
  __syncthreads();
  if ((int)threadIdx.x >= row_size) return;
  const int i = rb * 64 + threadIdx.x;
  float cur[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) cur[c] = boxes[(size_t)i * 7 + c];
  unsigned long long t = 0;
  for (int j = (rb == cb) ? (int)threadIdx.x + 1 : 0; j < col_size; ++j) {
    const float v = rotated ? iou_bev(cur, sbox + j * 7) : iou_normal(cur, sbox + j * 7);
    if (v > thresh) t |= 1ull << j;
  }
  mask[(size_t)i * col_blocks + cb] = t;
}

// greedy chain over the mask, one 256-thread workgroup; keep: kept positions ascending, *num_keep their number
__global__ __launch_bounds__(256) void nms_reduce(const unsigned long long* __restrict__ mask, int n, long long* __restrict__ keep,
                                                  int32_t* __restrict__ num_keep) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* remv = (unsigned long long*)smem;  // [col_blocks]
  __shared__ unsigned long long s_kept;
  const int col_blocks = (n + 63) / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = tid; j < col_blocks; j += 256) remv[j] = 0ull;
  __syncthreads();
  int nk = 0;
  for (int b = 0; b < col_blocks; ++b) {
    const int rows = min(n - b * 64, 64);
    if (wave == 0) {
      const unsigned long long diag = (lane < rows) ? mask[(size_t)(b * 64 + lane) * col_blocks + b] : 0ull;
      const unsigned dlo = (unsigned)diag, dhi = (unsigned)(diag >> 32);
      unsigned long long rem = remv[b], kept = 0ull;
      for (int i = 0; i < rows; ++i) {  // wave-uniform
        if (!((rem >> i) & 1ull)) {
          kept |= 1ull << i;
          rem |= ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)dhi, i) << 32) |
                 (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)dlo, i);  // (unsigned): no sign extension
        }
      }
      if ((kept >> lane) & 1ull) keep[nk + __popcll(kept & ((1ull << lane) - 1ull))] = (long long)b * 64 + lane;
      if (lane == 0) s_kept = kept;
    }
    __syncthreads();
    const unsigned long long kept = s_kept;
    nk += __popcll(kept);
    for (int j = b + 1 + tid; j < col_blocks; j += 256) {
      unsigned long long acc = remv[j], m = kept;
      while (m) {
        const int i = __ffsll((long long)m) - 1;
        m &= m - 1;
        acc |= mask[(size_t)(b * 64 + i) * col_blocks + j];
      }
      remv[j] = acc;
    }
    __syncthreads();
  }
  if (tid == 0) *num_keep = nk;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Greedy NMS that STOPS at max_keep kept boxes (round 4).  The reference runs the full chain over NMS_PRE_MAXSIZE = 9000 boxes per
// scene and then takes keep[:NMS_POST_MAXSIZE] (model_nms_utils.py:6-25, roi_head_template.py:45-100); whether box i is kept depends on
// the kept boxes before it only, so the first max_keep kept boxes of the full chain are exactly what a chain that stops there
// produces -- and at 9000 boxes the full chain is 81 M pair tests (nms_mask 1.2 ms) plus a 2.5 ms walk of ONE workgroup per scene.
// Here the candidates are taken in chunks of TOPK_CHUNK: the work array of a scene is [K slots: the boxes kept so far, unused slots =
// far-away dummies that overlap nothing][the chunk]; the ordinary mask + chain over that array continues the greedy chain exactly
// (kept boxes do not suppress each other, so they stay kept; a candidate is suppressed by a kept box or by an earlier candidate);
// the chain appends the chunk's kept boxes to the kept slots.  Every kernel of a later chunk returns at once when the scene is full:
// no host read-back anywhere.  All scenes of a batch share the launches (blockIdx.z).
constexpr int TOPK_CHUNK = 2560;
constexpr int TOPK_CHUNK0 = 768;    // the first chunk: with the usual keep rates a few hundred candidates fill NMS_POST_MAXSIZE = 256
                                   // (its mask is (K + 768)^2 / 2 pair tests instead of (K + 2560)^2 / 2: 0.49 -> ~0.07 ms)

struct TopkArgs {
  const float* boxes;        // (B, n, 7) sorted by descending score
  float* work;               // (B, Tmax, 7), Tmax = K + TOPK_CHUNK
  unsigned long long* mask;  // (B, Tmax, Tmax / 64) (a launch over T <= Tmax rows uses rows of T / 64 words)
  int Tmax;
  long long* keep;           // (B, max_keep), -1 padded
  int32_t* num_keep;         // (B)
  int n, K, T, max_keep, chunk0, chunk_n, rotated;   // T: rows of the work array in THIS launch (K + the chunk, a multiple of 64); chunk_n: candidates in it
  float thresh;
};

__device__ __forceinline__ void dummy_box(float* b, int slot) {
  b[0] = 1.0e7f + 64.f * (float)slot; b[1] = 1.0e7f; b[2] = 0.f; b[3] = 1.f; b[4] = 1.f; b[5] = 1.f; b[6] = 0.f;
}

__global__ __launch_bounds__(256) void topk_init(TopkArgs a) {
  const int s = blockIdx.z;
  for (int i = threadIdx.x; i < a.K; i += 256) dummy_box(a.work + ((size_t)s * a.Tmax + i) * 7, i);
  for (int i = threadIdx.x; i < a.max_keep; i += 256) a.keep[(size_t)s * a.max_keep + i] = -1;
  if (threadIdx.x == 0) a.num_keep[s] = 0;
}

__global__ __launch_bounds__(256) void topk_load(TopkArgs a) {
  const int s = blockIdx.z;
  if (a.num_keep[s] >= a.max_keep) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.T - a.K) return;
  float* dst = a.work + ((size_t)s * a.Tmax + a.K + j) * 7;
  const int src = a.chunk0 + j;
  if (j < a.chunk_n && src < a.n) {
    const float* p = a.boxes + ((size_t)s * a.n + src) * 7;
#pragma unroll
    for (int c = 0; c < 7; ++c) dst[c] = p[c];
  } else {
    dummy_box(dst, a.K + j);
  }
}

__global__ __launch_bounds__(64) void topk_mask(TopkArgs a) {
  const int s = blockIdx.z;
  if (a.num_keep[s] >= a.max_keep) return;
  const int rb = blockIdx.y, cb = blockIdx.x;
  if (cb < rb) return;
  __shared__ float sbox[64 * 7];
  const float* boxes = a.work + (size_t)s * a.Tmax * 7;
  for (int e = threadIdx.x; e < 64 * 7; e += 64) sbox[e] = boxes[(size_t)cb * 64 * 7 + e];
  __syncthreads();
  const int i = rb * 64 + threadIdx.x;
  float cur[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) cur[c] = boxes[(size_t)i * 7 + c];
  unsigned long long t = 0;
  for (int j = (rb == cb) ? (int)threadIdx.x + 1 : 0; j < 64; ++j) {
    const float v = a.rotated ? iou_bev(cur, sbox + j * 7) : iou_normal(cur, sbox + j * 7);
    if (v > a.thresh) t |= 1ull << j;
  }
  a.mask[((size_t)s * a.Tmax + i) * (a.Tmax / 64) + cb] = t;
}

// the chain of nms_reduce over the scene's work array; emits the chunk's kept boxes (positions >= K) into keep / the kept slots
__global__ __launch_bounds__(256) void topk_chain(TopkArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* remv = (unsigned long long*)smem;  // [col_blocks]
  __shared__ unsigned long long s_kept;
  __shared__ int s_nk;
  const int s = blockIdx.z;
  const int nk0 = a.num_keep[s];
  if (nk0 >= a.max_keep) return;
  const int col_blocks = a.T / 64, mstride = a.Tmax / 64;
  const unsigned long long* mask = a.mask + (size_t)s * a.Tmax * mstride;
  float* work = a.work + (size_t)s * a.Tmax * 7;
  long long* keep = a.keep + (size_t)s * a.max_keep;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = tid; j < col_blocks; j += 256) remv[j] = 0ull;
  if (tid == 0) s_nk = nk0;
  __syncthreads();
  const int n_here = min(a.n - a.chunk0, a.chunk_n);   // real candidates of this chunk (the rest of the array is dummies)
  for (int b = 0; b < col_blocks; ++b) {
    if (wave == 0) {
      const unsigned long long diag = mask[(size_t)(b * 64 + lane) * mstride + b];
      const unsigned dlo = (unsigned)diag, dhi = (unsigned)(diag >> 32);
      unsigned long long rem = remv[b], kept = 0ull;
      for (int i = 0; i < 64; ++i) {  // wave-uniform
        if (!((rem >> i) & 1ull)) {
          kept |= 1ull << i;
          rem |= ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)dhi, i) << 32) |
                 (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)dlo, i);
        }
      }
      // new kept boxes: candidates of this chunk (array position >= K, a real box), in order, until the scene is full
      const int pos = b * 64 + lane;
      const bool fresh = ((kept >> lane) & 1ull) && pos >= a.K && (pos - a.K) < n_here;
      const unsigned long long fm = __ballot(fresh);
      const int nk = s_nk;
      const int rank = nk + __popcll(fm & ((1ull << lane) - 1ull));
      if (fresh && rank < a.max_keep) {
        keep[rank] = (long long)a.chunk0 + (pos - a.K);
        if (rank < a.K) {
#pragma unroll
          for (int c = 0; c < 7; ++c) work[(size_t)rank * 7 + c] = work[(size_t)pos * 7 + c];   // (slot rank < K <= pos: no aliasing with a row still to be read)
        }
      }
      if (lane == 0) {
        s_kept = kept;
        s_nk = min(nk + __popcll(fm), a.max_keep);
      }
    }
    __syncthreads();
    if (s_nk >= a.max_keep) break;   // block-uniform
    const unsigned long long kept = s_kept;
    for (int j = b + 1 + tid; j < col_blocks; j += 256) {
      unsigned long long acc = remv[j], m = kept;
      while (m) {
        const int i = __ffsll((long long)m) - 1;
        m &= m - 1;
        acc |= mask[(size_t)(b * 64 + i) * mstride + j];
      }
      remv[j] = acc;
    }
    __syncthreads();
  }
  if (tid == 0) a.num_keep[s] = s_nk;
}

}  // namespace

extern "C" size_t btc_nms_topk_ws_bytes(int batch, int n, int max_keep) {
  if (batch <= 0 || max_keep <= 0) return 256;
  const size_t K = (size_t)(max_keep + 63) / 64 * 64, T = K + TOPK_CHUNK;
  return btc_align((size_t)batch * T * 7 * sizeof(float)) + btc_align((size_t)batch * T * (T / 64) * sizeof(unsigned long long));
}

extern "C" int btc_nms_topk(const float* boxes_sorted, int batch, int n, float thresh, int rotated, int max_keep, long long* keep,
                            int32_t* d_num_keep, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(batch >= 0 && n >= 0 && max_keep >= 1 && max_keep <= 4096, "btc_nms_topk: bad sizes (batch %d, n %d, max_keep %d)", batch, n, max_keep);
  BTC_CHECK_ARG(ws_bytes >= btc_nms_topk_ws_bytes(batch, n, max_keep), "btc_nms_topk: workspace too small");
  if (batch == 0) return BTC_OK;
  TopkArgs a;
  a.boxes = boxes_sorted; a.keep = keep; a.num_keep = d_num_keep; a.n = n; a.max_keep = max_keep; a.rotated = rotated; a.thresh = thresh;
  a.K = (max_keep + 63) / 64 * 64;
  a.Tmax = a.K + TOPK_CHUNK;
  a.T = a.Tmax;
  BtcCarver cv(ws);
  a.work = cv.take<float>((size_t)batch * a.Tmax * 7);
  a.mask = cv.take<unsigned long long>((size_t)batch * a.Tmax * (a.Tmax / 64));
  a.chunk0 = 0;
  a.chunk_n = 0;
  topk_init<<<dim3(1, 1, batch), 256, 0, stream>>>(a);
  BTC_LAUNCH_CHECK();
  for (int c0 = 0; c0 < n; c0 += a.chunk_n) {
    a.chunk0 = c0;
    a.chunk_n = c0 == 0 ? TOPK_CHUNK0 : (a.chunk_n * 2 < TOPK_CHUNK ? a.chunk_n * 2 : TOPK_CHUNK);   // 768, 1536, 2560, 2560, ...
    a.T = a.K + a.chunk_n;          // (both chunk sizes are multiples of 64)
    const int cb = a.T / 64;
    topk_load<<<dim3(btc_cdiv(a.chunk_n, 256), 1, batch), 256, 0, stream>>>(a);
    topk_mask<<<dim3(cb, cb, batch), 64, 0, stream>>>(a);
    topk_chain<<<dim3(1, 1, batch), 256, (size_t)cb * 8, stream>>>(a);
    BTC_LAUNCH_CHECK();
  }
  return BTC_OK;
}

extern "C" int btc_boxes_pairwise_bev(const float* boxes_a, int na, const float* boxes_b, int nb, int mode, float* out, void* stream) {
  BTC_CHECK_ARG(na >= 0 && nb >= 0 && (mode == 0 || mode == 1), "btc_boxes_pairwise_bev: bad arguments");
  if (na == 0 || nb == 0) return BTC_OK;
  dim3 grid(btc_cdiv(nb, 16), btc_cdiv(na, 16));
  pairwise_bev<<<grid, 256, 0, (hipStream_t)stream>>>(boxes_a, na, boxes_b, nb, mode, out);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}

extern "C" size_t btc_nms_ws_bytes(int n) {
  const size_t cb = (size_t)(n + 63) / 64;
  return btc_align((size_t)(n > 0 ? n : 1) * cb * sizeof(unsigned long long));
}

extern "C" int btc_nms(const float* boxes_sorted, int n, float thresh, int rotated, long long* keep, int32_t* d_num_keep, void* ws,
                       size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(n >= 0, "btc_nms: bad size");
  BTC_CHECK_ARG(ws_bytes >= btc_nms_ws_bytes(n), "btc_nms: workspace too small");
  if (n == 0) {
    BTC_HIP(hipMemsetAsync(d_num_keep, 0, sizeof(int32_t), stream));
    return BTC_OK;
  }
  const int cb = (n + 63) / 64;
  BTC_CHECK_ARG((size_t)cb * 8 <= 64 * 1024, "btc_nms: %d boxes exceed the removal words that fit the LDS (max 524288)", n);
  unsigned long long* mask = (unsigned long long*)ws;
  nms_mask<<<dim3(cb, cb), 64, 0, stream>>>(boxes_sorted, n, thresh, rotated, mask);
  BTC_LAUNCH_CHECK();
  nms_reduce<<<1, 256, (size_t)cb * 8, stream>>>(mask, n, keep, d_num_keep);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}
