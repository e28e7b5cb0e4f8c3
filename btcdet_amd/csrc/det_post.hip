// Fused post-processing of the detector's eval-mode outputs for gfx950 (include/btcdet_hip_infer.h: btc_det_select_nms, btc_det_finish).
//
// Replaces the per-scene Python loop of the reference's Detector3DTemplate.post_processing (detector3d_template.py:363-476) with
// model_nms_utils.class_agnostic_nms and generate_recall_record (:548-591): sigmoid, max, mask, nonzero, topk, an NMS with a host-side
// keep list, two IoU matrices and one read-back per recall threshold -- several dozen small launches and half a dozen read-backs per
// scene.  Here a batch is two launches and no read-back:
//
//   det_select_nms  grid (row blocks of 64 candidates, scenes).  EVERY workgroup repeats the cheap part -- scores, the threshold, a rank
//                   sort of <= 1024 keys in LDS (descending score, equal scores in ascending input index), the sorted boxes into LDS --
//                   then computes ITS 64 rows of the suppression mask over the valid candidates and publishes them to the workspace.
//                   The workgroup that draws the scene's last ticket walks the greedy chain (stopped at post_max kept boxes) and writes
//                   keep / num_keep.  The pair tests -- 524 K rotated IoUs at 1024 candidates -- are spread over the grid; the hand-over
//                   is the last-arriver protocol of btc_common.h.
//   det_finish      grid (ground-truth rows + 1, scenes).  Block g < G: the best 3-D IoU of ground truth g over the boxes (and the rois)
//                   -> the recall counters, added with 64-bit vector atomics.  Block G: the kept rows gathered into padded outputs and
//                   each output row's best IoU.
#include "btc_common.h"
#include "../../include/btcdet_hip_infer.h"
#include "iou3d_dev.h"

namespace {

constexpr int DET_MAX_N = 1024;      // candidates per scene (the ROI head's NMS_PRE_MAXSIZE at test time)
constexpr int DET_MAX_POST = 4096;
constexpr int DET_MAX_T = 8;         // recall thresholds
constexpr int DET_WORDS = DET_MAX_N / 64;

typedef unsigned long long u64;

// the score of one box and its class: sigmoid unless normalised, THEN the max (as the reference: the first of equal maxima wins, a NaN
// stays); raw: the max of the values as they are
__device__ __forceinline__ float det_score(const float* cls, int C, bool sigmoid, int* best_class) {
  float best = 0.f;
  int bc = 0;
  for (int c = 0; c < C; ++c) {
    const float x = cls[c];
    const float v = sigmoid ? 1.0f / (1.0f + expf(-x)) : x;
    if (c == 0 || v > best || (v != v && best == best)) {
      best = v;
      bc = c;
    }
  }
  *best_class = bc;
  return best;
}

struct SelArgs {
  const float* cls;      // (B, n, C)
  const float* boxes;    // (B, n, stride)
  int n, C, stride, normalized, rotated, pre_max, post_max;
  float score_thresh, nms_thresh;
  long long* keep;       // (B, post_max)
  int32_t* num_keep;     // (B)
  int32_t* best_class;   // (B, n)
  u64* mask;             // (B, n, words)
  int32_t* tickets;      // (B), zero at launch
  int words;             // row pitch of mask: (n + 63) / 64
};

__global__ __launch_bounds__(256) void det_select_nms(SelArgs a) {
  __shared__ u64 s_key[DET_MAX_N];
  __shared__ float s_box[DET_MAX_N * 7];            // the candidates' boxes in sorted order
  __shared__ unsigned short s_order[DET_MAX_N];     // sorted position -> input index
  __shared__ u64 s_remv[DET_WORDS];
  __shared__ u64 s_kept;
  __shared__ int s_count;
  const int s = blockIdx.y, rb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* cls = a.cls + (size_t)s * a.n * a.C;
  const float* boxes = a.boxes + (size_t)s * a.n * a.stride;
  if (tid == 0) s_count = 0;
  __syncthreads();
  // 1. score, class, threshold (a NaN fails >=).  key = (order-preserving bits of the score, ~index): a larger key sorts first
  for (int i = tid; i < a.n; i += 256) {
    int bc;
    float sc = det_score(cls + (size_t)i * a.C, a.C, !a.normalized, &bc);
    u64 key = 0;
    if (sc >= a.score_thresh) {
      sc += 0.0f;   // -0 -> +0: equal scores have equal bits
      unsigned u = __float_as_uint(sc);
      u = (u >> 31) ? ~u : (u | 0x80000000u);
      key = ((u64)u << 32) | (u64)(0xFFFFFFFFu - (unsigned)i);
      atomicAdd(&s_count, 1);
    }
    s_key[i] = key;
    if (rb == 0) a.best_class[(size_t)s * a.n + i] = bc;
  }
  __syncthreads();
  const int m = min(s_count, a.pre_max);   // candidates of the chain
  // 2. rank sort: the rank of a key is the number of larger keys (keys are distinct; 0 = below the threshold)
  for (int i = tid; i < a.n; i += 256) {
    const u64 k = s_key[i];
    if (k == 0) continue;
    int r = 0;
    for (int j = 0; j < a.n; ++j) r += (s_key[j] > k) ? 1 : 0;
    if (r < m) s_order[r] = (unsigned short)i;
  }
  __syncthreads();
  for (int e = tid; e < m * 7; e += 256) {
    const int r = e / 7, c = e - r * 7;
    s_box[e] = boxes[(size_t)s_order[r] * a.stride + c];
  }
  __syncthreads();
  // 3. this workgroup's rows of the mask: word (row, cb) bit j = candidate 64 cb + j (> row) overlaps candidate row above the threshold;
  //    wave w takes the column blocks rb + w, rb + w + 4, ...
  const int CB = (m + 63) >> 6;
  u64* mask = a.mask + (size_t)s * a.n * a.words;
  const int row = rb * 64 + lane;
  if (row < m) {
    float cur[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) cur[c] = s_box[row * 7 + c];
    for (int cb = rb + wave; cb < CB; cb += 4) {
      const int cols = min(m - cb * 64, 64);
      u64 t = 0;
      for (int j = (cb == rb) ? lane + 1 : 0; j < cols; ++j) {
        const float* o = s_box + (cb * 64 + j) * 7;
        const float v = a.rotated ? iou_bev(cur, o) : iou_normal(cur, o);
        if (v > a.nms_thresh) t |= 1ull << j;
      }
      btc_st_agent(mask + (size_t)row * a.words + cb, t);
    }
  }
  // 4. last-arriver hand-over (btc_common.h) among the scene's workgroups; the acquiring lane then waits for its invalidate before the
  //    workgroup meets again below
  if (!btc_last_arriver(a.tickets + s, (int)gridDim.x)) return;
  if (tid == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (tid < DET_WORDS) s_remv[tid] = 0ull;
  __syncthreads();
  // 5. the greedy chain, 64 candidates at a time (as nms_reduce of iou3d_nms.hip), stopped at post_max kept boxes
  long long* keep = a.keep + (size_t)s * a.post_max;
  int nk = 0;
  for (int b = 0; b < CB; ++b) {
    const int rows = min(m - b * 64, 64);
    if (wave == 0) {
      const u64 diag = (lane < rows) ? btc_ld_agent(mask + (size_t)(b * 64 + lane) * a.words + b) : 0ull;
      const unsigned dlo = (unsigned)diag, dhi = (unsigned)(diag >> 32);
      u64 rem = s_remv[b], kept = 0ull;
      for (int i = 0; i < rows; ++i) {  // wave-uniform
        if (!((rem >> i) & 1ull)) {
          kept |= 1ull << i;
          rem |= ((u64)(unsigned)__builtin_amdgcn_readlane((int)dhi, i) << 32) | (u64)(unsigned)__builtin_amdgcn_readlane((int)dlo, i);
        }
      }
      const int rank = nk + __popcll(kept & ((1ull << lane) - 1ull));
      if (((kept >> lane) & 1ull) && rank < a.post_max) keep[rank] = (long long)s_order[b * 64 + lane];
      if (lane == 0) s_kept = kept;
    }
    __syncthreads();
    const u64 kept = s_kept;
    nk += __popcll(kept);
    if (nk >= a.post_max) {   // block-uniform
      nk = a.post_max;
      break;
    }
    if (lane < rows && ((kept >> lane) & 1ull))
      for (int j = b + 1 + wave; j < CB; j += 4) atomicOr(&s_remv[j], btc_ld_agent(mask + (size_t)(b * 64 + lane) * a.words + j));
    __syncthreads();
  }
  for (int i = nk + tid; i < a.post_max; i += 256) keep[i] = -1;
  if (tid == 0) a.num_keep[s] = nk;
}

// 3-D IoU of iou3d_nms_utils.boxes_iou3d_gpu: BEV overlap x height overlap over the union volume, operation by operation
__device__ __forceinline__ float iou3d(const float* a, const float* b) {
  const float ov = box_overlap(a, b);
  const float hmax = fminf(a[2] + a[5] / 2, b[2] + b[5] / 2), hmin = fmaxf(a[2] - a[5] / 2, b[2] - b[5] / 2);
  const float o3 = ov * fmaxf(hmax - hmin, 0.f);
  const float va = a[3] * a[4] * a[5], vb = b[3] * b[4] * b[5];
  return o3 / fmaxf(va + vb - o3, 1e-6f);
}

struct FinArgs {
  const float* cls;
  const float* boxes;
  int n, C, stride, normalized, raw_score, post_max;
  const long long* keep;
  const int32_t* num_keep;
  const int32_t* best_class;
  const long long* labels;   // (B, n) or NULL
  const float* gt;           // (B, G, gt_stride) or NULL
  int G, gt_stride;
  const float* rois;         // (B, nr, roi_stride) or NULL
  int nr, roi_stride;
  float thr[DET_MAX_T];
  int T;
  float* pred_boxes;         // (B, post_max, stride)
  float* pred_scores;        // (B, post_max)
  long long* pred_labels;    // (B, post_max)
  float* pred_iou;           // (B, post_max)
  u64* counters;             // [1 + 2T]
};

__device__ __forceinline__ float block_max(float v, float* s_red) {
  v = btc_wave_reduce(v, [](float a, float b) { return fmaxf(a, b); });
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  __syncthreads();
  return v;
}

__global__ __launch_bounds__(256) void det_finish(FinArgs a) {
  __shared__ int s_last_nz;
  __shared__ float s_red[4];
  const int s = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
  const float* boxes = a.boxes + (size_t)s * a.n * a.stride;
  const float* gt = a.gt ? a.gt + (size_t)s * a.G * a.gt_stride : nullptr;
  const long long* keep = a.keep + (size_t)s * a.post_max;
  const int nk = min(max(a.num_keep[s], 0), a.post_max);
  // the scene's ground truth: trailing rows whose entries sum to zero are trimmed, never the first row (the reference's `while k > 0`)
  if (tid == 0) s_last_nz = 0;
  __syncthreads();
  for (int r = tid; r < a.G; r += 256) {
    float sum = 0.f;
    for (int c = 0; c < a.gt_stride; ++c) sum += gt[(size_t)r * a.gt_stride + c];
    if (sum != 0.f) atomicMax(&s_last_nz, r);
  }
  __syncthreads();
  const int ngt = a.G > 0 ? s_last_nz + 1 : 0;
  if (g < a.G) {
    // ---- recall of ground truth g: its best IoU over all n boxes when rois are given (the reference hands src_box_preds over), else over
    //      the kept boxes; and over the rois
    if (g >= ngt) return;   // block-uniform
    float gb[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) gb[c] = gt[(size_t)g * a.gt_stride + c];
    float best = 0.f, best_roi = 0.f;
    if (a.rois) {
      for (int i = tid; i < a.n; i += 256) best = fmaxf(best, iou3d(boxes + (size_t)i * a.stride, gb));
      const float* rois = a.rois + (size_t)s * a.nr * a.roi_stride;
      for (int i = tid; i < a.nr; i += 256) best_roi = fmaxf(best_roi, iou3d(rois + (size_t)i * a.roi_stride, gb));
      best_roi = block_max(best_roi, s_red);
    } else {
      for (int k = tid; k < nk; k += 256) {
        const long long idx = keep[k];
        if (idx >= 0 && idx < a.n) best = fmaxf(best, iou3d(boxes + (size_t)idx * a.stride, gb));
      }
    }
    best = block_max(best, s_red);
    if (tid == 0) {
      if (g == 0) atomicAdd(a.counters, (u64)ngt);
      for (int t = 0; t < a.T; ++t) {
        if (a.rois && best_roi > a.thr[t]) atomicAdd(a.counters + 1 + t, 1ull);
        if (best > a.thr[t]) atomicAdd(a.counters + 1 + a.T + t, 1ull);
      }
    }
    return;
  }
  // ---- block G: the padded outputs
  const float* cls = a.cls + (size_t)s * a.n * a.C;
  float* pb = a.pred_boxes + (size_t)s * a.post_max * a.stride;
  for (int k = tid; k < a.post_max; k += 256) {
    float score = 0.f, iou = 0.f;
    long long label = 0;
    const long long idx = k < nk ? keep[k] : -1;
    const bool row = idx >= 0 && idx < a.n;   // (an index outside the inputs is a padding row, never an address)
    if (row) {
      for (int c = 0; c < a.stride; ++c) pb[(size_t)k * a.stride + c] = boxes[(size_t)idx * a.stride + c];
      int bc;
      score = det_score(cls + (size_t)idx * a.C, a.C, !a.normalized && !a.raw_score, &bc);
      label = a.labels ? a.labels[(size_t)s * a.n + idx] : (long long)a.best_class[(size_t)s * a.n + idx] + 1;
    } else {
      for (int c = 0; c < a.stride; ++c) pb[(size_t)k * a.stride + c] = 0.f;
    }
    // best IoU of an output row: of kept box k -- or, with rois, of INPUT box k (the reference takes the row maxima of the matrix it
    // built, which is over all n boxes then; post_processing() hands it on only where the reference does)
    const long long src = a.rois ? (k < a.n ? (long long)k : -1) : (row ? idx : -1);
    if (src >= 0)
      for (int j = 0; j < ngt; ++j) iou = fmaxf(iou, iou3d(boxes + (size_t)src * a.stride, gt + (size_t)j * a.gt_stride));
    a.pred_scores[(size_t)s * a.post_max + k] = score;
    a.pred_labels[(size_t)s * a.post_max + k] = label;
    a.pred_iou[(size_t)s * a.post_max + k] = iou;
  }
}

}  // namespace

extern "C" size_t btc_det_select_nms_ws_bytes(int batch, int n) {
  if (batch <= 0 || n <= 0) return 256;
  return btc_align((size_t)batch * sizeof(int32_t)) + btc_align((size_t)batch * n * ((n + 63) / 64) * sizeof(u64));
}

extern "C" int btc_det_select_nms(const float* cls_preds, const float* box_preds, int batch, int n, int num_class, int box_stride, int normalized,
                                  float score_thresh, float nms_thresh, int rotated, int pre_max, int post_max, long long* keep,
                                  int32_t* num_keep, int32_t* best_class, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(batch >= 0 && n >= 0, "btc_det_select_nms: bad sizes (batch %d, n %d)", batch, n);
  BTC_CHECK_ARG(n <= DET_MAX_N, "btc_det_select_nms: n = %d exceeds %d candidates per scene (sort the scores and use btc_nms_topk)", n, DET_MAX_N);
  BTC_CHECK_ARG(num_class >= 1, "btc_det_select_nms: num_class = %d", num_class);
  BTC_CHECK_ARG(box_stride >= 7, "btc_det_select_nms: box_stride = %d, a box has 7 values", box_stride);
  BTC_CHECK_ARG(pre_max >= 1 && post_max >= 1 && post_max <= DET_MAX_POST, "btc_det_select_nms: pre_max = %d, post_max = %d (1 .. %d)", pre_max,
                post_max, DET_MAX_POST);
  BTC_CHECK_ARG(keep && num_keep && ws && (n == 0 || (cls_preds && box_preds && best_class)), "btc_det_select_nms: missing pointer");
  BTC_CHECK_ARG(ws_bytes >= btc_det_select_nms_ws_bytes(batch, n), "btc_det_select_nms: workspace too small");
  if (batch == 0) return BTC_OK;
  SelArgs a;
  a.cls = cls_preds; a.boxes = box_preds; a.n = n; a.C = num_class; a.stride = box_stride; a.normalized = normalized; a.rotated = rotated;
  a.pre_max = pre_max; a.post_max = post_max; a.score_thresh = score_thresh; a.nms_thresh = nms_thresh;
  a.keep = keep; a.num_keep = num_keep; a.best_class = best_class;
  a.words = (n + 63) / 64;
  BtcCarver cv(ws);
  a.tickets = cv.take<int32_t>(batch);
  a.mask = cv.take<u64>((size_t)batch * n * a.words);
  BTC_HIP(hipMemsetAsync(a.tickets, 0, btc_align((size_t)batch * sizeof(int32_t)), stream));   // the workspace arrives as garbage
  det_select_nms<<<dim3(a.words > 0 ? a.words : 1, batch), 256, 0, stream>>>(a);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}

extern "C" int btc_det_finish(const float* cls_preds, const float* box_preds, int batch, int n, int num_class, int box_stride, int normalized,
                              int raw_score, const long long* keep, const int32_t* num_keep, const int32_t* best_class, const long long* labels,
                              int post_max, const float* gt_boxes, int n_gt, int gt_stride, const float* rois, int n_rois, int roi_stride,
                              const float* h_thresh, int n_thresh, float* pred_boxes, float* pred_scores, long long* pred_labels,
                              float* pred_iou, long long* counters, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(batch >= 0 && n >= 0, "btc_det_finish: bad sizes (batch %d, n %d)", batch, n);
  BTC_CHECK_ARG(num_class >= 1, "btc_det_finish: num_class = %d", num_class);
  BTC_CHECK_ARG(box_stride >= 7, "btc_det_finish: box_stride = %d, a box has 7 values", box_stride);
  BTC_CHECK_ARG(post_max >= 1 && post_max <= DET_MAX_POST, "btc_det_finish: post_max = %d (1 .. %d)", post_max, DET_MAX_POST);
  BTC_CHECK_ARG(n_thresh >= 0 && n_thresh <= DET_MAX_T, "btc_det_finish: %d recall thresholds (at most %d)", n_thresh, DET_MAX_T);
  BTC_CHECK_ARG(n_gt >= 0 && n_gt <= 65535 && (!gt_boxes || n_gt == 0 || gt_stride >= 7), "btc_det_finish: bad ground truth (%d rows of %d values)",
                n_gt, gt_stride);
  BTC_CHECK_ARG(!rois || (n_rois >= 0 && roi_stride >= 7), "btc_det_finish: bad rois (%d rows of %d values)", n_rois, roi_stride);
  BTC_CHECK_ARG(keep && num_keep && pred_boxes && pred_scores && pred_labels && pred_iou && (n == 0 || (cls_preds && box_preds)) &&
                    (labels || best_class || n == 0),
                "btc_det_finish: missing pointer");
  BTC_CHECK_ARG(n_thresh == 0 || h_thresh, "btc_det_finish: missing pointer (h_thresh)");
  BTC_CHECK_ARG(!gt_boxes || n_gt == 0 || counters, "btc_det_finish: missing pointer (ground truth without counters)");
  if (batch == 0) return BTC_OK;
  FinArgs a;
  a.cls = cls_preds; a.boxes = box_preds; a.n = n; a.C = num_class; a.stride = box_stride; a.normalized = normalized; a.raw_score = raw_score;
  a.post_max = post_max; a.keep = keep; a.num_keep = num_keep; a.best_class = best_class; a.labels = labels;
  a.gt = (gt_boxes && n_gt > 0) ? gt_boxes : nullptr;
  a.G = a.gt ? n_gt : 0;
  a.gt_stride = gt_stride;
  a.rois = a.gt ? rois : nullptr;   // (the rois enter the recall record only)
  a.nr = n_rois; a.roi_stride = roi_stride;
  a.T = n_thresh;
  for (int t = 0; t < DET_MAX_T; ++t) a.thr[t] = t < n_thresh ? h_thresh[t] : 0.f;
  a.pred_boxes = pred_boxes; a.pred_scores = pred_scores; a.pred_labels = pred_labels; a.pred_iou = pred_iou;
  a.counters = (u64*)counters;
  det_finish<<<dim3(a.G + 1, batch), 256, 0, stream>>>(a);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}
