// The ROI head's training targets, fused (include/btcdet_hip_roi_targets.h: ONE launch per batch).
//
// Replaces ProposalTargetLayer.forward + canonical_targets of btcdet_amd/roi_targets.py (the reference's
// btcdet/models/roi_heads/target_assigner/proposal_target_layer.py:13-228 and roi_head_template.py:102-134): per scene a
// pairwise-overlap launch, a dozen elementwise launches for the 3-D IoU, a masked max, three sorts and five gathers, then the stacks, the
// label arithmetic and the canonical transform.
//   matching : workgroups tile (scene, RT_TILE rois); the RT_LANES lanes of a roi share its boxes and meet in a butterfly; the tile's
//              max_overlaps / gt_assignment leave with agent-scope stores
//   ticket   : btc_last_arriver on the scene's counter; the workgroup that completes a scene reads the scene's N overlaps back into LDS
//              and runs its sampling, gather, labels and transform; it leaves the counter zero.  No workgroup waits on another.
// Every index is formed from b < B, n < N, g < G, j < R; a sampled index is clamped into [0, N) and an assignment into [0, G) before
// it addresses anything; a draw is clamped into [0, max(n, 1) - 1] as a double before it becomes an index (a NaN uniform lands on 0).
#include "iou3d_dev.h"

#include "../../include/btcdet_hip_roi_targets.h"

namespace {

constexpr int RT_T = BTC_ROI_TARGETS_THREADS;
constexpr int RT_LANES = BTC_ROI_TARGETS_LANES;
constexpr int RT_TILE = BTC_ROI_TARGETS_TILE;
constexpr int RT_WAVES = RT_T / 64;
constexpr int RT_MAX = BTC_ROI_TARGETS_MAX_N;
constexpr int RT_PER = RT_MAX / RT_T;   // consecutive rois of one thread in the per-scene scans
static_assert(RT_LANES >= 1 && RT_LANES <= 64 && (RT_LANES & (RT_LANES - 1)) == 0 && RT_T % 64 == 0 && RT_MAX % RT_T == 0, "tile constants");
static_assert(BTC_ROI_TARGETS_MAX_R <= 65535 && RT_MAX <= 65535, "the per-scene lists hold 16-bit indices");

constexpr float RT_TWO_PI = (float)(2.0 * 3.14159265358979323846);
constexpr float RT_PI = (float)3.14159265358979323846;
constexpr float RT_HALF_PI = (float)(3.14159265358979323846 * 0.5);
constexpr float RT_THREE_HALF_PI = (float)(3.14159265358979323846 * 1.5);

struct RtParams {
  int B, N, G, M, tiles;
  BtcRoiTargetsConfig c;
  float inv_span;
};

struct RtOut {
  float *rois, *gt, *gt_src, *iou, *scores;
  int64_t *labels, *reg_valid;
  void* cls;
  float* max_overlaps;
  int64_t *gt_assignment, *sampled;
};

// torch's elementwise max / min / clamp: a NaN operand is handed on
__device__ __forceinline__ float rt_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }
__device__ __forceinline__ float rt_min(float a, float b) { return (a != a) ? a : ((b != b) ? b : (a < b ? a : b)); }

// the order of the masked max: larger value first (a NaN the largest), then the lower box index
__device__ __forceinline__ bool rt_better(float v, int g, float bv, int bg) {
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;
  if (!vn && v != bv) return v > bv;
  return g < bg;
}

__device__ __forceinline__ float rt_iou3d(const float* a, const float* b) {
  const float o = box_overlap(a, b);
  const float ha = a[5] / 2, hb = b[5] / 2;
  const float top = rt_min(a[2] + ha, b[2] + hb), bot = rt_max(a[2] - ha, b[2] - hb);
  const float h = rt_max(top - bot, 0.0f);
  const float o3 = o * h;
  const float va = (a[3] * a[4]) * a[5], vb = (b[3] * b[4]) * b[5];
  const float den = rt_max((va + vb) - o3, 1e-6f);
  return o3 / den;
}

__device__ __forceinline__ float rt_mod_two_pi(float x) {
  float m = fmodf(x, RT_TWO_PI);
  if (m != 0.0f && m < 0.0f) m += RT_TWO_PI;
  return m;
}

// members of `flag` in ascending index, then the non-members in ascending index (thread t owns rois t * RT_PER ..)
__device__ __forceinline__ int rt_list(const bool* flag /* RT_PER */, int N, unsigned short* list) {
  int mine = 0;
#pragma unroll
  for (int k = 0; k < RT_PER; ++k) mine += flag[k] ? 1 : 0;
  int total;
  int rank = btc_block_excl_scan<RT_WAVES>(mine, &total);
#pragma unroll
  for (int k = 0; k < RT_PER; ++k) {
    const int i = threadIdx.x * RT_PER + k;
    if (i < N) {
      if (flag[k]) list[rank] = (unsigned short)i;
      else list[total + (i - rank)] = (unsigned short)i;
      rank += flag[k] ? 1 : 0;
    }
  }
  return total;
}

__device__ __forceinline__ int rt_draw(float u, int n) {
  const double f = floor((double)u * (double)n);
  const int top = (n > 1 ? n : 1) - 1;
  return f >= 0.0 ? (f < (double)top ? (int)f : top) : 0;
}

__global__ __launch_bounds__(RT_T) void roi_targets_kernel(const float* __restrict__ rois, const float* __restrict__ scores,
                                                           const int64_t* __restrict__ labels, const float* __restrict__ gts,
                                                           const float* __restrict__ uniforms, const int64_t* __restrict__ sampled_in,
                                                           const RtParams P, const RtOut O, int32_t* __restrict__ counters) {
  __shared__ float s_ov[RT_MAX];
  __shared__ int s_asg[RT_MAX];
  __shared__ float s_key[RT_MAX];
  __shared__ unsigned short s_fg[RT_MAX], s_hard[RT_MAX], s_easy[RT_MAX];
  const int b = blockIdx.x / P.tiles, tile = blockIdx.x % P.tiles;
  const int N = P.N, G = P.G, R = P.c.R;

  // ---- matching: lane `sub` of roi n takes boxes sub, sub + RT_LANES, ...
  {
    const int n = tile * RT_TILE + (int)threadIdx.x / RT_LANES, sub = threadIdx.x % RT_LANES;
    const bool valid = n < N;
    float best = -1.0f;
    int arg = 0x7fffffff;
    if (valid) {
      float a[7];
      const float* rp = rois + ((size_t)b * N + n) * 7;
#pragma unroll
      for (int k = 0; k < 7; ++k) a[k] = rp[k];
      const int64_t lab = P.c.by_class ? labels[(size_t)b * N + n] : 0;
      for (int g = sub; g < G; g += RT_LANES) {
        const float* bp = gts + ((size_t)b * G + g) * 8;
        float v = -1.0f;
        if (!P.c.by_class || (int64_t)bp[7] == lab) v = rt_iou3d(a, bp);
        if (rt_better(v, g, best, arg)) best = v, arg = g;
      }
    }
#pragma unroll
    for (int o = RT_LANES / 2; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int og = __shfl_xor(arg, o, 64);
      if (rt_better(ov, og, best, arg)) best = ov, arg = og;
    }
    if (valid && sub == 0) {
      if (P.c.by_class && best < 0.0f) best = 0.0f, arg = 0;   // no same-class box
      btc_st_agent(&O.max_overlaps[(size_t)b * N + n], best);
      btc_st_agent(&O.gt_assignment[(size_t)b * N + n], (int64_t)arg);
    }
  }
  if (!btc_last_arriver(&counters[b], P.tiles)) return;   // (the protocol: btc_common.h)

  // ---- this workgroup completed scene b
  for (int i = threadIdx.x; i < N; i += RT_T) {
    s_ov[i] = btc_ld_agent(&O.max_overlaps[(size_t)b * N + i]);
    const int64_t a = btc_ld_agent(&O.gt_assignment[(size_t)b * N + i]);
    s_asg[i] = a < 0 ? 0 : (a >= G ? G - 1 : (int)a);
  }
  __syncthreads();
  int n_fg = 0, n_hard = 0, n_easy = 0;
  if (sampled_in == nullptr) {
    const float* u0 = uniforms + (size_t)b * 4 * P.M;
    bool fg[RT_PER], hard[RT_PER], easy[RT_PER];
#pragma unroll
    for (int k = 0; k < RT_PER; ++k) {
      const int i = threadIdx.x * RT_PER + k;
      const float ov = i < N ? s_ov[i] : 0.0f;
      fg[k] = i < N && ov >= P.c.fg_thresh;
      easy[k] = i < N && ov < P.c.cls_bg_lo;
      hard[k] = i < N && ov < P.c.reg_fg && ov >= P.c.cls_bg_lo;
      if (i < N) s_key[i] = fg[k] ? u0[i] : 2.0f;
    }
    n_hard = rt_list(hard, N, s_hard);
    n_easy = rt_list(easy, N, s_easy);
    int mine = 0;
#pragma unroll
    for (int k = 0; k < RT_PER; ++k) mine += fg[k] ? 1 : 0;
    n_fg = btc_block_sum<RT_WAVES>(mine);
    __syncthreads();   // s_key is complete
    // the rank of a foreground member by (key, index): a background key of 2 is above every uniform.  Members are dealt out to the
    // threads one by one here (the scans above own RT_PER neighbours per thread, which would leave 3 of 4 threads idle at N = 256)
    for (int i = threadIdx.x; i < N; i += RT_T) {
      const float key = s_key[i];
      if (key == 2.0f) continue;
      int rank = 0;
      for (int j = 0; j < N; ++j) {
        const float kj = s_key[j];
        rank += (kj < key || (kj == key && j < i)) ? 1 : 0;
      }
      if (rank < N) s_fg[rank] = (unsigned short)i;   // (rank < n_fg always; a NaN key would rank 0)
    }
    __syncthreads();
  }
  const int n_bg = n_easy + n_hard;
  const int fg_this = n_bg > 0 ? (n_fg < P.c.fg_quota ? n_fg : P.c.fg_quota) : (n_fg > 0 ? R : 0);
  const int m = R - fg_this;
  int hard_num = 0;
  if (n_hard > 0 && n_easy > 0) {
    const double f = floor((double)m * P.c.hard_bg_ratio);
    hard_num = f < (double)n_hard ? (f > 0.0 ? (int)f : 0) : n_hard;
  } else if (n_hard > 0) {
    hard_num = m;
  }
  for (int j = threadIdx.x; j < R; j += RT_T) {
    const size_t oj = (size_t)b * R + j;
    int s;
    if (sampled_in != nullptr) {
      const int64_t v = sampled_in[oj];
      s = v < 0 ? 0 : (v >= N ? N - 1 : (int)v);
    } else {
      const float* u = uniforms + (size_t)b * 4 * P.M;
      if (j < fg_this) {
        // (a rank at or past n_fg is never asked for: fg_this <= n_fg with background, the draw stays below n_fg without)
        const int r = n_bg > 0 ? (j < N - 1 ? j : N - 1) : rt_draw(u[(size_t)P.M + j], n_fg);
        s = s_fg[r < n_fg ? r : 0];
      } else if (j - fg_this < hard_num) {
        s = s_hard[rt_draw(u[(size_t)2 * P.M + j], n_hard)];
      } else {
        s = s_easy[rt_draw(u[(size_t)3 * P.M + j], n_easy)];
      }
      s = s < N ? s : N - 1;
    }
    O.sampled[oj] = (int64_t)s;
    const size_t is = (size_t)b * N + s;
    float r[7], g[8];
#pragma unroll
    for (int k = 0; k < 7; ++k) r[k] = rois[is * 7 + k];
    const float* gp = gts + ((size_t)b * G + s_asg[s]) * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] = gp[k];
    const float iou = s_ov[s];
#pragma unroll
    for (int k = 0; k < 7; ++k) O.rois[oj * 7 + k] = r[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) O.gt_src[oj * 8 + k] = g[k];
    O.iou[oj] = iou;
    O.scores[oj] = scores[is];
    O.labels[oj] = labels[is];
    O.reg_valid[oj] = iou > P.c.reg_fg ? 1 : 0;
    if (P.c.score_type == BTC_ROI_SCORE_ROI_IOU) {
      const float d = iou - P.c.cls_bg;
      const float mid = d * P.inv_span;
      ((float*)O.cls)[oj] = iou > P.c.cls_fg ? 1.0f : (iou < P.c.cls_bg ? 0.0f : mid);
    } else {
      ((int64_t*)O.cls)[oj] = (iou > P.c.cls_bg && iou < P.c.cls_fg) ? -1 : (iou > P.c.cls_fg ? 1 : 0);
    }
    // the matched box in the roi's frame
    const float ry = rt_mod_two_pi(r[6]);
    const float lx = g[0] - r[0], ly = g[1] - r[1], lz = g[2] - r[2];
    const float lh = g[6] - ry;
    const float na = -ry;
    const float c = cosf(na), sn = sinf(na);
    const float xc = lx * c, ys = ly * sn, xs = lx * sn, yc = ly * c;
    float hd = rt_mod_two_pi(lh);
    if (hd > RT_HALF_PI && hd < RT_THREE_HALF_PI) hd = rt_mod_two_pi(hd + RT_PI);
    if (hd > RT_PI) hd = hd - RT_TWO_PI;
    hd = hd < -RT_HALF_PI ? -RT_HALF_PI : (hd > RT_HALF_PI ? RT_HALF_PI : hd);
    float* go = O.gt + oj * 8;
    go[0] = xc - ys, go[1] = xs + yc, go[2] = lz;
    go[3] = g[3], go[4] = g[4], go[5] = g[5];
    go[6] = hd, go[7] = g[7];
  }
  if (threadIdx.x == 0) __hip_atomic_store(&counters[b], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

bool rt_shape_ok(int B, int N) { return B >= 1 && N >= 1 && N <= BTC_ROI_TARGETS_MAX_N && (long long)B * N * 7 < (1ll << 31); }

}  // namespace

extern "C" size_t btc_roi_targets_ws_bytes(int B, int N) {
  if (!rt_shape_ok(B, N)) return 0;
  return btc_align((size_t)B * sizeof(int32_t));
}

extern "C" int btc_roi_targets(const float* rois, const float* roi_scores, const int64_t* roi_labels, const float* gt_boxes, const float* uniforms,
                               const int64_t* sampled_in, int B, int N, int G, const BtcRoiTargetsConfig* cfg, float* rois_out, float* gt_of_rois,
                               float* gt_of_rois_src, float* gt_iou_of_rois, float* roi_scores_out, int64_t* roi_labels_out,
                               int64_t* reg_valid_mask, void* rcnn_cls_labels, float* max_overlaps, int64_t* gt_assignment,
                               int64_t* sampled_inds, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(cfg, "btc_roi_targets: missing configuration block");
  BTC_CHECK_ARG(B >= 1 && G >= 1, "btc_roi_targets: need B >= 1 and G >= 1, got B %d G %d", B, G);
  BTC_CHECK_ARG(N >= 1 && N <= BTC_ROI_TARGETS_MAX_N, "btc_roi_targets: N %d outside [1, %d]", N, BTC_ROI_TARGETS_MAX_N);
  const int R = cfg->R;
  BTC_CHECK_ARG(R >= 1 && R <= BTC_ROI_TARGETS_MAX_R, "btc_roi_targets: R %d outside [1, %d]", R, BTC_ROI_TARGETS_MAX_R);
  BTC_CHECK_ARG(cfg->fg_quota >= 0 && cfg->fg_quota <= R, "btc_roi_targets: fg_quota %d outside [0, R = %d]", cfg->fg_quota, R);
  BTC_CHECK_ARG(cfg->score_type == BTC_ROI_SCORE_ROI_IOU || cfg->score_type == BTC_ROI_SCORE_CLS, "btc_roi_targets: unknown score_type %d",
                cfg->score_type);
  const int M = R > N ? R : N;
  const long long widest = (long long)B * 8 * (G > M ? G : M);   // above every element count: B * N * 7, B * R * 8, B * G * 8, B * 4 * M
  BTC_CHECK_ARG(widest < (1ll << 31), "btc_roi_targets: B * 8 * max(N, R, G) = %lld does not fit 31 bits", widest);
  BTC_CHECK_ARG(rois && roi_scores && roi_labels && gt_boxes, "btc_roi_targets: missing pointer (rois, roi_scores, roi_labels or gt_boxes)");
  BTC_CHECK_ARG((uniforms != nullptr) != (sampled_in != nullptr), "btc_roi_targets: exactly one of uniforms and sampled_in");
  BTC_CHECK_ARG(rois_out && gt_of_rois && gt_of_rois_src && gt_iou_of_rois && roi_scores_out && roi_labels_out && reg_valid_mask && rcnn_cls_labels &&
                    max_overlaps && gt_assignment && sampled_inds && ws,
                "btc_roi_targets: missing pointer (an output or ws)");
  const size_t need = btc_roi_targets_ws_bytes(B, N);
  BTC_CHECK_ARG(need != 0 && ws_bytes >= need, "btc_roi_targets: workspace too small");
  RtParams P;
  P.B = B, P.N = N, P.G = G, P.M = M, P.tiles = btc_cdiv(N, RT_TILE);
  P.c = *cfg;
  P.inv_span = 1.0f / cfg->cls_span;
  RtOut O;
  O.rois = rois_out, O.gt = gt_of_rois, O.gt_src = gt_of_rois_src, O.iou = gt_iou_of_rois, O.scores = roi_scores_out;
  O.labels = roi_labels_out, O.reg_valid = reg_valid_mask, O.cls = rcnn_cls_labels;
  O.max_overlaps = max_overlaps, O.gt_assignment = gt_assignment, O.sampled = sampled_inds;
  roi_targets_kernel<<<B * P.tiles, RT_T, 0, stream>>>(rois, roi_scores, roi_labels, gt_boxes, uniforms, sampled_in, P, O, (int32_t*)ws);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}
