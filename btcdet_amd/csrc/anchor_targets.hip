// The anchor head's targets and boxes for gfx950 (include/btcdet_hip_heads.h: btc_anchor_targets, btc_decode_anchor_boxes).
//
// btc_anchor_targets -- AxisAlignedTargetAssigner.assign_targets + ResidualCoder.encode_torch for a batch, every anchor-class
// configuration and every scene, three launches:
//   at_prepare  one workgroup per scene: the rows the scene owns (trailing padding trimmed) -> nrows[b]; the scene's per-box maxima to 0.
//   at_top      one thread per (scene, anchor), a workgroup inside one scene.  The scene's boxes are staged 64 at a time in LDS as
//               snapped footprints with area and configuration; per box one wave-level maximum of the overlaps' bit patterns, one LDS
//               maximum per wave with a hit, one global atomic maximum per (workgroup, box with a hit).  Overlaps are >= 0, so the
//               unsigned order of the bits is the float order and the maximum does not depend on the order of arrival.
//   at_assign   the same staging and THE SAME at_iou, so `iou == top` compares identical bits; a thread tracks its best box, decides
//               forced / background / positive and writes its label, its target row and its weight.
// btc_decode_anchor_boxes -- ResidualCoder.decode_torch + the direction-bin correction, one launch, one thread per (scene, anchor).
// The configuration tables travel by value in the kernel arguments (AtTables, < 1 KB); nothing is uploaded.
// Every index is formed from a, b, j below A, B, n_b <= M; the class id read from a box row is checked before it indexes the table.
#include "btc_common.h"

#include "../../include/btcdet_hip_heads.h"

namespace {

constexpr int AT_T = 256;
constexpr int AT_WAVES = AT_T / 64;
constexpr int AT_CHUNK = 64;   // boxes staged per pass
constexpr float AT_PI = 3.14159265358979323846f;
constexpr float AT_INV_PI = 1.0f / AT_PI;             // the float32 reciprocal of the float32 pi
constexpr float AT_QUARTER_PI = (float)(3.14159265358979323846 / 4.0);

struct AtTables {
  int32_t slots, ncfg, num_class;
  int32_t slot_cfg[BTC_HEADS_MAX_SLOTS];
  int32_t class_cfg[BTC_HEADS_MAX_CLASSES];
  float matched[BTC_HEADS_MAX_CFGS], unmatched[BTC_HEADS_MAX_CFGS];
};

struct AtFoot {
  float x0, y0, x1, y1, area;
};

// the header's limit_period: val / period in the form of torch's device backend (a multiplication by the reciprocal)
__device__ __forceinline__ float at_limit_period(float v, float offset, float period, float inv_period) {
  const float q = v * inv_period;
  const float f = floorf(q + offset);
  const float m = f * period;
  return v - m;
}

__device__ __forceinline__ AtFoot at_foot(const float* __restrict__ b) {
  const float lp = at_limit_period(b[6], 0.5f, AT_PI, AT_INV_PI);
  const bool snapped = fabsf(lp) < AT_QUARTER_PI;
  const float wx = snapped ? b[3] : b[4], wy = snapped ? b[4] : b[3];
  const float hx = wx / 2.0f, hy = wy / 2.0f;
  AtFoot f;
  f.x0 = b[0] - hx, f.y0 = b[1] - hy, f.x1 = b[0] + hx, f.y1 = b[1] + hy;
  const float ex = f.x1 - f.x0, ey = f.y1 - f.y0;
  f.area = ex * ey;
  return f;
}

// the ONE statement of the overlap: at_top and at_assign both call it, so their results are the same bits
__device__ __forceinline__ float at_iou(const AtFoot& a, const AtFoot& g) {
  const float w = fmaxf(fminf(a.x1, g.x1) - fmaxf(a.x0, g.x0), 0.0f);
  const float h = fmaxf(fminf(a.y1, g.y1) - fmaxf(a.y0, g.y0), 0.0f);
  const float inter = w * h;
  const float sum = a.area + g.area;
  const float uni = sum - inter;
  return inter / fmaxf(uni, 1e-6f);
}

// the bit pattern a maximum is taken over: 0 for an overlap of zero (either sign)
__device__ __forceinline__ unsigned at_bits(float iou) { return iou > 0.0f ? __float_as_uint(iou) : 0u; }

__device__ __forceinline__ int at_class_cfg(const AtTables& t, float cls) {
  const int c = (int)cls;
  return (c >= 0 && c <= t.num_class) ? t.class_cfg[c] : -1;
}

__global__ __launch_bounds__(AT_T) void at_prepare(const float* __restrict__ gt, int M, int32_t* __restrict__ nrows, unsigned* __restrict__ top) {
  __shared__ int s_last[AT_WAVES];
  const int b = blockIdx.x;
  int last = -1;
  for (int j = threadIdx.x; j < M; j += AT_T) {
    const float* r = gt + ((size_t)b * M + j) * 8;
    const float s = (((((r[0] + r[1]) + r[2]) + r[3]) + r[4]) + r[5]) + r[6];
    if (s != 0.0f) last = j;   // j ascends per thread
    top[(size_t)b * M + j] = 0u;
  }
  last = btc_wave_all_max(last);
  if ((threadIdx.x & 63) == 0) s_last[threadIdx.x >> 6] = last;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < AT_WAVES; ++w) last = max(last, s_last[w]);
    nrows[b] = M == 0 ? 0 : max(1, last + 1);
  }
}

// stage rows [c0, c0 + nb) of scene b: thread k < nb takes row c0 + k
__device__ __forceinline__ void at_stage(const float* __restrict__ gt, int M, int b, int c0, int nb, const AtTables& tab, AtFoot* s_foot, int* s_cfg) {
  if ((int)threadIdx.x < nb) {
    const float* r = gt + ((size_t)b * M + c0 + threadIdx.x) * 8;
    s_foot[threadIdx.x] = at_foot(r);
    s_cfg[threadIdx.x] = at_class_cfg(tab, r[7]);
  }
}

__global__ __launch_bounds__(AT_T) void at_top(const float* __restrict__ anchors, int A, int tiles, const AtTables tab, const float* __restrict__ gt,
                                               int M, const int32_t* __restrict__ nrows, unsigned* __restrict__ top) {
  __shared__ AtFoot s_foot[AT_CHUNK];
  __shared__ int s_cfg[AT_CHUNK];
  __shared__ unsigned s_top[AT_CHUNK];
  const int b = blockIdx.x / tiles;
  const int a = (blockIdx.x % tiles) * AT_T + threadIdx.x;
  const int n = min(nrows[b], M);
  int mine = -2;   // no box has it
  AtFoot fa = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (a < A) {
    mine = tab.slot_cfg[a % tab.slots];
    fa = at_foot(anchors + (size_t)a * 7);
  }
  for (int c0 = 0; c0 < n; c0 += AT_CHUNK) {
    const int nb = min(AT_CHUNK, n - c0);
    __syncthreads();   // the previous chunk's LDS has been read
    at_stage(gt, M, b, c0, nb, tab, s_foot, s_cfg);
    if ((int)threadIdx.x < AT_CHUNK) s_top[threadIdx.x] = 0u;
    __syncthreads();
    for (int k = 0; k < nb; ++k) {
      const int cfg = s_cfg[k];
      if (cfg < 0) continue;   // the same in every thread
      unsigned bits = cfg == mine ? at_bits(at_iou(fa, s_foot[k])) : 0u;
      if (__ballot(bits != 0u) == 0ull) continue;   // the same in every lane of the wave
      bits = btc_wave_all_max(bits);
      if ((threadIdx.x & 63) == 0) atomicMax(s_top + k, bits);
    }
    __syncthreads();
    if ((int)threadIdx.x < nb && s_top[threadIdx.x] != 0u) atomicMax(top + (size_t)b * M + c0 + threadIdx.x, s_top[threadIdx.x]);
  }
}

__global__ __launch_bounds__(AT_T) void at_assign(const float* __restrict__ anchors, int A, int tiles, const AtTables tab, const float* __restrict__ gt,
                                                  int M, const int32_t* __restrict__ nrows, const unsigned* __restrict__ top,
                                                  int32_t* __restrict__ labels, float* __restrict__ targets, float* __restrict__ weights) {
  __shared__ AtFoot s_foot[AT_CHUNK];
  __shared__ int s_cfg[AT_CHUNK];
  __shared__ unsigned s_top[AT_CHUNK];
  const int b = blockIdx.x / tiles;
  const int a = (blockIdx.x % tiles) * AT_T + threadIdx.x;
  const int n = min(nrows[b], M);
  int mine = -2;
  AtFoot fa = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (a < A) {
    mine = tab.slot_cfg[a % tab.slots];
    fa = at_foot(anchors + (size_t)a * 7);
  }
  float best = 0.0f;
  int best_j = -1;
  bool forced = false;
  for (int c0 = 0; c0 < n; c0 += AT_CHUNK) {
    const int nb = min(AT_CHUNK, n - c0);
    __syncthreads();
    at_stage(gt, M, b, c0, nb, tab, s_foot, s_cfg);
    if ((int)threadIdx.x < nb) s_top[threadIdx.x] = top[(size_t)b * M + c0 + threadIdx.x];
    __syncthreads();
    for (int k = 0; k < nb; ++k) {
      if (s_cfg[k] != mine) continue;
      const float v = at_iou(fa, s_foot[k]);
      if (best_j < 0 || v > best) best = v, best_j = c0 + k;   // the smallest index among equal overlaps
      const unsigned t = s_top[k];
      forced = forced || (t != 0u && at_bits(v) == t);
    }
  }
  if (a >= A) return;
  const float* ar = anchors + (size_t)a * 7;
  int label = 0;
  const float* g = nullptr;
  if (best_j >= 0) {
    g = gt + ((size_t)b * M + best_j) * 8;
    const int cls = (int)g[7];
    if (forced) label = cls;
    else if (best < tab.unmatched[mine]) label = 0;
    else if (best >= tab.matched[mine]) label = cls;
    else label = -1;
  }
  const size_t i = (size_t)b * A + a;
  float t[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (label > 0) {
    const float dxa = fmaxf(ar[3], 1e-5f), dya = fmaxf(ar[4], 1e-5f), dza = fmaxf(ar[5], 1e-5f);
    const float dxg = fmaxf(g[3], 1e-5f), dyg = fmaxf(g[4], 1e-5f), dzg = fmaxf(g[5], 1e-5f);
    const float xx = dxa * dxa, yy = dya * dya;
    const float diag = sqrtf(xx + yy);
    t[0] = (g[0] - ar[0]) / diag;
    t[1] = (g[1] - ar[1]) / diag;
    t[2] = (g[2] - ar[2]) / dza;
    t[3] = logf(dxg / dxa);
    t[4] = logf(dyg / dya);
    t[5] = logf(dzg / dza);
    t[6] = g[6] - ar[6];
  }
  labels[i] = label;
  weights[i] = label > 0 ? 1.0f : 0.0f;
#pragma unroll
  for (int k = 0; k < 7; ++k) targets[i * 7 + k] = t[k];
}

__global__ __launch_bounds__(AT_T) void at_decode(const float* __restrict__ preds, const float* __restrict__ anchors, const float* __restrict__ dirs,
                                                  long long total, int A, int bins, float off, float lim, float period, float inv_period,
                                                  float* __restrict__ boxes) {
  const long long i = (long long)blockIdx.x * AT_T + threadIdx.x;
  if (i >= total) return;
  const float* t = preds + (size_t)i * 7;
  const float* a = anchors + (size_t)(i % A) * 7;
  const float xx = a[3] * a[3], yy = a[4] * a[4];
  const float diag = sqrtf(xx + yy);
  float o[7];
  const float px = t[0] * diag, py = t[1] * diag, pz = t[2] * a[5];
  o[0] = px + a[0], o[1] = py + a[1], o[2] = pz + a[2];
  o[3] = expf(t[3]) * a[3], o[4] = expf(t[4]) * a[4], o[5] = expf(t[5]) * a[5];
  float rot = t[6] + a[6];
  if (dirs != nullptr) {
    const float* d = dirs + (size_t)i * bins;
    int k = 0;
    float top = d[0];
    for (int j = 1; j < bins; ++j) {
      const float v = d[j];
      if (v > top) top = v, k = j;
    }
    const float lp = at_limit_period(rot - off, lim, period, inv_period);
    const float base = lp + off;
    const float turn = period * (float)k;
    rot = base + turn;
  }
  o[6] = rot;
#pragma unroll
  for (int k = 0; k < 7; ++k) boxes[(size_t)i * 7 + k] = o[k];
}

}  // namespace

extern "C" size_t btc_anchor_targets_ws_bytes(int B, int M) {
  if (B < 1 || M < 0 || (long long)B * M * 8 >= (1ll << 31)) return 0;
  return btc_align((size_t)B * sizeof(int32_t)) + btc_align((size_t)B * (size_t)M * sizeof(unsigned));
}

extern "C" int btc_anchor_targets(const float* anchors, int A, int slots, const int32_t* h_slot_cfg, int ncfg, const float* h_matched,
                                  const float* h_unmatched, const int32_t* h_class_cfg, int num_class, const float* gt, int B, int M,
                                  int32_t* labels, float* targets, float* weights, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(B >= 1, "btc_anchor_targets: need B >= 1, got %d", B);
  BTC_CHECK_ARG(A >= 0 && M >= 0, "btc_anchor_targets: negative count (A %d, M %d)", A, M);
  BTC_CHECK_ARG(slots >= 1 && slots <= BTC_HEADS_MAX_SLOTS, "btc_anchor_targets: slots %d outside [1, %d]", slots, BTC_HEADS_MAX_SLOTS);
  BTC_CHECK_ARG(A % slots == 0, "btc_anchor_targets: A %d is not a multiple of slots %d", A, slots);
  BTC_CHECK_ARG(ncfg >= 1 && ncfg <= BTC_HEADS_MAX_CFGS, "btc_anchor_targets: ncfg %d outside [1, %d]", ncfg, BTC_HEADS_MAX_CFGS);
  BTC_CHECK_ARG(num_class >= 0 && num_class < BTC_HEADS_MAX_CLASSES, "btc_anchor_targets: num_class %d outside [0, %d)", num_class, BTC_HEADS_MAX_CLASSES);
  BTC_CHECK_ARG(h_slot_cfg && h_matched && h_unmatched && h_class_cfg && ws,
                "btc_anchor_targets: missing pointer (h_slot_cfg, h_matched, h_unmatched, h_class_cfg or ws)");
  BTC_CHECK_ARG((anchors && labels && targets && weights) || A == 0, "btc_anchor_targets: missing pointer (anchors, labels, targets or weights)");
  BTC_CHECK_ARG(gt || M == 0 || A == 0, "btc_anchor_targets: missing pointer (gt)");
  const long long widest = (long long)B * (A > M ? A : M) * 8;
  BTC_CHECK_ARG(widest < (1ll << 31), "btc_anchor_targets: B * max(A, M) * 8 = %lld does not fit 31 bits", widest);
  AtTables tab;
  tab.slots = slots, tab.ncfg = ncfg, tab.num_class = num_class;
  for (int s = 0; s < BTC_HEADS_MAX_SLOTS; ++s) {
    tab.slot_cfg[s] = s < slots ? h_slot_cfg[s] : 0;
    BTC_CHECK_ARG(tab.slot_cfg[s] >= 0 && tab.slot_cfg[s] < ncfg, "btc_anchor_targets: h_slot_cfg[%d] = %d outside [0, %d)", s, tab.slot_cfg[s], ncfg);
  }
  for (int c = 0; c < BTC_HEADS_MAX_CLASSES; ++c) {
    tab.class_cfg[c] = c <= num_class ? h_class_cfg[c] : -1;
    BTC_CHECK_ARG(tab.class_cfg[c] >= -1 && tab.class_cfg[c] < ncfg, "btc_anchor_targets: h_class_cfg[%d] = %d outside [-1, %d)", c, tab.class_cfg[c], ncfg);
  }
  for (int c = 0; c < BTC_HEADS_MAX_CFGS; ++c) tab.matched[c] = c < ncfg ? h_matched[c] : 0.f, tab.unmatched[c] = c < ncfg ? h_unmatched[c] : 0.f;
  const size_t need = btc_anchor_targets_ws_bytes(B, M);
  BTC_CHECK_ARG(need != 0 && ws_bytes >= need, "btc_anchor_targets: workspace too small");
  if (A == 0) return BTC_OK;
  BtcCarver c(ws);
  int32_t* nrows = c.take<int32_t>(B);
  unsigned* top = c.take<unsigned>((size_t)B * M);
  const int tiles = btc_cdiv(A, AT_T);   // B * tiles <= B * A < 2^28
  at_prepare<<<B, AT_T, 0, stream>>>(gt, M, nrows, top);
  BTC_LAUNCH_CHECK();
  if (M > 0) {
    at_top<<<B * tiles, AT_T, 0, stream>>>(anchors, A, tiles, tab, gt, M, nrows, top);
    BTC_LAUNCH_CHECK();
  }
  at_assign<<<B * tiles, AT_T, 0, stream>>>(anchors, A, tiles, tab, gt, M, nrows, top, labels, targets, weights);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}

extern "C" int btc_decode_anchor_boxes(const float* box_preds, const float* anchors, const float* dir_cls_preds, int B, int A, int bins,
                                       float dir_offset, float dir_limit_offset, float* boxes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(B >= 1, "btc_decode_anchor_boxes: need B >= 1, got %d", B);
  BTC_CHECK_ARG(A >= 0, "btc_decode_anchor_boxes: negative count (A %d)", A);
  const long long total = (long long)B * A;
  BTC_CHECK_ARG(total * 8 < (1ll << 31), "btc_decode_anchor_boxes: B * A * 8 = %lld does not fit 31 bits", total * 8);
  BTC_CHECK_ARG((box_preds && anchors && boxes) || A == 0, "btc_decode_anchor_boxes: missing pointer (box_preds, anchors or boxes)");
  BTC_CHECK_ARG(dir_cls_preds == nullptr || bins >= 1, "btc_decode_anchor_boxes: need bins >= 1 with dir_cls_preds, got %d", bins);
  BTC_CHECK_ARG(dir_cls_preds == nullptr || total * bins < (1ll << 31), "btc_decode_anchor_boxes: B * A * bins does not fit 31 bits");
  if (A == 0) return BTC_OK;
  float period = 0.f, inv_period = 0.f;
  if (dir_cls_preds != nullptr) {
    period = (float)(2.0 * 3.141592653589793 / (double)bins);
    inv_period = 1.0f / period;
  }
  at_decode<<<btc_cdiv(total, AT_T), AT_T, 0, stream>>>(box_preds, anchors, dir_cls_preds, total, A, bins, dir_offset, dir_limit_offset, period,
                                                         inv_period, boxes);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}
