// The ROI head's loss, fused (include/btcdet_hip_roi_loss.h: forward one launch, backward one launch).
//
// Replaces ConvHead.get_loss -> rcnn_cls_loss / rcnn_reg_loss of btcdet_amd/roi_targets.py (the reference's RoIHeadTemplate.get_loss,
// btcdet/models/roi_heads/roi_head_template.py:134-229, with ResidualCoder.encode_torch / decode_torch of utils/box_coder_utils.py,
// the smooth L1 of utils/loss_utils.py:174-236 and get_corner_loss_lidar of :309-332): there a sigmoid and a
// binary cross-entropy, two clones with in-place edits, an encode, a decode, a rotation, three corner expansions, two norms, a min, two
// smooth-L1s and masked sums, plus an autograd twin of each -- a few hundred launches over 256 rois.
//   cls    = cls_weight    / n_valid * sum_{valid}      bce(sigmoid(x), t)                    n_valid = max(#{label >= 0}, 1)
//   reg    = reg_weight    / n_fg    * sum_{fg, k}      smoothL1_{1/9}(r_k - encode(gt, roi)_k)     n_fg = max(#{mask > 0}, 1)
//   corner = corner_weight / n_fg    * sum_{fg} 1/8 sum_j smoothL1_1(min(|P_j - Q_j|, |P_j - Q'_j|))
// A roi is read as far as its label and mask ask: the class logit unless ignored, everything else only when foreground.  RL_LANES lanes
// share a roi (1: one thread walks the eight corners; 8: a lane per corner).  A workgroup stores five doubles (three sums, two counts);
// the last workgroup to arrive adds them in a fixed order.  Every index is formed from i < N, k < 7 and gt_width.
#include "btc_common.h"

#include "../../include/btcdet_hip_roi_loss.h"

namespace {

constexpr int RL_T = BTC_ROI_LOSS_THREADS;
constexpr int RL_LANES = BTC_ROI_LOSS_LANES;
constexpr int RL_TILE = BTC_ROI_LOSS_TILE;
constexpr int RL_WAVES = RL_T / 64;
constexpr int RL_Q = 5;   // per workgroup: class sum, regression sum, corner sum, valid count, foreground count
constexpr float RL_BETA = (float)(1.0 / 9.0);
constexpr float RL_HALF_BETA = 0.5f * RL_BETA;   // exact
constexpr float RL_PI = (float)3.14159265358979323846;
static_assert(RL_LANES == 1 || RL_LANES == 8, "one thread per roi, or one lane per corner");

struct RlArgs {
  const float *cls, *reg, *rois, *gt, *src;
  const int64_t* mask;
  const void* labels;
  int gt_width, kind, N, with_corner;
  float w[3];
};

// max(x, c) that hands a NaN on, as torch's clamp_min does
__device__ __forceinline__ float rl_clamp_min(float x, float c) { return x < c ? c : x; }

__device__ __forceinline__ float rl_label(const RlArgs& A, int i) {
  return A.kind == BTC_ROI_SCORE_CLS ? (float)((const int64_t*)A.labels)[i] : ((const float*)A.labels)[i];
}

// binary cross-entropy on a float32 sigmoid: the term, and d term / dx
__device__ __forceinline__ void rl_cls(float x, float t, float* term, float* d) {
  const float e = expf(-fabsf(x));
  const float r = 1.0f / (1.0f + e);
  const float er = e * r;
  const float p = x >= 0.0f ? r : er;
  const float om = 1.0f - p;
  const float l1 = fmaxf(logf(om), -100.0f), l0 = fmaxf(logf(p), -100.0f);
  const float a = (t - 1.0f) * l1, b = t * l0;
  *term = a - b;
  const float pq = om * p;
  const float q = (p - t) / fmaxf(pq, 1e-12f);
  *d = q * pq;
}

// the encoded target of a foreground roi against the roi with its centre and heading zeroed
__device__ __forceinline__ void rl_encode(const float* __restrict__ roi, const float* __restrict__ gt, float* v) {
  const float a3 = rl_clamp_min(roi[3], 1e-5f), a4 = rl_clamp_min(roi[4], 1e-5f), a5 = rl_clamp_min(roi[5], 1e-5f);
  const float g3 = rl_clamp_min(gt[3], 1e-5f), g4 = rl_clamp_min(gt[4], 1e-5f), g5 = rl_clamp_min(gt[5], 1e-5f);
  const float q3 = a3 * a3, q4 = a4 * a4;
  const float diag = sqrtf(q3 + q4);
  v[0] = gt[0] / diag, v[1] = gt[1] / diag, v[2] = gt[2] / a5;
  v[3] = logf(g3 / a3), v[4] = logf(g4 / a4), v[5] = logf(g5 / a5);
  v[6] = gt[6];
}

__device__ __forceinline__ float rl_smooth_l1(float d) {
  const float n = fabsf(d);
  const float nn = n * n;
  return n < RL_BETA ? 0.5f * nn / RL_BETA : n - RL_HALF_BETA;
}

// the decoded box of a foreground roi (UNCLAMPED roi dims) and what its corners need
struct RlBox {
  float dg, s5, l[3], c, s, cx, cy, cz, ch, sh;
};

__device__ __forceinline__ RlBox rl_decode(const float* __restrict__ r, const float* __restrict__ roi) {
  RlBox b;
  const float q3 = roi[3] * roi[3], q4 = roi[4] * roi[4];
  b.dg = sqrtf(q3 + q4), b.s5 = roi[5];
  const float bx = r[0] * b.dg, by = r[1] * b.dg, bz = r[2] * b.s5;
#pragma unroll
  for (int k = 0; k < 3; ++k) b.l[k] = expf(r[3 + k]) * roi[3 + k];
  const float h = r[6] + roi[6];
  b.c = cosf(roi[6]), b.s = sinf(roi[6]);
  const float xc = bx * b.c, ys = by * b.s, xs = bx * b.s, yc = by * b.c;
  b.cx = (xc - ys) + roi[0], b.cy = (xs + yc) + roi[1], b.cz = bz + roi[2];
  b.ch = cosf(h), b.sh = sinf(h);
  return b;
}

// the matched box and its half-turn twin
struct RlGt {
  float w[6], cg[2], sg[2];
};

__device__ __forceinline__ RlGt rl_gt(const float* __restrict__ src) {
  RlGt g;
#pragma unroll
  for (int k = 0; k < 6; ++k) g.w[k] = src[k];
  const float hf = src[6] + RL_PI;
  g.cg[0] = cosf(src[6]), g.sg[0] = sinf(src[6]);
  g.cg[1] = cosf(hf), g.sg[1] = sinf(hf);
  return g;
}

// corner j of the prediction against the same corner of either twin: m = the smaller distance, D = the difference to that twin
// (the unflipped one on a tie), R = the corner's rotated offset
struct RlCorner {
  float m, D[3], R[2], hx, hy, hz;
};

__device__ __forceinline__ RlCorner rl_corner(const RlBox& b, const RlGt& g, int j) {
  RlCorner o;
  o.hx = (j & 2) ? -0.5f : 0.5f, o.hy = ((j + 1) & 2) ? -0.5f : 0.5f, o.hz = (j & 4) ? 0.5f : -0.5f;
  const float x = b.l[0] * o.hx, y = b.l[1] * o.hy, z = b.l[2] * o.hz;
  const float xc = x * b.ch, ys = y * b.sh, xs = x * b.sh, yc = y * b.ch;
  o.R[0] = xc - ys, o.R[1] = xs + yc;
  const float P[3] = {o.R[0] + b.cx, o.R[1] + b.cy, z + b.cz};
  const float gx = g.w[3] * o.hx, gy = g.w[4] * o.hy, gz = g.w[5] * o.hz;
  float dist[2], D[2][3];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const float ac = gx * g.cg[f], bs = gy * g.sg[f], as = gx * g.sg[f], bc = gy * g.cg[f];
    const float Q[3] = {(ac - bs) + g.w[0], (as + bc) + g.w[1], gz + g.w[2]};
#pragma unroll
    for (int a = 0; a < 3; ++a) D[f][a] = P[a] - Q[a];
    const float xx = D[f][0] * D[f][0], yy = D[f][1] * D[f][1], zz = D[f][2] * D[f][2];
    dist[f] = sqrtf((xx + yy) + zz);
  }
  const bool flip = dist[1] < dist[0];
  o.m = flip ? dist[1] : dist[0];
#pragma unroll
  for (int a = 0; a < 3; ++a) o.D[a] = flip ? D[1][a] : D[0][a];
  return o;
}

__device__ __forceinline__ float rl_corner_term(float m) {
  const float hm = 0.5f * m;
  return 0.125f * (m < 1.0f ? hm * m : m - 0.5f);
}

// the seven chain components of one corner (header: u_j)
__device__ __forceinline__ void rl_corner_grad(const RlBox& b, const RlCorner& o, float* u) {
  float G[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) G[a] = o.m < 1.0f ? o.D[a] : o.D[a] / o.m;
  const float gxc = G[0] * b.ch, gys = G[1] * b.sh, gyc = G[1] * b.ch, gxs = G[0] * b.sh;
  const float qx = gxc + gys, qy = gyc - gxs;
  u[0] = G[0], u[1] = G[1], u[2] = G[2];
  u[3] = qx * o.hx, u[4] = qy * o.hy, u[5] = G[2] * o.hz;
  const float yr = G[1] * o.R[0], xr = G[0] * o.R[1];
  u[6] = yr - xr;
}

// partial[g * RL_Q + q]: q = 0 class, 1 regression, 2 corner, 3 valid rois, 4 foreground rois
__global__ __launch_bounds__(RL_T) void roi_loss_fwd(const RlArgs A, double* __restrict__ partial, int32_t* __restrict__ counter,
                                                     float* __restrict__ out, float* __restrict__ norms) {
  __shared__ double s_red[RL_WAVES][RL_Q];
  __shared__ double s_fin[32][RL_Q];
  const int sub = threadIdx.x % RL_LANES, slot = threadIdx.x / RL_LANES;
  double acc[RL_Q] = {0, 0, 0, 0, 0};
  for (int i = blockIdx.x * RL_TILE + slot; i < A.N; i += (int)gridDim.x * RL_TILE) {
    if (sub == 0) {
      const float lab = rl_label(A, i);
      if (lab >= 0.0f) {
        float term, d;
        rl_cls(A.cls[i], fmaxf(lab, 0.0f), &term, &d);
        acc[0] += (double)term, acc[3] += 1.0;
      }
    }
    if (A.mask[i] <= 0) continue;
    const float* r = A.reg + (size_t)i * 7;
    const float* roi = A.rois + (size_t)i * 7;
    if (sub == 0) {
      acc[4] += 1.0;
      float v[7];
      rl_encode(roi, A.gt + (size_t)i * A.gt_width, v);
#pragma unroll
      for (int k = 0; k < 7; ++k)
        if (!isnan(v[k])) acc[1] += (double)rl_smooth_l1(r[k] - v[k]);
    }
    if (A.with_corner) {
      const RlBox b = rl_decode(r, roi);
      const RlGt g = rl_gt(A.src + (size_t)i * A.gt_width);
#pragma unroll
      for (int j = sub; j < 8; j += RL_LANES) acc[2] += (double)rl_corner_term(rl_corner(b, g, j).m);
    }
  }
#pragma unroll
  for (int q = 0; q < RL_Q; ++q) {
    acc[q] = btc_wave_sum(acc[q]);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6][q] = acc[q];
  }
  __syncthreads();
  if (threadIdx.x < RL_Q) {
    const double v = (s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + (s_red[2][threadIdx.x] + s_red[3][threadIdx.x]);
    btc_st_agent(&partial[(size_t)blockIdx.x * RL_Q + threadIdx.x], v);
  }
  if (!btc_last_arriver(counter, (int)gridDim.x)) return;   // (the protocol: btc_common.h)
  // the last workgroup: thread (g0, q) = (tid / 8, tid % 8) adds quantity q over workgroups g0, g0 + 32, ... ascending; threads 0..4 then
  // add the 32 rows of their quantity ascending
  const int q = threadIdx.x & 7, g0 = threadIdx.x >> 3;
  if (q < RL_Q) {
    double v = 0.0;
    for (int g = g0; g < (int)gridDim.x; g += 32) v += btc_ld_agent(&partial[(size_t)g * RL_Q + q]);
    s_fin[g0][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < RL_Q) {
    double v = 0.0;
    for (int g = 0; g < 32; ++g) v += s_fin[g][threadIdx.x];
    s_red[0][threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double nv = s_red[0][3] > 1.0 ? s_red[0][3] : 1.0, nf = s_red[0][4] > 1.0 ? s_red[0][4] : 1.0;
    const double iv = 1.0 / nv, inf_ = 1.0 / nf;
    const float o0 = (float)(s_red[0][0] * iv * (double)A.w[0]);
    const float o1 = (float)(s_red[0][1] * inf_ * (double)A.w[1]);
    const float o2 = A.with_corner ? (float)(s_red[0][2] * inf_ * (double)A.w[2]) : 0.0f;
    const float o3 = o1 + o2;
    out[0] = o0, out[1] = o1, out[2] = o2, out[3] = o3;
    out[4] = o0 + o3;   // (the fp32 sums `cls + (reg + corner)` the caller would otherwise make with two more launches)
    norms[0] = (float)iv, norms[1] = (float)inf_;
    __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// every element of d_cls / d_reg is written: the caller allocates them uninitialised
__global__ __launch_bounds__(RL_T) void roi_loss_bwd(const RlArgs A, const float* __restrict__ norms, const float* __restrict__ g,
                                                     float* __restrict__ d_cls, float* __restrict__ d_reg) {
  const long long tid = (long long)blockIdx.x * RL_T + threadIdx.x;
  const long long il = tid / RL_LANES;
  const int sub = (int)(tid % RL_LANES);
  if (il >= A.N) return;   // (the lanes of a roi leave together)
  const int i = (int)il;
  const float gu = g[0];
  const float gv = gu * norms[0], gf = gu * norms[1];
  if (sub == 0) {
    const float lab = rl_label(A, i);
    float dv = 0.0f;
    if (lab >= 0.0f) {
      float term, d;
      rl_cls(A.cls[i], fmaxf(lab, 0.0f), &term, &d);
      dv = (gv * A.w[0]) * d;
    }
    d_cls[i] = dv;
  }
  float* dr = d_reg + (size_t)i * 7;
  if (A.mask[i] <= 0) {
    if (sub == 0) {
#pragma unroll
      for (int k = 0; k < 7; ++k) dr[k] = 0.0f;
    }
    return;
  }
  const float* r = A.reg + (size_t)i * 7;
  const float* roi = A.rois + (size_t)i * 7;
  float res[7] = {0, 0, 0, 0, 0, 0, 0};
  if (sub == 0) {
    const float s1 = gf * A.w[1];
    float v[7];
    rl_encode(roi, A.gt + (size_t)i * A.gt_width, v);
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const float d = r[k] - v[k];
      const float gr = fabsf(d) < RL_BETA ? d / RL_BETA : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));
      res[k] = isnan(v[k]) ? 0.0f : s1 * gr;
    }
  }
  if (A.with_corner) {
    const RlBox b = rl_decode(r, roi);
    const RlGt gt = rl_gt(A.src + (size_t)i * A.gt_width);
    float U[7];
    if (RL_LANES == 1) {
      float u[8][7];
#pragma unroll
      for (int j = 0; j < 8; ++j) rl_corner_grad(b, rl_corner(b, gt, j), u[j]);
#pragma unroll
      for (int a = 0; a < 7; ++a) U[a] = ((u[0][a] + u[4][a]) + (u[2][a] + u[6][a])) + ((u[1][a] + u[5][a]) + (u[3][a] + u[7][a]));
    } else {
      rl_corner_grad(b, rl_corner(b, gt, sub), U);
#pragma unroll
      for (int a = 0; a < 7; ++a) {
        // (a three-step ladder inside the roi's eight lanes; a + b == b + a, so every lane holds the header's tree)
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) U[a] = U[a] + __shfl_xor(U[a], o, 64);
      }
    }
    if (sub == 0) {
      const float s2 = (gf * A.w[2]) * 0.125f;
      const float ex = U[0] * b.c + U[1] * b.s, ey = U[1] * b.c - U[0] * b.s;
      float cn[7];
      cn[0] = s2 * (ex * b.dg), cn[1] = s2 * (ey * b.dg), cn[2] = s2 * (U[2] * b.s5);
#pragma unroll
      for (int k = 0; k < 3; ++k) cn[3 + k] = s2 * (U[3 + k] * b.l[k]);
      cn[6] = s2 * U[6];
#pragma unroll
      for (int k = 0; k < 7; ++k) res[k] = res[k] + cn[k];
    }
  }
  if (sub == 0) {
#pragma unroll
    for (int k = 0; k < 7; ++k) dr[k] = res[k];
  }
}

int rl_tiles(int N) {
  int t = btc_cdiv(N, RL_TILE);
  return t < 1 ? 1 : (t > BTC_ROI_LOSS_MAX_TILES ? BTC_ROI_LOSS_MAX_TILES : t);
}

// the checks both entry points share
int rl_check(const char* who, const float* cls, const float* reg, const float* rois, const float* gt, const float* src, int gt_width,
             const int64_t* mask, const void* labels, int kind, int N) {
  BTC_CHECK_ARG(N >= 0, "%s: negative count (N %d)", who, N);
  BTC_CHECK_ARG((long long)N * 8 < (1ll << 31), "%s: N * 8 = %lld does not fit 31 bits", who, (long long)N * 8);
  BTC_CHECK_ARG(gt_width >= 7, "%s: gt_width %d below 7", who, gt_width);
  BTC_CHECK_ARG(kind == BTC_ROI_SCORE_ROI_IOU || kind == BTC_ROI_SCORE_CLS, "%s: unknown label_kind %d", who, kind);
  BTC_CHECK_ARG(N == 0 || (cls && reg && rois && gt && src && mask && labels),
                "%s: missing pointer (rcnn_cls, rcnn_reg, rois, gt_of_rois, gt_of_rois_src, reg_valid_mask or cls_labels)", who);
  return BTC_OK;
}

RlArgs rl_args(const float* cls, const float* reg, const float* rois, const float* gt, const float* src, int gt_width, const int64_t* mask,
               const void* labels, int kind, int N, int with_corner, float w0, float w1, float w2) {
  RlArgs A;
  A.cls = cls, A.reg = reg, A.rois = rois, A.gt = gt, A.src = src, A.mask = mask, A.labels = labels;
  A.gt_width = gt_width, A.kind = kind, A.N = N, A.with_corner = with_corner != 0;
  A.w[0] = w0, A.w[1] = w1, A.w[2] = w2;
  return A;
}

}  // namespace

extern "C" size_t btc_roi_loss_ws_bytes(int N) {
  if (N < 0 || (long long)N * 8 >= (1ll << 31)) return 0;
  return 256 + (size_t)rl_tiles(N) * RL_Q * sizeof(double);
}

extern "C" int btc_roi_loss_fwd(const float* rcnn_cls, const float* rcnn_reg, const float* rois, const float* gt_of_rois,
                                const float* gt_of_rois_src, int gt_width, const int64_t* reg_valid_mask, const void* cls_labels,
                                int label_kind, int N, int with_corner, float cls_weight, float reg_weight, float corner_weight, float* out,
                                float* norms, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = rl_check("btc_roi_loss_fwd", rcnn_cls, rcnn_reg, rois, gt_of_rois, gt_of_rois_src, gt_width, reg_valid_mask, cls_labels, label_kind, N);
  if (rc != BTC_OK) return rc;
  BTC_CHECK_ARG(out && norms && ws, "btc_roi_loss_fwd: missing pointer (out, norms or ws)");
  const size_t need = btc_roi_loss_ws_bytes(N);
  BTC_CHECK_ARG(need != 0 && ws_bytes >= need, "btc_roi_loss_fwd: workspace too small");
  const RlArgs A = rl_args(rcnn_cls, rcnn_reg, rois, gt_of_rois, gt_of_rois_src, gt_width, reg_valid_mask, cls_labels, label_kind, N, with_corner,
                           cls_weight, reg_weight, corner_weight);
  int32_t* counter = (int32_t*)ws;   // first 256 bytes zero on entry / exit
  double* partial = (double*)((char*)ws + 256);
  roi_loss_fwd<<<rl_tiles(N), RL_T, 0, stream>>>(A, partial, counter, out, norms);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}

extern "C" int btc_roi_loss_bwd(const float* rcnn_cls, const float* rcnn_reg, const float* rois, const float* gt_of_rois,
                                const float* gt_of_rois_src, int gt_width, const int64_t* reg_valid_mask, const void* cls_labels,
                                int label_kind, int N, int with_corner, float cls_weight, float reg_weight, float corner_weight,
                                const float* norms, const float* grad_total, float* d_cls, float* d_reg, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = rl_check("btc_roi_loss_bwd", rcnn_cls, rcnn_reg, rois, gt_of_rois, gt_of_rois_src, gt_width, reg_valid_mask, cls_labels, label_kind, N);
  if (rc != BTC_OK) return rc;
  BTC_CHECK_ARG(norms && grad_total, "btc_roi_loss_bwd: missing pointer (norms or grad_total)");
  BTC_CHECK_ARG(N == 0 || (d_cls && d_reg), "btc_roi_loss_bwd: missing pointer (d_cls or d_reg)");
  if (N == 0) return BTC_OK;
  const RlArgs A = rl_args(rcnn_cls, rcnn_reg, rois, gt_of_rois, gt_of_rois_src, gt_width, reg_valid_mask, cls_labels, label_kind, N, with_corner,
                           cls_weight, reg_weight, corner_weight);
  roi_loss_bwd<<<btc_cdiv((long long)N * RL_LANES, RL_T), RL_T, 0, stream>>>(A, norms, grad_total, d_cls, d_reg);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}
