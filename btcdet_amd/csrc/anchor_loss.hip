// The anchor head's loss, fused (include/btcdet_hip_anchor_loss.h: forward one launch, backward one launch).
//
// Replaces AnchorHeadTemplate.get_loss -> get_cls_layer_loss / get_box_reg_layer_loss
// (/root/reference/btcdet/models/dense_heads/anchor_head_template.py:102-225) with the loss functions of
// /root/reference/btcdet/utils/loss_utils.py:9-73 (sigmoid focal, alpha 0.25, gamma 2), :174-236 (smooth L1, beta 1/9, the code
// weights built and never applied) and :281-306 (cross-entropy over the direction bins): there a one-hot tensor over (B, A, C + 1), the
// anchors repeated per scene, two cats for the heading products and several dozen elementwise launches plus their autograd twins.
//   n_b = max(#positives of scene b, 1)
//   cls = cls_weight / B * sum_b 1/n_b sum_{a cared, c} alpha_t pt^2 (max(x, 0) - x t + log1p(exp(-|x|)))
//   loc = loc_weight / B * sum_b 1/n_b sum_{a positive, k} smoothL1(u_k - v_k), column 6 as sin(p) cos(t) against cos(p) sin(t)
//   dir = dir_weight / B * sum_b 1/n_b sum_{a positive} CE(dir logits, direction bin of t_6 + anchor_6)
// An anchor is read as far as its label asks: class logits unless ignored, everything else only when positive -- nearly every anchor
// is background.  A workgroup stays inside one scene and stores four doubles (three sums, its positive count); the last workgroup to
// arrive reduces scene by scene, one wave per scene, in a fixed order.  Every index is formed from b < B, a < A, c < C, j < bins; the
// direction bin is clamped to [0, bins) as a float before it becomes an index (a NaN heading lands on bin 0).
#include "btc_common.h"

#include "../../include/btcdet_hip_anchor_loss.h"

namespace {

constexpr int AL_T = BTC_ANCHOR_LOSS_THREADS;
constexpr int AL_WAVES = AL_T / 64;
constexpr float AL_BETA = (float)(1.0 / 9.0);
constexpr float AL_HALF_BETA = 0.5f * AL_BETA;                     // exact
constexpr float AL_TWO_PI = (float)(2.0 * 3.14159265358979323846);
constexpr float AL_INV_TWO_PI = 1.0f / AL_TWO_PI;                  // the float32 reciprocal of the float32 2 pi

struct AlParams {
  int B, A, C, bins, tiles;
  float dir_offset, inv_bin_w;
  float w[3];   // forward: the three weights; backward: weight_q / (float)B
};

// sigmoid focal pieces of one (anchor, class): term = w * bce, d term / dx = +-w * ((2 * qt) * bce + pt)
struct AlFocal {
  float w, bce, pt, qt;
};

__device__ __forceinline__ AlFocal al_focal(float x, bool t) {
  const float e = expf(-fabsf(x));
  const float r = 1.0f / (1.0f + e);
  const float er = e * r;
  const float p = x >= 0.0f ? r : er;
  const float om = 1.0f - p;
  AlFocal f;
  f.pt = t ? om : p, f.qt = t ? p : om;
  const float lin = fmaxf(x, 0.0f) - (t ? x : 0.0f);
  f.bce = lin + log1pf(e);
  const float pt2 = f.pt * f.pt;
  f.w = (t ? 0.25f : 0.75f) * pt2;
  return f;
}

// the class that counts as hot for a cared label (0: none)
__device__ __forceinline__ int al_hot(int lab, int C) { return lab > 0 ? (C == 1 ? 1 : lab) : 0; }

// column k of a positive anchor: d = u - v and du / dp_k; false when the target side is NaN (the column is skipped)
__device__ __forceinline__ bool al_diff(const float* __restrict__ p, const float* __restrict__ t, int k, float* d, float* chain) {
  if (k < 6) {
    const float v = t[k];
    *d = p[k] - v, *chain = 1.0f;
    return !isnan(v);
  }
  const float sp = sinf(p[6]), cp = cosf(p[6]), st = sinf(t[6]), ct = cosf(t[6]);
  const float u = sp * ct, v = cp * st;
  const float cc = cp * ct, ss = sp * st;
  *d = u - v, *chain = cc + ss;
  return !isnan(v);
}

__device__ __forceinline__ float al_smooth_l1(float d) {
  const float n = fabsf(d);
  const float nn = n * n;
  return n < AL_BETA ? 0.5f * nn / AL_BETA : n - AL_HALF_BETA;
}

__device__ __forceinline__ int al_dir_bin(float t6, float a6, const AlParams& P) {
  const float rot = t6 + a6;
  const float v = rot - P.dir_offset;
  const float q = v * AL_INV_TWO_PI;
  const float m = floorf(q) * AL_TWO_PI;
  const float lp = v - m;
  const float kf = floorf(lp * P.inv_bin_w);
  return (int)fminf(fmaxf(kf, 0.0f), (float)(P.bins - 1));
}

// partial[(b * tiles + tile) * 4 + q]: q = 0 class, 1 location, 2 direction, 3 positives
__global__ __launch_bounds__(AL_T) void anchor_loss_fwd(const float* __restrict__ cls, const float* __restrict__ box, const float* __restrict__ dir,
                                                        const int32_t* __restrict__ labels, const float* __restrict__ tgt,
                                                        const float* __restrict__ anchors, const AlParams P, double* __restrict__ partial,
                                                        int32_t* __restrict__ counter, float* __restrict__ out, float* __restrict__ norms) {
  __shared__ double s_red[AL_WAVES][4];
  const int b = blockIdx.x / P.tiles, tile = blockIdx.x % P.tiles;
  double acc[4] = {0, 0, 0, 0};
  for (int a = tile * AL_T + threadIdx.x; a < P.A; a += P.tiles * AL_T) {
    const size_t i = (size_t)b * P.A + a;
    const int lab = labels[i];
    if (lab < 0) continue;
    const int hot = al_hot(lab, P.C);
    for (int c = 0; c < P.C; ++c) {
      const AlFocal f = al_focal(cls[i * P.C + c], c + 1 == hot);
      acc[0] += (double)(f.w * f.bce);
    }
    if (lab == 0) continue;
    acc[3] += 1.0;
    const float* p = box + i * 7;
    const float* t = tgt + i * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      float d, chain;
      if (al_diff(p, t, k, &d, &chain)) acc[1] += (double)al_smooth_l1(d);
    }
    if (P.bins > 0) {
      const float* z = dir + i * P.bins;
      const int kb = al_dir_bin(t[6], anchors[(size_t)a * 7 + 6], P);
      float m = z[0];
      for (int j = 1; j < P.bins; ++j) m = fmaxf(m, z[j]);
      float s = 0.0f;
      for (int j = 0; j < P.bins; ++j) s += expf(z[j] - m);
      acc[2] += (double)(logf(s) - (z[kb] - m));
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    acc[q] = btc_wave_sum(acc[q]);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6][q] = acc[q];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const double v = (s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + (s_red[2][threadIdx.x] + s_red[3][threadIdx.x]);
    btc_st_agent(&partial[(size_t)blockIdx.x * 4 + threadIdx.x], v);
  }
  if (!btc_last_arriver(counter, (int)gridDim.x)) return;   // (the protocol: btc_common.h)
  // the last workgroup: wave w takes scenes w, w + 4, ...; lane l sums quantity l % 4 over tiles l / 4, l / 4 + 16, ... in order, then a
  // fixed tree over the 16 lanes of each quantity; lane 0 of the wave carries sum_b S_q(b) / n_b over its scenes, ascending
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double tot[3] = {0, 0, 0};
  for (int s = wave; s < P.B; s += AL_WAVES) {
    double v = 0.0;
    for (int g = lane >> 2; g < P.tiles; g += 16) v += btc_ld_agent(&partial[((size_t)s * P.tiles + g) * 4 + (lane & 3)]);
#pragma unroll
    for (int o = 32; o >= 4; o >>= 1) v += __shfl_down(v, o, 64);   // lanes 0..3: the scene's four quantities
    const double npos = __shfl(v, 3, 64);
    const double nb = npos > 1.0 ? npos : 1.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) tot[q] += __shfl(v, q, 64) / nb;
    if (lane == 0) norms[s] = (float)(1.0 / nb);
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) s_red[wave][q] = tot[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float o[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double v = (s_red[0][q] + s_red[1][q]) + (s_red[2][q] + s_red[3][q]);
      o[q] = (float)(v / (double)P.B * (double)P.w[q]);
      out[q] = o[q];
    }
    const float box_loss = o[1] + o[2];
    out[3] = o[0] + box_loss;   // (the fp32 sums `cls + (loc + dir)` the caller would otherwise make with two more launches)
    __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// every element of d_cls / d_box / d_dir is written: the caller allocates them uninitialised
__global__ __launch_bounds__(AL_T) void anchor_loss_bwd(const float* __restrict__ cls, const float* __restrict__ box, const float* __restrict__ dir,
                                                        const int32_t* __restrict__ labels, const float* __restrict__ tgt,
                                                        const float* __restrict__ anchors, const AlParams P, const float* __restrict__ norms,
                                                        const float* __restrict__ g, float* __restrict__ d_cls, float* __restrict__ d_box,
                                                        float* __restrict__ d_dir) {
  const long long total = (long long)P.B * P.A;
  const long long il = (long long)blockIdx.x * AL_T + threadIdx.x;
  if (il >= total) return;
  const size_t i = (size_t)il;
  const int b = (int)(il / P.A), a = (int)(il % P.A);
  const int lab = labels[i];
  const float gn = g[0] * norms[b];
  if (lab < 0) {
    for (int c = 0; c < P.C; ++c) d_cls[i * P.C + c] = 0.0f;
  } else {
    const int hot = al_hot(lab, P.C);
    const float sc = gn * P.w[0];
    for (int c = 0; c < P.C; ++c) {
      const bool t = c + 1 == hot;
      const AlFocal f = al_focal(cls[i * P.C + c], t);
      const float inner = (2.0f * f.qt) * f.bce + f.pt;
      const float gr = f.w * inner;
      d_cls[i * P.C + c] = sc * (t ? -gr : gr);
    }
  }
  if (lab <= 0) {
#pragma unroll
    for (int k = 0; k < 7; ++k) d_box[i * 7 + k] = 0.0f;
    for (int j = 0; j < P.bins; ++j) d_dir[i * P.bins + j] = 0.0f;
    return;
  }
  const float* p = box + i * 7;
  const float* t = tgt + i * 7;
  const float sl = gn * P.w[1];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    float d, chain, v = 0.0f;
    if (al_diff(p, t, k, &d, &chain)) {
      const float gr = fabsf(d) < AL_BETA ? d / AL_BETA : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));
      v = sl * gr;
      if (k == 6) v = v * chain;
    }
    d_box[i * 7 + k] = v;
  }
  if (P.bins > 0) {
    const float* z = dir + i * P.bins;
    const int kb = al_dir_bin(t[6], anchors[(size_t)a * 7 + 6], P);
    const float sd = gn * P.w[2];
    float m = z[0];
    for (int j = 1; j < P.bins; ++j) m = fmaxf(m, z[j]);
    float s = 0.0f;
    for (int j = 0; j < P.bins; ++j) s += expf(z[j] - m);
    for (int j = 0; j < P.bins; ++j) {
      const float soft = expf(z[j] - m) / s;
      d_dir[i * P.bins + j] = sd * (soft - (j == kb ? 1.0f : 0.0f));
    }
  }
}

int al_tiles(int A) {
  int t = btc_cdiv(A, AL_T);
  return t < 1 ? 1 : (t > BTC_ANCHOR_LOSS_MAX_TILES ? BTC_ANCHOR_LOSS_MAX_TILES : t);
}

// the checks both entry points share
int al_check(const char* who, const float* cls, const float* box, const float* dir, const int32_t* labels, const float* tgt, const float* anchors,
             int B, int A, int C, int bins) {
  BTC_CHECK_ARG(B >= 1, "%s: need B >= 1, got %d", who, B);
  BTC_CHECK_ARG(A >= 0, "%s: negative count (A %d)", who, A);
  BTC_CHECK_ARG(C >= 1 && C < BTC_HEADS_MAX_CLASSES, "%s: C %d outside [1, %d)", who, C, BTC_HEADS_MAX_CLASSES);
  BTC_CHECK_ARG(bins >= 0 && bins <= BTC_ANCHOR_LOSS_MAX_BINS, "%s: bins %d outside [0, %d]", who, bins, BTC_ANCHOR_LOSS_MAX_BINS);
  const int widest = C > 7 ? (C > bins ? C : bins) : (bins > 7 ? bins : 7);
  BTC_CHECK_ARG((long long)B * A * widest < (1ll << 31), "%s: B * A * max(C, 7, bins) = %lld does not fit 31 bits", who, (long long)B * A * widest);
  BTC_CHECK_ARG(A == 0 || (cls && box && labels && tgt && anchors),
                "%s: missing pointer (cls_preds, box_preds, box_cls_labels, box_reg_targets or anchors)", who);
  BTC_CHECK_ARG(A == 0 || bins == 0 || dir, "%s: missing pointer (dir_cls_preds with bins %d)", who, bins);
  return BTC_OK;
}

AlParams al_params(int B, int A, int C, int bins, float dir_offset, float w0, float w1, float w2) {
  AlParams P;
  P.B = B, P.A = A, P.C = C, P.bins = bins, P.tiles = al_tiles(A);
  P.dir_offset = dir_offset;
  P.inv_bin_w = bins > 0 ? 1.0f / (float)(2.0 * 3.14159265358979323846 / (double)bins) : 0.0f;
  P.w[0] = w0, P.w[1] = w1, P.w[2] = bins > 0 ? w2 : 0.0f;
  return P;
}

}  // namespace

extern "C" size_t btc_anchor_loss_ws_bytes(int B, int A) {
  if (B < 1 || A < 0 || (long long)B * A * 7 >= (1ll << 31) || (long long)B * BTC_ANCHOR_LOSS_MAX_TILES >= (1ll << 31)) return 0;
  return 256 + (size_t)B * (size_t)al_tiles(A) * 4 * sizeof(double);
}

extern "C" int btc_anchor_loss_fwd(const float* cls_preds, const float* box_preds, const float* dir_cls_preds, const int32_t* box_cls_labels,
                                   const float* box_reg_targets, const float* anchors, int B, int A, int C, int bins, float cls_weight,
                                   float loc_weight, float dir_weight, float dir_offset, float* out, float* norms, void* ws, size_t ws_bytes,
                                   void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = al_check("btc_anchor_loss_fwd", cls_preds, box_preds, dir_cls_preds, box_cls_labels, box_reg_targets, anchors, B, A, C, bins);
  if (rc != BTC_OK) return rc;
  BTC_CHECK_ARG(out && norms && ws, "btc_anchor_loss_fwd: missing pointer (out, norms or ws)");
  const size_t need = btc_anchor_loss_ws_bytes(B, A);
  BTC_CHECK_ARG(need != 0 && ws_bytes >= need, "btc_anchor_loss_fwd: workspace too small");
  const AlParams P = al_params(B, A, C, bins, dir_offset, cls_weight, loc_weight, dir_weight);
  int32_t* counter = (int32_t*)ws;   // first 256 bytes zero on entry / exit
  double* partial = (double*)((char*)ws + 256);
  anchor_loss_fwd<<<B * P.tiles, AL_T, 0, stream>>>(cls_preds, box_preds, dir_cls_preds, box_cls_labels, box_reg_targets, anchors, P, partial, counter,
                                                    out, norms);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}

extern "C" int btc_anchor_loss_bwd(const float* cls_preds, const float* box_preds, const float* dir_cls_preds, const int32_t* box_cls_labels,
                                   const float* box_reg_targets, const float* anchors, int B, int A, int C, int bins, float cls_weight,
                                   float loc_weight, float dir_weight, float dir_offset, const float* norms, const float* grad_total, float* d_cls,
                                   float* d_box, float* d_dir, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = al_check("btc_anchor_loss_bwd", cls_preds, box_preds, dir_cls_preds, box_cls_labels, box_reg_targets, anchors, B, A, C, bins);
  if (rc != BTC_OK) return rc;
  BTC_CHECK_ARG(norms && grad_total, "btc_anchor_loss_bwd: missing pointer (norms or grad_total)");
  BTC_CHECK_ARG(A == 0 || (d_cls && d_box), "btc_anchor_loss_bwd: missing pointer (d_cls or d_box)");
  BTC_CHECK_ARG(A == 0 || bins == 0 || d_dir, "btc_anchor_loss_bwd: missing pointer (d_dir with bins %d)", bins);
  if (A == 0) return BTC_OK;
  const float fb = (float)B;
  const AlParams P = al_params(B, A, C, bins, dir_offset, cls_weight / fb, loc_weight / fb, dir_weight / fb);
  anchor_loss_bwd<<<btc_cdiv((long long)B * A, AL_T), AL_T, 0, stream>>>(cls_preds, box_preds, dir_cls_preds, box_cls_labels, box_reg_targets, anchors, P,
                                                                         norms, grad_total, d_cls, d_box, d_dir);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}
