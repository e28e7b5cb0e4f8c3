// KITTI AP evaluation for gfx950 (include/btcdet_hip_infer.h: btc_kitti_overlaps, btc_kitti_match_tp, btc_kitti_match_stats).
//
// Replaces the reference's kitti_object_eval_python (eval.py: numba on the CPU; rotate_iou.py: numba.cuda, which does not exist on
// ROCm).  The reference computes pairwise overlaps over 50-frame blocks -- most pairs cross-frame and thrown away -- and then runs one
// sequential greedy matching per frame x metric x class x difficulty x overlap level x score threshold.  Here the ground truths and
// detections of ALL frames arrive concatenated with per-frame offsets and an evaluation is a constant number of launches:
//
//   kitti_overlaps     grid (frames, pair blocks).  One thread per (detection, ground truth) pair of ONE frame: the image-box IoU, the
//                      rotated BEV IoU and the 3-D IoU (they share the rotated intersection), then the detection-against-DontCare
//                      pairs.  All float64: the work is a few hundred thousand pairs, bound by launch latency, not by the FP64 pipe,
//                      and float64 keeps every value far inside the margins the decisions below are held to.  The rotated
//                      intersection is exact geometry: rectangle A is expressed in B's frame and clipped against B's four axis-aligned
//                      half-planes (Sutherland-Hodgman, <= 8 vertices).  iou3d_dev.h's box_overlap is NOT used: it carries the NMS
//                      kernel's 1e-2 in_box2d margin.
//   kitti_match_tp     pass A of compute_statistics_jit (thresh = 0, compute_fp = False): one thread per (frame, combination), a
//                      combination being metric x class x difficulty x overlap level.  Writes, per ground truth, the detection it
//                      matched as a true positive (or -1); the host gathers the scores and forms the <= 41 thresholds in float64.
//   kitti_match_stats  pass B (compute_fp = True): one wave per (frame, combination), lanes over the thresholds.  The lanes of a wave
//                      walk the same overlaps, so the loads are wave-uniform.  tp / fp / fn go to int32 counters with atomics; the
//                      similarity (1 + cos(d alpha)) / 2 is float64, written as a per-frame partial ...
//   kitti_sim_reduce   ... and summed over the frames in frame order by one thread per (combination, threshold): same bits every run.
//
// Both matching kernels run match_one<FP> (FP = compute_fp) and keep a 1024-bit "assigned" set per thread in LDS (word-major,
// lane-minor: conflict-free), 8 KB per wave -- that, with the serial ground-truth x detection walk of one thread, bounds them: the walk is latency-bound on dependent compares,
// the grid (frames x combinations waves) is what fills the machine.  Scores are float64 end to end: ties and the first-in-order rule
// (`dt_score > valid_detection`) are decided on the values the caller holds.
#include "btc_common.h"
#include "../../include/btcdet_hip_infer.h"

namespace {

constexpr int KE_MAX_N = 1024;            // detections / ground truths per frame
constexpr int KE_WORDS = KE_MAX_N / 64;
constexpr int KE_PTS = 41;                // N_SAMPLE_PTS
constexpr int KE_GT_COLS = 12;            // bbox 4, location 3, dimensions 3 (l, h, w), rotation_y, alpha
constexpr int KE_DT_COLS = 13;            // ... and score

typedef unsigned long long u64;

// area of the intersection of two rotated rectangles (cx, cy, xd, yd, angle; rotate_iou.py's corner convention: the local corner
// (x, y) sits at (c x + s y + cx, -s x + c y + cy)).  A's corners in B's frame, clipped against |x| <= xd_B / 2, |y| <= yd_B / 2.
__device__ double rect_inter(double ax, double ay, double aw, double al, double aa, double bx, double by, double bw, double bl, double ba) {
  const double dx = ax - bx, dy = ay - by;
  const double r = 0.5 * (sqrt(aw * aw + al * al) + sqrt(bw * bw + bl * bl));
  if (dx * dx + dy * dy > r * r) return 0.0;   // the circumscribed circles are apart
  const double ca = cos(aa), sa = sin(aa), cb = cos(ba), sb = sin(ba);
  double px[10], py[10], qx[10], qy[10];
  const double hx[4] = {-aw / 2, -aw / 2, aw / 2, aw / 2}, hy[4] = {-al / 2, al / 2, al / 2, -al / 2};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double wx = ca * hx[i] + sa * hy[i] + dx, wy = -sa * hx[i] + ca * hy[i] + dy;   // world, relative to B's centre
    px[i] = cb * wx - sb * wy;                                                              // B's frame: the transpose of B's rotation
    py[i] = sb * wx + cb * wy;
  }
  int n = 4;
  const double lim[2] = {bw / 2, bl / 2};
#pragma unroll 1
  for (int e = 0; e < 4; ++e) {
    // half-plane s * coord <= limit; e: 0 x <= hw, 1 -x <= hw, 2 y <= hl, 3 -y <= hl
    const bool use_y = e >= 2;
    const double sg = (e & 1) ? -1.0 : 1.0, L = lim[e >> 1];
    int m = 0;
    for (int i = 0; i < n; ++i) {
      const int j = (i + 1 == n) ? 0 : i + 1;
      const double da = L - sg * (use_y ? py[i] : px[i]), db = L - sg * (use_y ? py[j] : px[j]);
      if (da >= 0 && m < 10) {
        qx[m] = px[i];
        qy[m] = py[i];
        ++m;
      }
      if ((da >= 0) != (db >= 0) && m < 10) {
        const double t = da / (da - db);
        qx[m] = px[i] + t * (px[j] - px[i]);
        qy[m] = py[i] + t * (py[j] - py[i]);
        ++m;
      }
    }
    n = m;   // (a convex quadrilateral cut four times has at most 8 vertices; the writes above stop at 10 whatever rounding does)
    if (n < 3) return 0.0;
    for (int i = 0; i < n; ++i) {
      px[i] = qx[i];
      py[i] = qy[i];
    }
  }
  double s = 0.0;
  for (int i = 0; i < n; ++i) {
    const int j = (i + 1 == n) ? 0 : i + 1;
    s += px[i] * py[j] - py[i] * px[j];
  }
  return fabs(s) / 2;
}

struct OvArgs {
  const double* gt;          // [NG][12]
  const double* dt;          // [ND][13]
  const double* dc;          // [NC][4]
  const int32_t* frames;     // [F + 1][3]: first ground truth, detection, DontCare box of a frame
  const long long* pairs;    // [F + 1][2]: first (detection, ground truth) pair, first (detection, DontCare) pair
  long long P;               // pairs of one metric
  double* ov;                // [3][P]
  double* ov_dc;             // [PD]
};

__global__ __launch_bounds__(256) void kitti_overlaps(OvArgs a) {
  const int f = blockIdx.x;
  const int g0 = a.frames[f * 3 + 0], d0 = a.frames[f * 3 + 1], c0 = a.frames[f * 3 + 2];
  const int ng = a.frames[f * 3 + 3] - g0, nd = a.frames[f * 3 + 4] - d0, nc = a.frames[f * 3 + 5] - c0;
  const long long q = (long long)blockIdx.y * 256 + threadIdx.x;
  const long long np = (long long)nd * ng, npc = (long long)nd * nc;
  if (q < np) {
    const int j = (int)(q / ng), i = (int)(q - (long long)j * ng);
    const double* D = a.dt + (size_t)(d0 + j) * KE_DT_COLS;
    const double* G = a.gt + (size_t)(g0 + i) * KE_GT_COLS;
    // image boxes: image_box_overlap, criterion -1
    double o2 = 0.0;
    const double iw = fmin(D[2], G[2]) - fmax(D[0], G[0]);
    if (iw > 0) {
      const double ih = fmin(D[3], G[3]) - fmax(D[1], G[1]);
      if (ih > 0) o2 = iw * ih / ((D[2] - D[0]) * (D[3] - D[1]) + (G[2] - G[0]) * (G[3] - G[1]) - iw * ih);
    }
    // BEV: (x, z, l, w, ry); 3-D: x height overlap over the union of volumes, y the bottom face
    const double inter = rect_inter(D[4], D[6], D[7], D[9], D[10], G[4], G[6], G[7], G[9], G[10]);
    double ob = 0.0, o3 = 0.0;
    if (inter > 0) {
      ob = inter / (D[7] * D[9] + G[7] * G[9] - inter);
      const double h = fmin(D[5], G[5]) - fmax(D[5] - D[8], G[5] - G[8]);
      if (h > 0) {
        const double inc = h * inter;
        o3 = inc / (D[7] * D[8] * D[9] + G[7] * G[8] * G[9] - inc);
      }
    }
    const long long at = a.pairs[f * 2] + q;
    a.ov[at] = o2;
    a.ov[a.P + at] = ob;
    a.ov[2 * a.P + at] = o3;
  } else if (q - np < npc) {
    const long long qc = q - np;
    const int j = (int)(qc / nc), i = (int)(qc - (long long)j * nc);
    const double* D = a.dt + (size_t)(d0 + j) * KE_DT_COLS;
    const double* C = a.dc + (size_t)(c0 + i) * 4;
    double o = 0.0;
    const double iw = fmin(D[2], C[2]) - fmax(D[0], C[0]);
    if (iw > 0) {
      const double ih = fmin(D[3], C[3]) - fmax(D[1], C[1]);
      if (ih > 0) o = iw * ih / ((D[2] - D[0]) * (D[3] - D[1]));   // criterion 0: the detection's area
    }
    a.ov_dc[a.pairs[f * 2 + 1] + qc] = o;
  }
}

struct MatchArgs {
  const double* ov;          // [3][P]
  const double* ov_dc;       // [PD]
  const double* gt;
  const double* dt;
  const int8_t* ign_gt;      // [C * D][NG]
  const int8_t* ign_dt;      // [C * D][ND]
  const double* min_ov;      // [K][3][C]
  const double* thr;         // [combos][41]     (pass B)
  const int32_t* n_thr;      // [combos]
  const int32_t* frames;
  const long long* pairs;
  long long P;
  int F, NG, ND, m0, M, C, D, K, aos;
  int32_t* tp_det;           // [combos][NG]     (pass A)
  int32_t* tp_count;         // [combos]
  int32_t* counts;           // [combos][41][3]  (pass B)
  double* sim_part;          // [F][C * D * K][41]
};

// One greedy matching, the loops of compute_statistics_jit in their order.  FP = compute_fp.  `asg`: this thread's assigned set, word w
// at asg[w * 64]; thr: the score threshold (FP).  Pass A writes tp_det; pass B returns tp / fp / fn / similarity.
template <bool FP>
__device__ __forceinline__ void match_one(const MatchArgs& a, int f, int combo, double thr, u64* asg, int* o_tp, int* o_fp, int* o_fn,
                                          double* o_sim) {
  const int k = combo % a.K, d = (combo / a.K) % a.D, c = (combo / (a.K * a.D)) % a.C, mi = combo / (a.K * a.D * a.C);
  const int metric = a.m0 + mi;
  const int g0 = a.frames[f * 3 + 0], d0 = a.frames[f * 3 + 1], c0 = a.frames[f * 3 + 2];
  const int ng = a.frames[f * 3 + 3] - g0, nd = a.frames[f * 3 + 4] - d0, nc = a.frames[f * 3 + 5] - c0;
  const double min_ov = a.min_ov[((size_t)k * 3 + metric) * a.C + c];
  const double* ov = a.ov + (size_t)metric * a.P + a.pairs[f * 2];
  const int8_t* ig = a.ign_gt + (size_t)(c * a.D + d) * a.NG + g0;
  const int8_t* id = a.ign_dt + (size_t)(c * a.D + d) * a.ND + d0;
  const double* dt = a.dt + (size_t)d0 * KE_DT_COLS;
  const int words = (nd + 63) >> 6;
  const bool want_sim = FP && a.aos && metric == 0;   // the similarity belongs to the bbox metric only
  for (int w = 0; w < words; ++w) asg[w * 64] = 0ull;
  int tp = 0, fp = 0, fn = 0;
  double sim = 0.0;
  const double NO_DETECTION = -10000000.0;
  for (int i = 0; i < ng; ++i) {
    const int gi = ig[i];
    if (!FP) a.tp_det[(size_t)combo * a.NG + g0 + i] = -1;
    if (gi == -1) continue;
    int det = -1;
    double valid = NO_DETECTION, best = 0.0;
    bool took_ignored = false;
    for (int j = 0; j < nd; ++j) {
      const int dj = id[j];
      if (dj == -1) continue;
      if ((asg[(j >> 6) * 64] >> (j & 63)) & 1ull) continue;
      const double sc = dt[(size_t)j * KE_DT_COLS + 12];
      if (FP && sc < thr) continue;
      const double o = ov[(size_t)j * ng + i];
      if (!(o > min_ov)) continue;
      if (!FP) {
        if (sc > valid) {
          det = j;
          valid = sc;
        }
      } else if ((o > best || took_ignored) && dj == 0) {
        best = o;
        det = j;
        valid = 1.0;
        took_ignored = false;
      } else if (valid == NO_DETECTION && dj == 1) {
        det = j;
        valid = 1.0;
        took_ignored = true;
      }
    }
    if (valid == NO_DETECTION) {
      if (gi == 0) ++fn;
    } else {
      if (!(gi == 1 || id[det] == 1)) {
        ++tp;
        if (!FP) a.tp_det[(size_t)combo * a.NG + g0 + i] = d0 + det;
        if (FP && want_sim) sim += (1.0 + cos(a.gt[(size_t)(g0 + i) * KE_GT_COLS + 11] - dt[(size_t)det * KE_DT_COLS + 11])) / 2.0;
      }
      asg[(det >> 6) * 64] |= 1ull << (det & 63);
    }
  }
  if (FP) {
    for (int j = 0; j < nd; ++j)
      if (id[j] == 0 && !((asg[(j >> 6) * 64] >> (j & 63)) & 1ull) && !(dt[(size_t)j * KE_DT_COLS + 12] < thr)) ++fp;
    if (metric == 0) {
      const double* odc = a.ov_dc + a.pairs[f * 2 + 1];
      for (int i = 0; i < nc; ++i)
        for (int j = 0; j < nd; ++j) {
          if ((asg[(j >> 6) * 64] >> (j & 63)) & 1ull) continue;
          if (id[j] != 0) continue;
          if (dt[(size_t)j * KE_DT_COLS + 12] < thr) continue;
          if (odc[(size_t)j * nc + i] > min_ov) {
            asg[(j >> 6) * 64] |= 1ull << (j & 63);
            --fp;
          }
        }
    }
  }
  *o_tp = tp;
  *o_fp = fp;
  *o_fn = fn;
  *o_sim = sim;
}

// pass A: one thread per (frame, combination), the combination fastest
__global__ __launch_bounds__(64) void kitti_match_tp(MatchArgs a) {
  __shared__ u64 s_asg[KE_WORDS * 64];
  const int combos = a.M * a.C * a.D * a.K;
  const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
  if (t >= (long long)a.F * combos) return;
  const int f = (int)(t / combos), combo = (int)(t - (long long)f * combos);
  int tp, fp, fn;
  double sim;
  match_one<false>(a, f, combo, 0.0, s_asg + threadIdx.x, &tp, &fp, &fn, &sim);
  if (tp) atomicAdd(a.tp_count + combo, tp);
}

// pass B: one wave per (frame, combination), lanes over the thresholds
__global__ __launch_bounds__(64) void kitti_match_stats(MatchArgs a) {
  __shared__ u64 s_asg[KE_WORDS * 64];
  const int combos = a.M * a.C * a.D * a.K;
  const int f = (int)(blockIdx.x / combos), combo = (int)(blockIdx.x - (unsigned)f * combos);
  const int t = threadIdx.x;
  if (t >= KE_PTS) return;
  const bool want_sim = a.aos && a.m0 == 0 && combo < a.C * a.D * a.K;   // the bbox metric's combinations come first
  const int nt = min(max(a.n_thr[combo], 0), KE_PTS);
  int tp = 0, fp = 0, fn = 0;
  double sim = 0.0;
  if (t < nt) {
    match_one<true>(a, f, combo, a.thr[(size_t)combo * KE_PTS + t], s_asg + t, &tp, &fp, &fn, &sim);
    int32_t* cnt = a.counts + ((size_t)combo * KE_PTS + t) * 3;
    if (tp) atomicAdd(cnt + 0, tp);
    if (fp) atomicAdd(cnt + 1, fp);
    if (fn) atomicAdd(cnt + 2, fn);
  }
  if (want_sim) a.sim_part[((size_t)f * (a.C * a.D * a.K) + combo) * KE_PTS + t] = sim;
}

// similarity[cdk][t] = the per-frame partials summed in frame order
__global__ __launch_bounds__(64) void kitti_sim_reduce(const double* part, int F, int n, double* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int f = 0; f < F; ++f) s += part[(size_t)f * n + i];
  out[i] = s;
}

// the host's frame table: offsets ascending from 0, at most 1024 detections / ground truths per frame; -> totals and pair counts
int check_frames(const char* who, const int32_t* h, int F, long long* NG, long long* ND, long long* NC, long long* P, long long* PD, int* max_pairs) {
  BTC_CHECK_ARG(F >= 0, "%s: n_frames = %d", who, F);
  BTC_CHECK_ARG(h, "%s: missing pointer (h_frames)", who);
  BTC_CHECK_ARG(h[0] == 0 && h[1] == 0 && h[2] == 0, "%s: the frame table does not start at 0", who);
  long long p = 0, pd = 0, mp = 0;
  for (int f = 0; f < F; ++f) {
    const long long ng = (long long)h[f * 3 + 3] - h[f * 3 + 0], nd = (long long)h[f * 3 + 4] - h[f * 3 + 1], nc = (long long)h[f * 3 + 5] - h[f * 3 + 2];
    BTC_CHECK_ARG(ng >= 0 && nd >= 0 && nc >= 0, "%s: negative count in frame %d (%lld ground truths, %lld detections, %lld DontCare)", who, f, ng, nd, nc);
    BTC_CHECK_ARG(ng <= KE_MAX_N, "%s: frame %d has %lld ground truths, more than %d", who, f, ng, KE_MAX_N);
    BTC_CHECK_ARG(nd <= KE_MAX_N, "%s: frame %d has %lld detections, more than %d", who, f, nd, KE_MAX_N);
    BTC_CHECK_ARG(nc <= ng, "%s: frame %d has more DontCare boxes (%lld) than ground truths (%lld)", who, f, nc, ng);
    p += nd * ng;
    pd += nd * nc;
    if (nd * (ng + nc) > mp) mp = nd * (ng + nc);
  }
  *NG = h[F * 3 + 0];
  *ND = h[F * 3 + 1];
  *NC = h[F * 3 + 2];
  *P = p;
  *PD = pd;
  *max_pairs = (int)mp;
  return BTC_OK;
}

int check_combos(const char* who, int F, int m0, int M, int C, int D, int K, long long* combos) {
  BTC_CHECK_ARG(m0 >= 0 && M >= 1 && m0 + M <= 3, "%s: metrics %d .. %d (0 bbox, 1 bev, 2 3d)", who, m0, m0 + M - 1);
  BTC_CHECK_ARG(C >= 1 && D >= 1 && K >= 1, "%s: %d classes, %d difficulties, %d overlap levels", who, C, D, K);
  *combos = (long long)M * C * D * K;
  BTC_CHECK_ARG(*combos <= 65536 && (long long)F * *combos < 2147483647ll, "%s: %lld combinations x %d frames is too many for one launch", who, *combos, F);
  return BTC_OK;
}

}  // namespace

extern "C" int btc_kitti_overlaps(const double* gt_rows, const double* dt_rows, const double* dc_boxes, const int32_t* frames,
                                  const long long* pairs, const int32_t* h_frames, int n_frames, double* ov, double* ov_dc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  long long NG, ND, NC, P, PD;
  int max_pairs;
  const int rc = check_frames("btc_kitti_overlaps", h_frames, n_frames, &NG, &ND, &NC, &P, &PD, &max_pairs);
  if (rc != BTC_OK) return rc;
  BTC_CHECK_ARG(frames && pairs, "btc_kitti_overlaps: missing pointer (frame tables)");
  BTC_CHECK_ARG((NG == 0 || gt_rows) && (ND == 0 || dt_rows) && (NC == 0 || dc_boxes) && (P == 0 || ov) && (PD == 0 || ov_dc),
                "btc_kitti_overlaps: missing pointer");
  if (n_frames == 0 || max_pairs == 0) return BTC_OK;
  OvArgs a;
  a.gt = gt_rows; a.dt = dt_rows; a.dc = dc_boxes; a.frames = frames; a.pairs = pairs; a.P = P; a.ov = ov; a.ov_dc = ov_dc;
  kitti_overlaps<<<dim3(n_frames, btc_cdiv(max_pairs, 256)), 256, 0, stream>>>(a);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}

extern "C" int btc_kitti_match_tp(const double* ov, const double* dt_rows, const int8_t* ign_gt, const int8_t* ign_dt, const double* min_overlaps,
                                  const int32_t* frames, const long long* pairs, const int32_t* h_frames, int n_frames, int metric_first,
                                  int n_metric, int n_class, int n_diff, int n_level, int32_t* tp_det, int32_t* tp_count, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  long long NG, ND, NC, P, PD, combos;
  int max_pairs;
  int rc = check_frames("btc_kitti_match_tp", h_frames, n_frames, &NG, &ND, &NC, &P, &PD, &max_pairs);
  if (rc != BTC_OK) return rc;
  rc = check_combos("btc_kitti_match_tp", n_frames, metric_first, n_metric, n_class, n_diff, n_level, &combos);
  if (rc != BTC_OK) return rc;
  BTC_CHECK_ARG(frames && pairs && min_overlaps && tp_count, "btc_kitti_match_tp: missing pointer");
  BTC_CHECK_ARG((NG == 0 || (ign_gt && tp_det)) && (ND == 0 || (dt_rows && ign_dt)) && (P == 0 || ov), "btc_kitti_match_tp: missing pointer");
  BTC_HIP(hipMemsetAsync(tp_count, 0, (size_t)combos * sizeof(int32_t), stream));
  if (n_frames == 0) return BTC_OK;
  MatchArgs a = {};
  a.ov = ov; a.dt = dt_rows; a.ign_gt = ign_gt; a.ign_dt = ign_dt; a.min_ov = min_overlaps; a.frames = frames; a.pairs = pairs; a.P = P;
  a.F = n_frames; a.NG = (int)NG; a.ND = (int)ND; a.m0 = metric_first; a.M = n_metric; a.C = n_class; a.D = n_diff; a.K = n_level;
  a.tp_det = tp_det; a.tp_count = tp_count;
  kitti_match_tp<<<btc_cdiv((long long)n_frames * combos, 64), 64, 0, stream>>>(a);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}

extern "C" size_t btc_kitti_match_stats_ws_bytes(int n_frames, int n_class, int n_diff, int n_level, int compute_aos) {
  if (!compute_aos || n_frames <= 0 || n_class <= 0 || n_diff <= 0 || n_level <= 0) return 256;
  return btc_align((size_t)n_frames * n_class * n_diff * n_level * KE_PTS * sizeof(double));
}

extern "C" int btc_kitti_match_stats(const double* ov, const double* ov_dc, const double* gt_rows, const double* dt_rows, const int8_t* ign_gt,
                                     const int8_t* ign_dt, const double* min_overlaps, const double* thresholds, const int32_t* n_thresholds,
                                     const int32_t* frames, const long long* pairs, const int32_t* h_frames, int n_frames, int metric_first,
                                     int n_metric, int n_class, int n_diff, int n_level, int compute_aos, int32_t* counts, double* similarity,
                                     void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  long long NG, ND, NC, P, PD, combos;
  int max_pairs;
  int rc = check_frames("btc_kitti_match_stats", h_frames, n_frames, &NG, &ND, &NC, &P, &PD, &max_pairs);
  if (rc != BTC_OK) return rc;
  rc = check_combos("btc_kitti_match_stats", n_frames, metric_first, n_metric, n_class, n_diff, n_level, &combos);
  if (rc != BTC_OK) return rc;
  const bool sim = compute_aos && metric_first == 0;
  BTC_CHECK_ARG(frames && pairs && min_overlaps && thresholds && n_thresholds && counts && similarity && ws, "btc_kitti_match_stats: missing pointer");
  BTC_CHECK_ARG((NG == 0 || (ign_gt && gt_rows)) && (ND == 0 || (dt_rows && ign_dt)) && (P == 0 || ov) && (PD == 0 || ov_dc),
                "btc_kitti_match_stats: missing pointer");
  BTC_CHECK_ARG(ws_bytes >= btc_kitti_match_stats_ws_bytes(n_frames, n_class, n_diff, n_level, sim), "btc_kitti_match_stats: workspace too small");
  const int cdk = n_class * n_diff * n_level;
  BTC_HIP(hipMemsetAsync(counts, 0, (size_t)combos * KE_PTS * 3 * sizeof(int32_t), stream));
  if (!sim || n_frames == 0) BTC_HIP(hipMemsetAsync(similarity, 0, (size_t)cdk * KE_PTS * sizeof(double), stream));
  if (n_frames == 0) return BTC_OK;
  MatchArgs a = {};
  a.ov = ov; a.ov_dc = ov_dc; a.gt = gt_rows; a.dt = dt_rows; a.ign_gt = ign_gt; a.ign_dt = ign_dt; a.min_ov = min_overlaps;
  a.thr = thresholds; a.n_thr = n_thresholds; a.frames = frames; a.pairs = pairs; a.P = P;
  a.F = n_frames; a.NG = (int)NG; a.ND = (int)ND; a.m0 = metric_first; a.M = n_metric; a.C = n_class; a.D = n_diff; a.K = n_level;
  a.aos = sim ? 1 : 0;
  a.counts = counts; a.sim_part = (double*)ws;
  kitti_match_stats<<<(unsigned)((long long)n_frames * combos), 64, 0, stream>>>(a);
  BTC_LAUNCH_CHECK();
  if (sim) {
    kitti_sim_reduce<<<btc_cdiv((long long)cdk * KE_PTS, 64), 64, 0, stream>>>(a.sim_part, n_frames, cdk * KE_PTS, similarity);
    BTC_LAUNCH_CHECK();
  }
  return BTC_OK;
}
