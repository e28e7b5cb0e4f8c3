// The best-match templates of a class from the resident objects of a ground-truth database for gfx950 (include/btcdet_hip_templates.h:
// btc_nn_sqdist, btc_match_candidates, btc_select_templates).
//
//   tm_nn        one workgroup per (query segment, target segment) pair: 256 query rows at a time, one per lane, against the target staged
//                in LDS 256 rows at a time (tm_nn_segment, the device function the greedy filter below uses too).
//   tm_match     one workgroup per (object, TM_CPB candidates).  The object's rows stay in registers, TM_QR per lane; a candidate's rows go
//                through LDS in tiles of TM_TILE float4 and every lane reads row k of the tile at the same address -- a broadcast, no bank
//                conflict -- for a running minimum per query row; the thread that stages a row also tests it against the object's box and
//                sets its cell's bit in an LDS bitmap with atomicOr.  Workgroup maximum, one sqrt, the bitmap written out whole.
//   tsel_pick    one workgroup per object: popcounts and the argmin over K, the nearest-neighbour filter of the winner against the
//                growing set (own rows + the flagged rows of earlier winners), flag bytes and the template's size into the workspace.
//   tsel_offsets one wave ranks the templates' sizes -> tmpl_offsets.
//   tsel_write   one workgroup per object copies its rows and compacts the flagged rows of every chosen winner behind them, in order.
//
// tm_match is bound by the VALU: per (query row, candidate row) three subtractions, three multiplications, two additions and a minimum
// -- nine float32 operations, none contracted (the header holds d2 to separately rounded steps) -- against one 16-byte LDS broadcast per
// TM_QR of them.  Every index formed from a device array is clamped to n, M, K or capacity before it addresses anything.
#include "btc_common.h"

#include "../../include/btcdet_hip_templates.h"

namespace {

constexpr int TM_T = 256;        // threads of every workgroup here
constexpr int TM_WAVES = TM_T / 64;
constexpr int TM_QR = 4;         // query rows a lane of tm_match holds: TM_T * TM_QR = 1024 per pass
constexpr int TM_TILE = 512;     // candidate rows per LDS tile of tm_match
constexpr int TM_NN_TILE = 256;  // target rows per LDS tile of tm_nn_segment
constexpr int TM_CPB = 8;        // candidates per workgroup of tm_match
constexpr int TM_MAXW = 2048;    // bitmap words an LDS bitmap holds
constexpr int TM_MAXK = 8192;    // candidates tsel_pick keeps alive flags for
constexpr int TM_MAXBM = 8;

__device__ __forceinline__ float tm_d2(float px, float py, float pz, float qx, float qy, float qz) {
  const float dx = px - qx, dy = py - qy, dz = pz - qz;
  return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// rows [first, first + rows) of segment j, clamped to [0, n] (and to `cap` rows); j outside [0, M) -> empty
__device__ __forceinline__ void tm_span(const int32_t* __restrict__ seg, int j, int M, int n, int cap, int& first, int& rows) {
  first = 0, rows = 0;
  if (j < 0 || j >= M) return;
  first = min(max(seg[2 * j], 0), n);
  rows = min(min(max(seg[2 * j + 1], 0), n - first), cap);
}

// Every thread of the workgroup calls it (two barriers per tile).  -> min(m, the smallest d2 of (qx, qy, qz) against rows
// [first, first + rows) of pts); flags != NULL: a row whose flag byte is 0 is skipped.
__device__ __forceinline__ float tm_nn_segment(float qx, float qy, float qz, const float* __restrict__ pts, int first, int rows,
                                               const unsigned char* flags, float4* __restrict__ s_tile, float m) {
  for (int t0 = 0; t0 < rows; t0 += TM_NN_TILE) {
    const int nt = min(TM_NN_TILE, rows - t0);
    __syncthreads();   // the previous tile has been read
    for (int k = threadIdx.x; k < nt; k += TM_T) {
      const float* p = pts + (size_t)(first + t0 + k) * 3;
      const bool on = !flags || flags[t0 + k] != 0;
      s_tile[k] = make_float4(on ? p[0] : INFINITY, p[1], p[2], 0.f);   // dx = inf -> d2 = inf: never the minimum
    }
    __syncthreads();
    for (int k = 0; k < nt; ++k) {
      const float4 p = s_tile[k];
      m = fminf(m, tm_d2(p.x, p.y, p.z, qx, qy, qz));
    }
  }
  return m;
}

__global__ __launch_bounds__(TM_T) void tm_nn(const float* __restrict__ q_points, int nq, const float* __restrict__ t_points, int nt,
                                              const int32_t* __restrict__ pairs, const int32_t* __restrict__ out_offsets, int out_rows,
                                              float* __restrict__ out) {
  __shared__ float4 s_tile[TM_NN_TILE];
  const int p = blockIdx.x;
  const int q_first = pairs[4 * p], q_rows = pairs[4 * p + 1];
  const int t_first = min(max(pairs[4 * p + 2], 0), nt);
  const int t_rows = min(max(pairs[4 * p + 3], 0), nt - t_first);
  const long long o0 = out_offsets[p];
  for (int r0 = 0; r0 < q_rows; r0 += TM_T) {   // uniform in the workgroup
    const int r = r0 + threadIdx.x;
    const long long qi = (long long)q_first + r, dst = o0 + r;
    const bool live = r < q_rows && qi >= 0 && qi < nq && dst >= 0 && dst < out_rows;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) qx = q_points[qi * 3], qy = q_points[qi * 3 + 1], qz = q_points[qi * 3 + 2];
    const float m = tm_nn_segment(qx, qy, qz, t_points, t_first, t_rows, nullptr, s_tile, INFINITY);
    if (live) out[dst] = m;
  }
}

struct TmGrid {
  float x0, y0, cell;
  int nx, ny, W;
};

// the bit of (x, y), or -1 when the row is outside the grid
__device__ __forceinline__ int tm_cell_bit(const TmGrid& gr, float x, float y) {
  const float fx = floorf((x - gr.x0) / gr.cell), fy = floorf((y - gr.y0) / gr.cell);
  if (!(fx >= 0.f && fx < (float)gr.nx && fy >= 0.f && fy < (float)gr.ny)) return -1;
  return (int)fx * gr.ny + (int)fy;
}

__global__ __launch_bounds__(TM_T) void tm_match(const float* __restrict__ pts, int n, const int32_t* __restrict__ seg,
                                                 const float* __restrict__ half, int M, const int32_t* __restrict__ obj,
                                                 const int32_t* __restrict__ cand, int G, int K, TmGrid gr, float* __restrict__ max_dist,
                                                 uint32_t* __restrict__ sel_occ) {
  __shared__ float4 s_t[TM_TILE];
  __shared__ unsigned s_bits[TM_MAXW];
  __shared__ float s_wmax[TM_WAVES];
  const int groups = (K + TM_CPB - 1) / TM_CPB;
  const int g = blockIdx.x / groups, k0 = (blockIdx.x % groups) * TM_CPB;
  const int tid = threadIdx.x;
  int i = obj[g];
  if (i < 0 || i >= M) i = -1;
  int q_first, q_rows;
  tm_span(seg, i, M, n, n, q_first, q_rows);
  float hx = 0.f, hy = 0.f, hz = 0.f;
  if (i >= 0) hx = half[3 * i], hy = half[3 * i + 1], hz = half[3 * i + 2];
  const int npass = max((q_rows + TM_T * TM_QR - 1) / (TM_T * TM_QR), 1);
  for (int k = k0; k < min(k0 + TM_CPB, K); ++k) {
    const size_t pair = (size_t)g * K + k;
    int c = cand[pair];
    if (i < 0 || c < 0 || c >= M) {   // uniform in the workgroup
      if (tid == 0) max_dist[pair] = INFINITY;
      for (int w = tid; w < gr.W; w += TM_T) sel_occ[pair * gr.W + w] = 0u;
      continue;
    }
    int t_first, t_rows;
    tm_span(seg, c, M, n, n, t_first, t_rows);
    for (int w = tid; w < gr.W; w += TM_T) s_bits[w] = 0u;   // ordered before the first atomicOr by the tile loop's barrier
    float run = 0.f;                                         // the largest minimum of this lane's rows, as d2
    for (int pass = 0; pass < npass; ++pass) {
      float qx[TM_QR], qy[TM_QR], qz[TM_QR], m[TM_QR];
      bool live[TM_QR];
#pragma unroll
      for (int j = 0; j < TM_QR; ++j) {
        const int r = (pass * TM_QR + j) * TM_T + tid;
        live[j] = r < q_rows;
        const float* p = pts + (size_t)(q_first + (live[j] ? r : 0)) * 3;
        qx[j] = live[j] ? p[0] : 0.f, qy[j] = live[j] ? p[1] : 0.f, qz[j] = live[j] ? p[2] : 0.f;
        m[j] = INFINITY;
      }
      for (int t0 = 0; t0 < t_rows; t0 += TM_TILE) {
        const int nt = min(TM_TILE, t_rows - t0);
        __syncthreads();   // the previous tile has been read
        for (int r = tid; r < nt; r += TM_T) {
          const float* p = pts + (size_t)(t_first + t0 + r) * 3;
          const float x = p[0], y = p[1], z = p[2];
          s_t[r] = make_float4(x, y, z, 0.f);
          if (pass == 0 && fabsf(x) <= hx && fabsf(y) <= hy && fabsf(z) <= hz) {
            const int b = tm_cell_bit(gr, x, y);
            if (b >= 0) atomicOr(&s_bits[b >> 5], 1u << (b & 31));
          }
        }
        __syncthreads();
        for (int r = 0; r < nt; ++r) {
          const float4 p = s_t[r];
#pragma unroll
          for (int j = 0; j < TM_QR; ++j) m[j] = fminf(m[j], tm_d2(qx[j], qy[j], qz[j], p.x, p.y, p.z));
        }
      }
#pragma unroll
      for (int j = 0; j < TM_QR; ++j)
        if (live[j]) run = fmaxf(run, m[j]);
    }
    run = btc_wave_allreduce(run, [](float a, float b) { return fmaxf(a, b); });
    if ((tid & 63) == 0) s_wmax[tid >> 6] = run;
    __syncthreads();   // s_wmax and every bit of s_bits
    if (tid == 0) {
      float v = s_wmax[0];
      for (int w = 1; w < TM_WAVES; ++w) v = fmaxf(v, s_wmax[w]);
      max_dist[pair] = sqrtf(v);
    }
    for (int w = tid; w < gr.W; w += TM_T) sel_occ[pair * gr.W + w] = s_bits[w];
    __syncthreads();   // before the next candidate clears s_bits and s_wmax
  }
}

// ---- the greedy rounds
struct TselBest {
  float h;
  int k, extra;
};
__device__ __forceinline__ bool tsel_better(const TselBest& a, const TselBest& b) {   // a before b: smaller h, the lower k among equals
  return a.k >= 0 && (b.k < 0 || a.h < b.h || (a.h == b.h && a.k < b.k));
}

__global__ __launch_bounds__(TM_T) void tsel_pick(const float* __restrict__ pts, int n, const int32_t* __restrict__ seg, int M,
                                                  const int32_t* __restrict__ obj, const int32_t* __restrict__ cand,
                                                  const float* __restrict__ iou, const float* __restrict__ max_dist,
                                                  const uint32_t* __restrict__ sel_occ, const uint32_t* __restrict__ own_occ, int K, int W,
                                                  int max_bm, int num_extra, float iou_thresh, float ratio, float nearest_sq, int max_rows,
                                                  int32_t* __restrict__ chosen, unsigned char* __restrict__ flags, int32_t* __restrict__ total) {
  __shared__ float4 s_tile[TM_NN_TILE];
  __shared__ unsigned s_aug[TM_MAXW];
  __shared__ unsigned char s_alive[TM_MAXK];
  __shared__ TselBest s_best[TM_WAVES];
  __shared__ int s_red[TM_WAVES];
  __shared__ int s_del[TM_MAXBM], s_src;   // the winners of earlier rounds; the place in the list this round's rows come from
  __shared__ int s_set_obj[TM_MAXBM + 1], s_set_round[TM_MAXBM + 1];   // the growing set: segment s = the rows of s_set_obj[s] flagged in round s_set_round[s] (-1: all)
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int i = obj[g];
  if (i < 0 || i >= M) i = -1;
  int own_first, own_rows;
  tm_span(seg, i, M, n, max_rows, own_first, own_rows);
  const int32_t* my_cand = cand + (size_t)g * K;
  int alive = 0;
  for (int k = tid; k < K; k += TM_T) {
    const int c = my_cand[k];
    const bool on = i >= 0 && c >= 0 && c < M;
    s_alive[k] = on;
    alive += on;
  }
  alive = btc_wave_all_sum(alive);
  if (lane == 0) s_red[wave] = alive;
  for (int w = tid; w < W; w += TM_T) s_aug[w] = i >= 0 ? own_occ[(size_t)i * W + w] : 0u;
  for (int r = tid; r < max_bm; r += TM_T) chosen[(size_t)g * max_bm + r] = -1;
  if (tid == 0) s_set_obj[0] = i, s_set_round[0] = -1;
  __syncthreads();
  alive = 0;
  for (int w = 0; w < TM_WAVES; ++w) alive += s_red[w];
  __syncthreads();   // s_red has been read
  int set_segs = 1, set_rows = own_rows, aug_num = 0, n_del = 0;
  for (int round = 0; round < max_bm && alive > 0; ++round) {
    TselBest best = {INFINITY, -1, 0};
    for (int k = tid; k < K; k += TM_T) {
      if (s_alive[k] != 1) continue;
      const uint32_t* so = sel_occ + ((size_t)g * K + k) * W;
      int extra = 0;
      for (int w = 0; w < W; ++w) extra += __popc(so[w] & ~s_aug[w]);
      const float io = iou[(size_t)g * K + k];
      const float h = ((max_dist[(size_t)g * K + k] + ratio / (float)extra) + (io < iou_thresh ? 2.f : 0.f)) + (extra < 30 ? 1.f : 0.f);
      const TselBest mine = {h, k, extra};
      if (h == h && tsel_better(mine, best)) best = mine;
    }
    for (int o = 32; o > 0; o >>= 1) {
      TselBest other = {__shfl_xor(best.h, o), __shfl_xor(best.k, o), __shfl_xor(best.extra, o)};
      if (tsel_better(other, best)) best = other;
    }
    if (lane == 0) s_best[wave] = best;
    __syncthreads();
    best = s_best[0];
    for (int w = 1; w < TM_WAVES; ++w)
      if (tsel_better(s_best[w], best)) best = s_best[w];
    __syncthreads();
    if (best.k < 0) break;                                                   // uniform: every thread read the same s_best
    if ((iou[(size_t)g * K + best.k] < iou_thresh && set_rows > 0) || best.extra == 0) break;
    if (tid == 0) {   // the rows come from the candidate as many listed places in front of the winner as deleted winners stand in front of it
      int p = best.k;
      for (int d = 0; d < n_del; ++d)
        if (s_del[d] < best.k) {
          do --p;
          while (p > 0 && s_alive[p] == 0);
        }
      s_src = p;
    }
    __syncthreads();
    const int c = my_cand[s_src];
    int c_first, c_rows;
    tm_span(seg, c, M, n, max_rows, c_first, c_rows);
    unsigned char* my_flags = flags + ((size_t)g * max_bm + round) * max_rows;
    int added = 0;
    for (int r0 = 0; r0 < c_rows; r0 += TM_T) {
      const int r = r0 + tid;
      const bool live = r < c_rows;
      const float* p = pts + (size_t)(c_first + (live ? r : 0)) * 3;
      const float qx = p[0], qy = p[1], qz = p[2];
      float m = INFINITY;
      for (int s = 0; s < set_segs; ++s) {
        int f, rows;
        tm_span(seg, s_set_obj[s], M, n, max_rows, f, rows);
        const int sr = s_set_round[s];
        m = tm_nn_segment(qx, qy, qz, pts, f, rows, sr < 0 ? nullptr : flags + ((size_t)g * max_bm + sr) * max_rows, s_tile, m);
      }
      const bool keep = live && m > nearest_sq;
      if (live) my_flags[r] = keep;
      added += __syncthreads_count(keep);
    }
    if (added > 4) {
      if (tid == 0) {
        chosen[(size_t)g * max_bm + round] = c;
        s_set_obj[set_segs] = c, s_set_round[set_segs] = round;
      }
      set_segs += 1, set_rows += added;
      const uint32_t* so = sel_occ + ((size_t)g * K + best.k) * W;
      int bits = 0;
      for (int w = tid; w < W; w += TM_T) {
        const unsigned v = s_aug[w] | so[w];
        s_aug[w] = v;
        bits += __popc(v);
      }
      bits = btc_wave_all_sum(bits);
      if (lane == 0) s_red[wave] = bits;
      __syncthreads();   // s_red, s_aug, s_set_*, and this round's flag bytes
      aug_num = 0;
      for (int w = 0; w < TM_WAVES; ++w) aug_num += s_red[w];
    }
    if (alive == 1 || aug_num >= num_extra) break;
    if (tid == 0) s_alive[best.k] = 2, s_del[n_del] = best.k;   // 2: listed, no longer alive
    alive -= 1, n_del += 1;
    __syncthreads();
  }
  if (tid == 0) total[g] = set_rows;
}

// tmpl_offsets[g] = rows of the templates in front of template g, tmpl_offsets[G] = all
__global__ __launch_bounds__(64) void tsel_offsets(const int32_t* __restrict__ total, int G, int32_t* __restrict__ tmpl_offsets) {
  btc_wave_offsets_of_counts(total, G, tmpl_offsets);
}

__global__ __launch_bounds__(TM_T) void tsel_write(const float* __restrict__ pts, int n, const int32_t* __restrict__ seg, int M,
                                                   const int32_t* __restrict__ obj, int max_bm, int max_rows,
                                                   const int32_t* __restrict__ chosen, const unsigned char* __restrict__ flags,
                                                   const int32_t* __restrict__ tmpl_offsets, int capacity, float* __restrict__ out,
                                                   int32_t* __restrict__ src) {
  __shared__ int s_wcnt[TM_WAVES];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long base = tmpl_offsets[g];
  for (int s = 0; s <= max_bm; ++s) {
    const int j = s == 0 ? obj[g] : chosen[(size_t)g * max_bm + s - 1];
    int first, rows;
    tm_span(seg, j, M, n, max_rows, first, rows);
    const unsigned char* fl = s == 0 ? nullptr : flags + ((size_t)g * max_bm + s - 1) * max_rows;
    for (int r0 = 0; r0 < rows; r0 += TM_T) {   // uniform in the workgroup
      const int r = r0 + tid;
      const bool keep = r < rows && (!fl || fl[r] != 0);
      const unsigned long long mk = __ballot(keep);
      if (lane == 0) s_wcnt[wave] = __popcll(mk);
      __syncthreads();
      long long dst = base + __popcll(mk & ((1ull << lane) - 1ull));
      int all = 0;
      for (int w = 0; w < TM_WAVES; ++w) {
        if (w < wave) dst += s_wcnt[w];
        all += s_wcnt[w];
      }
      if (keep && dst >= 0 && dst < capacity) {
        const float* p = pts + (size_t)(first + r) * 3;
        out[dst * 3] = p[0], out[dst * 3 + 1] = p[1], out[dst * 3 + 2] = p[2];
        if (src) src[dst * 2] = j, src[dst * 2 + 1] = r;
      }
      base += all;
      __syncthreads();   // s_wcnt has been read
    }
  }
}

inline bool tsel_sizes_ok(int G, int max_bm, int max_rows) {
  return G >= 0 && max_bm >= 1 && max_bm <= TM_MAXBM && max_rows >= 0 && (long long)G * (max_bm + 1) * (long long)max_rows < (1ll << 31);
}

}  // namespace

extern "C" int btc_nn_sqdist(const float* q_points, int nq, const float* t_points, int nt, const int32_t* pairs, const int32_t* out_offsets, int P,
                             int out_rows, float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(P >= 0 && nq >= 0 && nt >= 0 && out_rows >= 0, "btc_nn_sqdist: negative count (P %d, nq %d, nt %d, out_rows %d)", P, nq, nt, out_rows);
  BTC_CHECK_ARG((pairs && out_offsets) || P == 0, "btc_nn_sqdist: missing pointer (pairs or out_offsets)");
  BTC_CHECK_ARG(q_points || nq == 0, "btc_nn_sqdist: missing pointer (q_points)");
  BTC_CHECK_ARG(t_points || nt == 0, "btc_nn_sqdist: missing pointer (t_points)");
  BTC_CHECK_ARG(out || out_rows == 0, "btc_nn_sqdist: missing pointer (out)");
  if (P == 0 || out_rows == 0 || nq == 0) return BTC_OK;
  tm_nn<<<P, TM_T, 0, stream>>>(q_points, nq, t_points, nt, pairs, out_offsets, out_rows, out);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}

extern "C" int btc_match_candidates(const float* points, int n, const int32_t* seg, const float* half, int M, const int32_t* obj, const int32_t* cand,
                                    int G, int K, float x0, float y0, float cell, int nx, int ny, float* max_dist, uint32_t* sel_occ,
                                    void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(n >= 0 && M >= 0 && G >= 0, "btc_match_candidates: negative count (n %d, M %d, G %d)", n, M, G);
  BTC_CHECK_ARG(K >= 1, "btc_match_candidates: need K >= 1, got %d", K);
  BTC_CHECK_ARG(nx >= 1 && ny >= 1 && cell > 0.f, "btc_match_candidates: need a grid of nx, ny >= 1 cells of size > 0 (nx %d, ny %d, cell %g)", nx, ny,
                (double)cell);
  const long long words = ((long long)nx * ny + 31) / 32;
  BTC_CHECK_ARG(words <= TM_MAXW, "btc_match_candidates: a bitmap of %lld words, at most %d", words, TM_MAXW);
  const int groups = (K + TM_CPB - 1) / TM_CPB;
  BTC_CHECK_ARG((long long)G * K * words < (1ll << 31) && (long long)G * groups < (1ll << 31), "btc_match_candidates: G * K * W does not fit 31 bits");
  BTC_CHECK_ARG((obj && cand && max_dist && sel_occ) || G == 0, "btc_match_candidates: missing pointer (obj, cand, max_dist or sel_occ)");
  BTC_CHECK_ARG((seg && half) || M == 0, "btc_match_candidates: missing pointer (seg or half)");
  BTC_CHECK_ARG(points || n == 0, "btc_match_candidates: missing pointer (points)");
  if (G == 0) return BTC_OK;
  const TmGrid gr = {x0, y0, cell, nx, ny, (int)words};
  tm_match<<<G * groups, TM_T, 0, stream>>>(points, n, seg, half, M, obj, cand, G, K, gr, max_dist, sel_occ);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}

extern "C" size_t btc_select_templates_ws_bytes(int G, int max_num_bm, int max_rows) {
  if (!tsel_sizes_ok(G, max_num_bm, max_rows)) return 0;
  const size_t rounds = (size_t)(G > 0 ? G : 1) * max_num_bm;
  return btc_align(rounds * (size_t)(max_rows > 0 ? max_rows : 1)) + btc_align((size_t)(G > 0 ? G : 1) * sizeof(int32_t));   // flags, total
}

extern "C" int btc_select_templates(const float* points, int n, const int32_t* seg, int M, const int32_t* obj, const int32_t* cand, const float* iou,
                                    const float* max_dist, const uint32_t* sel_occ, const uint32_t* own_occ, int G, int K, int W, int max_num_bm,
                                    int num_extra_coords, float iou_thresh, float ratio, float nearest_sq, int max_rows, int capacity, float* out,
                                    int32_t* src, int32_t* tmpl_offsets, int32_t* chosen, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(G >= 0 && M >= 0 && n >= 0 && capacity >= 0 && max_rows >= 0 && num_extra_coords >= 0,
                "btc_select_templates: negative count (G %d, M %d, n %d, capacity %d, max_rows %d, num_extra_coords %d)", G, M, n, capacity, max_rows,
                num_extra_coords);
  BTC_CHECK_ARG(K >= 1 && K <= TM_MAXK, "btc_select_templates: need 1 <= K <= %d, got %d", TM_MAXK, K);
  BTC_CHECK_ARG(W >= 1 && W <= TM_MAXW, "btc_select_templates: need 1 <= W <= %d, got %d", TM_MAXW, W);
  BTC_CHECK_ARG(max_num_bm >= 1 && max_num_bm <= TM_MAXBM, "btc_select_templates: need 1 <= max_num_bm <= %d, got %d", TM_MAXBM, max_num_bm);
  BTC_CHECK_ARG(tsel_sizes_ok(G, max_num_bm, max_rows), "btc_select_templates: G * (max_num_bm + 1) * max_rows does not fit 31 bits");
  BTC_CHECK_ARG(tmpl_offsets && chosen && ws, "btc_select_templates: missing pointer (tmpl_offsets, chosen or ws)");
  BTC_CHECK_ARG((obj && cand && iou && max_dist && sel_occ) || G == 0, "btc_select_templates: missing pointer (obj, cand, iou, max_dist or sel_occ)");
  BTC_CHECK_ARG((seg && own_occ) || M == 0, "btc_select_templates: missing pointer (seg or own_occ)");
  BTC_CHECK_ARG(points || n == 0, "btc_select_templates: missing pointer (points)");
  BTC_CHECK_ARG(out || capacity == 0, "btc_select_templates: missing pointer (out)");
  BTC_CHECK_ARG(ws_bytes >= btc_select_templates_ws_bytes(G, max_num_bm, max_rows), "btc_select_templates: workspace too small");
  BtcCarver c(ws);
  const size_t rounds = (size_t)(G > 0 ? G : 1) * max_num_bm;
  unsigned char* flags = c.take<unsigned char>(rounds * (size_t)(max_rows > 0 ? max_rows : 1));
  int32_t* total = c.take<int32_t>(G > 0 ? G : 1);
  if (G > 0) {
    tsel_pick<<<G, TM_T, 0, stream>>>(points, n, seg, M, obj, cand, iou, max_dist, sel_occ, own_occ, K, W, max_num_bm, num_extra_coords, iou_thresh,
                                      ratio, nearest_sq, max_rows, chosen, flags, total);
    BTC_LAUNCH_CHECK();
  }
  tsel_offsets<<<1, 64, 0, stream>>>(total, G, tmpl_offsets);
  BTC_LAUNCH_CHECK();
  if (G > 0 && capacity > 0) {
    tsel_write<<<G, TM_T, 0, stream>>>(points, n, seg, M, obj, max_num_bm, max_rows, chosen, flags, tmpl_offsets, capacity, out, src);
    BTC_LAUNCH_CHECK();
  }
  return BTC_OK;
}
