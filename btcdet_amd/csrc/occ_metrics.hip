// Occupancy metrics of an eval batch for gfx950 (include/btcdet_hip_infer.h: btc_occ_metrics).
//
// Replaces the reference's Detector3DTemplate.occ_post_processing (detector3d_template.py:479-546 over
// point_box_utils.torch_points_in_box_3d_box_label_batch): five full reductions over the occupancy grid, then per scene a 4x4 matrix
// inverse and an (N, M, 3) einsum, and per threshold and scene a nonzero, a gather, a max and one read-back.  Here a batch is one memset
// and two launches, whatever the number of scenes, boxes and points, and nothing is read back:
//
//   occ_cells   one streaming pass over the probability and the three byte masks, 16 cells per thread and step: the probability as four
//               aligned float4 (a head and a tail are peeled so that the body starts on a 16-byte boundary of `prob`), each mask as 16
//               bytes at whatever address it has (the masks are slices of one byte arena: a byte's alignment is all they promise).  Five
//               counts per thread -> wave64 shuffles -> one 64-bit atomic per workgroup and counter, into the workspace.
//   occ_points  one thread per added occupancy point.  A workgroup walks the scenes its 256 points belong to (one, at a boundary two:
//               PassOccVox writes the points scene by scene; any order is correct), stages that scene's valid boxes in LDS 256 at a time as
//               centre, half extents, cos / sin, and every thread tests its point against the staged boxes.  A point inside a box raises the
//               box's word with an atomicMax of the probability's bit pattern (non-negative floats order like unsigned integers).  The
//               workgroup that draws the last ticket (btc_common.h) counts, per threshold, the valid boxes whose word reached it, and writes
//               the whole row of 16 counters.
#include "btc_common.h"
#include "../../include/btcdet_hip_infer.h"

namespace {

typedef unsigned long long u64;

constexpr int OCC_CELLS_PER_THREAD = 16;
constexpr int OCC_BLOCK = 256;
constexpr int OCC_MAX_BLOCKS = 2048;
constexpr int OCC_BOX_CHUNK = 256;
constexpr int OCC_N_THRESH = 9;

// workspace: [ticket | the five cell counters | one word per (scene, box)], each 256-byte aligned; ONE memset zeroes all of it
struct OccWs {
  int32_t* ticket;
  u64* cells;
  unsigned* box_max;
};

inline size_t occ_ws_head() { return 512; }

struct CellArgs {
  const float* prob;
  const unsigned char* cls;
  const unsigned char* pos;
  const unsigned char* neg;
  long long n, head, groups;   // cells; cells before the first 16-byte boundary of prob; 16-cell groups of the body
  u64* out;                    // [5] total, pos_num, neg_num, pos_predict, pos_correct (zero at launch)
};

// 16 mask bytes at any address
__device__ __forceinline__ void ld16(const unsigned char* p, unsigned w[4]) { __builtin_memcpy(w, p, 16); }

__device__ __forceinline__ void cell1(const CellArgs& a, long long i, unsigned c[5]) {
  const bool hit = a.prob[i] >= 0.5f;   // (a NaN fails)
  const bool pos = a.pos[i] != 0;
  c[0] += a.cls[i] != 0;
  c[1] += pos;
  c[2] += a.neg[i] != 0;
  c[3] += hit;
  c[4] += pos && hit;
}

__global__ __launch_bounds__(OCC_BLOCK) void occ_cells(CellArgs a) {
  __shared__ unsigned s_part[OCC_BLOCK / 64][5];
  const int tid = threadIdx.x;
  unsigned c[5] = {0u, 0u, 0u, 0u, 0u};
  const long long stride = (long long)gridDim.x * OCC_BLOCK;
  for (long long g = (long long)blockIdx.x * OCC_BLOCK + tid; g < a.groups; g += stride) {
    const long long i = a.head + g * OCC_CELLS_PER_THREAD;
    unsigned wc[4], wp[4], wn[4];
    ld16(a.cls + i, wc);
    ld16(a.pos + i, wp);
    ld16(a.neg + i, wn);
    const float4* pv = reinterpret_cast<const float4*>(a.prob + i);   // 16-byte aligned: head cells were peeled
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = pv[q];
      const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool hit = f[e] >= 0.5f;
        const bool pos = ((wp[q] >> (8 * e)) & 0xFFu) != 0;
        c[0] += ((wc[q] >> (8 * e)) & 0xFFu) != 0;
        c[1] += pos;
        c[2] += ((wn[q] >> (8 * e)) & 0xFFu) != 0;
        c[3] += hit;
        c[4] += pos && hit;
      }
    }
  }
  if (blockIdx.x == 0) {   // the peeled cells: < 4 in front, < 16 behind
    const long long tail0 = a.head + a.groups * OCC_CELLS_PER_THREAD;
    if (tid < a.head) cell1(a, tid, c);
    if (tid >= 64 && tail0 + (tid - 64) < a.n) cell1(a, tail0 + (tid - 64), c);
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const unsigned v = btc_wave_sum(c[k]);
    if ((tid & 63) == 0) s_part[tid >> 6][k] = v;
  }
  __syncthreads();
  if (tid < 5) {
    u64 v = 0;
    for (int w = 0; w < OCC_BLOCK / 64; ++w) v += s_part[w][tid];
    if (v) atomicAdd(a.out + tid, v);
  }
}

struct PointArgs {
  const float* pnts;         // (n, 4) x y z probability
  const long long* b_ind;    // (n)
  long long n;
  const float* gt;           // (B, M, stride)
  const int32_t* gt_num;     // (B)
  int B, M, stride;
  const int32_t* pos_all_num;
  OccWs ws;
  float thr[OCC_N_THRESH];
  long long* counters;       // [16]
};

__device__ __forceinline__ int occ_valid_boxes(const PointArgs& a, int b) { return min(max(a.gt_num[b], 0), a.M); }

__global__ __launch_bounds__(OCC_BLOCK) void occ_points(PointArgs a) {
  __shared__ float s_box[OCC_BOX_CHUNK][8];   // cx cy cz hx hy hz cos sin
  __shared__ int s_lo, s_hi;
  __shared__ unsigned s_cnt[OCC_N_THRESH];
  __shared__ u64 s_boxes;
  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * OCC_BLOCK + tid;
  if (tid == 0) {
    s_lo = a.B;
    s_hi = -1;
  }
  __syncthreads();
  int scene = -1;
  float px = 0.f, py = 0.f, pz = 0.f, pr = 0.f;
  if (i < a.n) {
    const long long b = a.b_ind[i];
    const float4 p = *reinterpret_cast<const float4*>(a.pnts + i * 4);
    // below the lowest threshold (or NaN) a point can raise no count: it takes no part
    if (b >= 0 && b < a.B && p.w >= a.thr[0]) {
      scene = (int)b;
      px = p.x; py = p.y; pz = p.z; pr = p.w;
      atomicMin(&s_lo, scene);
      atomicMax(&s_hi, scene);
    }
  }
  __syncthreads();
  const int lo = s_lo, hi = s_hi;
  for (int s = lo; s <= hi; ++s) {            // block-uniform
    const int nb = occ_valid_boxes(a, s);     // rows past gt_boxes_num[s] are never read
    const float* gt = a.gt + (size_t)s * a.M * a.stride;
    unsigned* word = a.ws.box_max + (size_t)s * a.M;
    for (int c0 = 0; c0 < nb; c0 += OCC_BOX_CHUNK) {
      const int cn = min(nb - c0, OCC_BOX_CHUNK);
      if (tid < cn) {
        const float* g = gt + (size_t)(c0 + tid) * a.stride;
        s_box[tid][0] = g[0]; s_box[tid][1] = g[1]; s_box[tid][2] = g[2];
        s_box[tid][3] = g[3] * 0.5f; s_box[tid][4] = g[4] * 0.5f; s_box[tid][5] = g[5] * 0.5f;
        s_box[tid][6] = cosf(g[6]); s_box[tid][7] = sinf(g[6]);
      }
      __syncthreads();
      if (scene == s) {
        for (int j = 0; j < cn; ++j) {
          const float dx = px - s_box[j][0], dy = py - s_box[j][1], dz = pz - s_box[j][2];
          const float cs = s_box[j][6], sn = s_box[j][7];
          const float lx = dx * cs + dy * sn, ly = dy * cs - dx * sn;
          // both faces inclusive; a NaN is outside
          if (fabsf(lx) <= s_box[j][3] && fabsf(ly) <= s_box[j][4] && fabsf(dz) <= s_box[j][5]) atomicMax(word + c0 + j, __float_as_uint(pr));
        }
      }
      __syncthreads();
    }
  }
  // last-arriver hand-over (btc_common.h): the payload here is the atomics; the acquiring lane then waits for its invalidate before
  // the workgroup meets again below
  if (!btc_last_arriver(a.ws.ticket, (int)gridDim.x)) return;
  if (tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_boxes = 0ull;
  }
  if (tid < OCC_N_THRESH) s_cnt[tid] = 0u;
  __syncthreads();
  unsigned cnt[OCC_N_THRESH];
#pragma unroll
  for (int t = 0; t < OCC_N_THRESH; ++t) cnt[t] = 0u;
  const long long words = (long long)a.B * a.M;
  for (long long w = tid; w < words; w += OCC_BLOCK) {
    const int b = (int)(w / a.M), j = (int)(w - (long long)b * a.M);
    if (j >= occ_valid_boxes(a, b)) continue;
    const float best = __uint_as_float(btc_ld_agent(a.ws.box_max + w));
#pragma unroll
    for (int t = 0; t < OCC_N_THRESH; ++t) cnt[t] += best >= a.thr[t];
  }
#pragma unroll
  for (int t = 0; t < OCC_N_THRESH; ++t) {
    const unsigned v = btc_wave_sum(cnt[t]);
    if ((tid & 63) == 0 && v) atomicAdd(&s_cnt[t], v);
  }
  u64 nb = 0;
  for (int b = tid; b < a.B; b += OCC_BLOCK) nb += (u64)occ_valid_boxes(a, b);
  if (nb) atomicAdd(&s_boxes, nb);
  __syncthreads();
  if (tid < 5) a.counters[tid] = (long long)btc_ld_agent(a.ws.cells + tid);
  if (tid == 5) a.counters[5] = (long long)a.pos_all_num[0];
  if (tid == 6) a.counters[6] = (long long)s_boxes;
  if (tid >= 7 && tid < 16) a.counters[tid] = (long long)s_cnt[tid - 7];
}

OccWs occ_carve(void* ws) {
  OccWs w;
  w.ticket = (int32_t*)ws;
  w.cells = (u64*)((char*)ws + 256);
  w.box_max = (unsigned*)((char*)ws + occ_ws_head());
  return w;
}

}  // namespace

extern "C" size_t btc_occ_metrics_ws_bytes(int batch, int max_boxes) {
  const size_t words = (batch > 0 && max_boxes > 0) ? (size_t)batch * (size_t)max_boxes : 0;
  return occ_ws_head() + btc_align(words * sizeof(unsigned));
}

extern "C" int btc_occ_metrics(const float* prob, const uint8_t* cls_mask, const uint8_t* pos_mask, const uint8_t* neg_mask, long long n_cells,
                               const int32_t* pos_all_num, const float* occ_pnts, const long long* occ_b_ind, long long n_points,
                               const float* gt_boxes, const int32_t* gt_boxes_num, int batch, int max_boxes, int gt_stride, long long* counters,
                               void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(n_cells >= 0 && n_points >= 0 && batch >= 0 && max_boxes >= 0, "btc_occ_metrics: bad sizes (%lld cells, %lld points, batch %d, %d boxes)",
                n_cells, n_points, batch, max_boxes);
  BTC_CHECK_ARG(n_cells == 0 || (prob && cls_mask && pos_mask && neg_mask), "btc_occ_metrics: missing pointer (probability or mask)");
  BTC_CHECK_ARG(((uintptr_t)prob & 3) == 0, "btc_occ_metrics: prob is not aligned to a float");
  BTC_CHECK_ARG(n_points == 0 || (occ_pnts && occ_b_ind), "btc_occ_metrics: missing pointer (points)");
  BTC_CHECK_ARG(((uintptr_t)occ_pnts & 15) == 0, "btc_occ_metrics: occ_pnts is not aligned to 16 bytes");
  BTC_CHECK_ARG(batch == 0 || gt_boxes_num, "btc_occ_metrics: missing pointer (gt_boxes_num)");
  BTC_CHECK_ARG(batch == 0 || max_boxes == 0 || (gt_boxes && gt_stride >= 7), "btc_occ_metrics: bad ground truth (%d rows of %d values)", max_boxes,
                gt_stride);
  BTC_CHECK_ARG(pos_all_num && counters && ws, "btc_occ_metrics: missing pointer (pos_all_num, counters or workspace)");
  BTC_CHECK_ARG(((uintptr_t)ws & 7) == 0 && ((uintptr_t)counters & 7) == 0, "btc_occ_metrics: counters / workspace not aligned to 8 bytes");
  const long long pblocks = (n_points + OCC_BLOCK - 1) / OCC_BLOCK;
  BTC_CHECK_ARG(pblocks <= 0x7FFFFFFFll, "btc_occ_metrics: %lld points exceed one launch", n_points);
  const size_t need = btc_occ_metrics_ws_bytes(batch, max_boxes);
  BTC_CHECK_ARG(ws_bytes >= need, "btc_occ_metrics: workspace too small (%zu < %zu)", ws_bytes, need);
  const OccWs w = occ_carve(ws);
  BTC_HIP(hipMemsetAsync(ws, 0, need, stream));   // the workspace arrives as garbage
  if (n_cells > 0) {
    CellArgs c;
    c.prob = prob; c.cls = cls_mask; c.pos = pos_mask; c.neg = neg_mask; c.n = n_cells;
    c.head = (long long)(((16 - ((uintptr_t)prob & 15)) & 15) / 4);
    if (c.head > n_cells) c.head = n_cells;
    c.groups = (n_cells - c.head) / OCC_CELLS_PER_THREAD;
    c.out = w.cells;
    long long blocks = (c.groups + OCC_BLOCK - 1) / OCC_BLOCK;
    blocks = blocks < 1 ? 1 : (blocks > OCC_MAX_BLOCKS ? OCC_MAX_BLOCKS : blocks);
    occ_cells<<<(int)blocks, OCC_BLOCK, 0, stream>>>(c);
    BTC_LAUNCH_CHECK();
  }
  PointArgs p;
  p.pnts = occ_pnts; p.b_ind = occ_b_ind; p.n = n_points; p.gt = gt_boxes; p.gt_num = gt_boxes_num; p.B = batch; p.M = max_boxes;
  p.stride = gt_stride; p.pos_all_num = pos_all_num; p.ws = w; p.counters = counters;
  for (int i = 1; i <= OCC_N_THRESH; ++i) p.thr[i - 1] = (float)(i * 0.1);   // the product in double, then rounded: torch's float32 scalar
  occ_points<<<(int)(pblocks < 1 ? 1 : pblocks), OCC_BLOCK, 0, stream>>>(p);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}
