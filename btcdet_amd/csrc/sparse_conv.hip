// Sparse convolution apply for gfx950: fused, output-stationary implicit GEMM on the fp32 MFMA pipe.
//
// Replaces spconv's indice_conv / indice_subm_conv / indice_inverse_conv (one gather + mm +
// scatter-add launch triple PER KERNEL OFFSET) with ONE launch per layer:
// a workgroup owns 64 output rows, walks the K offsets of the neighbour map, gathers the rows
// that exist into LDS, and accumulates  acc += A_k (64 x Cin) * W[k] (Cin x Cout)  with
// v_mfma_f32_16x16x4_f32.  No atomics, no per-offset temporaries; the summation order is fixed
// (offset ascending, channel ascending) and the f32 MFMA is an exact fmaf chain, so results are
// bit-reproducible and equal to the CPU oracle's fmaf chain.
//
// Roofline: HBM/L2 bound at BtcDet's channel widths: per output row the kernel
// moves (pairs * Cin + Cout) * 4 B and does 2 * pairs * Cin * Cout flop.
//
// Forward, data gradient, max-pool and to-dense live here; the weight gradient is in conv_wgrad.hip.
#include "conv_tile.h"

namespace {

constexpr int KC = 32;       // reduction-channel chunk staged in LDS
constexpr int LDA = KC + 2;  // bank-conflict-free A fragment reads (ds_read_b32, 2 x 32-lane groups)

// out[i] = bias + sum_k feat[nbr[i][k]] @ Wk     (TRANS_W = false: Wk = W[k]      (Cin x Cout), fwd)
// din[j] =        sum_k dout[nbr[j][k]] @ Wk     (TRANS_W = true : Wk = W[k]^T    (Cout x Cin), dgrad)
// Cred = reduction channels, Cres = result channels; W is always stored [K][Cin][Cout].
//
// Work items = (active offset k, 32-channel chunk).  Register-staged software pipeline: the global loads of item
// i+1 (gathered rows + weight panel) are issued before the MFMAs of item i and land in registers while the matrix
// pipe runs; all loads of an item are issued back to back (one memory latency per item, not one per element).
template <int NT, bool TRANS_W, bool VEC, int KB, int THREADS>
__global__ __launch_bounds__(THREADS) void conv_apply(const float* __restrict__ feat, const float* __restrict__ W,
                                                  const float* __restrict__ bias, const int32_t* __restrict__ nbr,
                                                  int n_rows, int K, int Cred, int Cres, float* __restrict__ out, int mirror, const BnFuse bn) {
  // mirror: `nbr` is a submanifold layer's forward map read as its backward map -- column K-1-k holds offset k (rulebook.hip)
  // bn: batch statistics of the result for the BatchNorm behind this layer, gathered in the epilogue (bn_fuse.h)
  // KB > 1 (narrow layers, Cred <= 32: one chunk per offset): KB active offsets are staged per phase, which divides the
  // number of barrier-separated phases by KB and multiplies the loads in flight per workgroup by KB.
  // THREADS = 256 / 128 / 64 -> 64 / 32 / 16 output rows per workgroup (one 16-row MFMA slab per wave): small and
  // mid-size layers do not have enough 64-row tiles to hide memory latency by occupancy, so they get smaller workgroups.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TM = THREADS / 4;                   // rows per workgroup (shadows the file-level TM)
  constexpr int LDB = ldb_of(NT);
  constexpr int NB = NT * 512 / THREADS;            // weight-panel floats per thread and offset (KC * NT*16 / THREADS)
  float* As = (float*)smem;                         // [KB][TM][LDA]
  float* Bs = As + KB * TM * LDA;                   // [KB][KC][LDB]
  int32_t* s_nbr = (int32_t*)(Bs + KB * KC * LDB);  // [TM][K]
  int32_t* s_kact = s_nbr + TM * K;                 // [K] flags, then the compact list of active offsets
  int32_t* s_nact = s_kact + K;                     // [1]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.x * TM;
  const int n0 = blockIdx.y * (NT * 16);

  for (int e = tid; e < K; e += THREADS) s_kact[e] = 0;
  __syncthreads();
  {
    const long long gbase = (long long)row0 * K;
    const long long gend = (long long)n_rows * K;
    for (int e = tid; e < TM * K; e += THREADS) {
      const int kk = e % K;
      int v = (gbase + e < gend) ? nbr[mirror ? gbase + e - kk + (K - 1 - kk) : gbase + e] : -1;
      s_nbr[e] = v;
      if (v >= 0) s_kact[kk] = 1;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int k = 0; k < K; ++k)
      if (s_kact[k]) s_kact[n++] = k;  // in-place compaction (n <= k)
    *s_nact = n;
  }
  __syncthreads();
  const int n_act = *s_nact;
  const int n_chunks = (KB > 1) ? 1 : (Cred + KC - 1) / KC;
  const int n_items = (KB > 1) ? (n_act + KB - 1) / KB : n_act * n_chunks;

  f32x4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int arow = wave * 16 + (lane & 15);
  const int kq = lane >> 4;

  float4 av[KB][2];   // VEC : 2 float4 of each A tile
  float as_[KB][8];   // !VEC: 8 scalars
  float bv[KB][NB];

  // cursors of the prefetch walk (one item ahead) and of the compute walk over the (offset, chunk) items: no integer division by
  // the runtime n_chunks inside the loop (conv_apply_split.hip)
  int pq = 0, pr = 0, cr = 0;
  auto prefetch = [&](int item) {
    const int pq_now = pq, pr_now = pr;
    if (KB == 1 && ++pr == n_chunks) { pr = 0; ++pq; }
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const int ai = (KB > 1) ? item * KB + kb : pq_now;
      const bool live = ai < n_act;
      const int k = live ? s_kact[ai] : 0;
      const int cc = (KB > 1) ? 0 : pr_now * KC;
      const int kc = min(KC, Cred - cc);
      const float* Wk = W + (size_t)k * Cred * Cres;
      if (VEC) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          int e = i * THREADS + tid, r = e / (KC / 4), c = (e % (KC / 4)) * 4;
          int j = live ? s_nbr[r * K + k] : -1;
          av[kb][i] = (j >= 0 && c < kc) ? *reinterpret_cast<const float4*>(feat + (size_t)j * Cred + cc + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          int e = i * THREADS + tid, r = e / KC, c = e % KC;
          int j = live ? s_nbr[r * K + k] : -1;
          as_[kb][i] = (j >= 0 && c < kc) ? feat[(size_t)j * Cred + cc + c] : 0.f;
        }
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        int e = i * THREADS + tid;
        if (!TRANS_W) {
          int r = e / (NT * 16), c = e % (NT * 16);
          bv[kb][i] = (live && r < kc && n0 + c < Cres) ? Wk[(size_t)(cc + r) * Cres + n0 + c] : 0.f;
        } else {  // Wk^T[r = co][c = ci] = W[k][ci][co]; consecutive threads read along co (contiguous)
          int c = e / KC, r = e % KC;
          bv[kb][i] = (live && r < kc && n0 + c < Cres) ? Wk[(size_t)(n0 + c) * Cred + cc + r] : 0.f;
        }
      }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      float* A = As + kb * TM * LDA;
      float* B = Bs + kb * KC * LDB;
      if (VEC) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          int e = i * THREADS + tid, r = e / (KC / 4), c = (e % (KC / 4)) * 4;
          float* d = A + r * LDA + c;
          d[0] = av[kb][i].x; d[1] = av[kb][i].y; d[2] = av[kb][i].z; d[3] = av[kb][i].w;
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          int e = i * THREADS + tid, r = e / KC, c = e % KC;
          A[r * LDA + c] = as_[kb][i];
        }
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        int e = i * THREADS + tid;
        if (!TRANS_W) {
          int r = e / (NT * 16), c = e % (NT * 16);
          B[r * LDB + c] = bv[kb][i];
        } else {
          int c = e / KC, r = e % KC;
          B[r * LDB + c] = bv[kb][i];
        }
      }
    }
  };

  if (n_items > 0) prefetch(0);
  for (int item = 0; item < n_items; ++item) {
    const int cc = (KB > 1) ? 0 : cr * KC;
    if (KB == 1 && ++cr == n_chunks) cr = 0;
    const int kc = min(KC, Cred - cc);
    __syncthreads();  // the previous item's fragment reads are done
    commit();
    __syncthreads();
    if (item + 1 < n_items) prefetch(item + 1);  // in flight during the MFMAs below
    const int steps = (kc + 3) >> 2;
    const int cnt = (KB > 1) ? min(KB, n_act - item * KB) : 1;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      if (kb >= cnt) break;  // block-uniform; padded offsets hold zeros anyway
      const float* A = As + kb * TM * LDA;
      const float* B = Bs + kb * KC * LDB;
      for (int q = 0; q < steps; ++q) {
        float a = A[arow * LDA + q * 4 + kq];
        const float* bp = B + (q * 4 + kq) * LDB + (lane & 15);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[nt * 16], acc[nt], 0, 0, 0);
      }
    }
  }

  float vals[NT][4];
  bool valid[4];
  int rows[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) rows[r] = row0 + wave * 16 + kq * 4 + r < n_rows ? row0 + wave * 16 + kq * 4 + r : -1;
  const bool ev = !TRANS_W && bn.ev_mean != nullptr;   // (bn_fuse.h, second mode; forward instances only)
  apply_tile_epilogue<NT, true>(acc, rows, n0, bias, Cres, out, bn, ev, vals, valid);
  if (bn.slots) {
    bn_fuse_wave<NT>(bn, vals, valid, n0, (int)((blockIdx.x * (THREADS / 64) + wave) & (bn.nslots - 1)));
    bn_fuse_finish(bn, (int*)smem, (double*)(smem + 16));
  }
}

// ------------------------------------------------------------------------------------------------------------
// Weight-stationary variant for narrow layers (Cred, Cres <= 32: K*Cred*Cres*4 <= 110 KB).  The profile of
// conv_apply on these layers is dominated by L2->LDS re-reads of the K weight panels by every 64-row workgroup and
// by the serial chain of K barrier-separated gather->MFMA phases per tile.  Here one persistent 16-wave workgroup
// per CU keeps ALL K panels resident in LDS (160 KB per CU on gfx950); every wave walks its own 16-row tiles with
// no workgroup barrier after the weight load; the A fragments are gathered STRAIGHT INTO REGISTERS in MFMA layout
// (lane (row, kq) loads channels q*4+kq), WS_KB offsets at a time, one group ahead of the MFMAs.
// Same summation order as conv_apply (offset ascending, channel ascending) -> same bits.
// ------------------------------------------------------------------------------------------------------------
constexpr int WS_WAVES = 16;
constexpr int WS_KB = 8;    // offsets per group of gathers (round 6: 4 -> 8 with WS_Q below: a 27-offset tile is 4 dependent round trips, not 7;
                            // 5 -> 32 at 210 K rows 80 -> 72 us, 4 -> 16 18.5 -> 16.4, same bits; 14 offsets per group measured 77)
constexpr int WS_Q = 2;     // k-steps of a row: the kernel is launched for reductions of <= 8 channels only (it sized its fragment registers for 32)

__host__ __device__ inline size_t ws_lds_bytes(int K, int Cred, int nt) {
  int crp = (Cred + 3) & ~3;
  return (size_t)K * crp * (nt * 16) * sizeof(float) + (size_t)WS_WAVES * 16 * K * sizeof(int32_t);
}

// EV: the eval-mode BatchNorm epilogue (bn_fuse.h, second mode) is a TEMPLATE parameter of this family: as a run-time branch it cost the
// two-tile forward instance 7 registers and its fifth wave per SIMD
template <int NT, bool TRANS_W, bool EV = false>
__global__ __launch_bounds__(WS_WAVES * 64) void conv_apply_ws(const float* __restrict__ feat, const float* __restrict__ W,
                                                              const float* __restrict__ bias, const int32_t* __restrict__ nbr,
                                                              int n_rows, int K, int Cred, int Cres, float* __restrict__ out, int mirror,
                                                              const BnFuse bn) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int LDW = NT * 16;
  constexpr int QMAX = WS_Q;
  const int crp = (Cred + 3) & ~3;
  float* Ws = (float*)smem;                                     // [K][crp][LDW], column XOR-swizzled by (row & 1) << 4 when NT == 2
  int32_t* nb_all = (int32_t*)(Ws + (size_t)K * crp * LDW);     // [WS_WAVES][16][K]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4, lrow = lane & 15;
  int32_t* nb = nb_all + wave * 16 * K;

  // ---- resident weights: Ws[k][r][c] = Wk[r][c]  (Wk = W[k] or W[k]^T), zero padded; loads batched 8 deep
  {
    const int total = K * crp * LDW;
    for (int base = 0; base < total; base += WS_WAVES * 64 * 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        int e = base + u * WS_WAVES * 64 + tid;
        int c = e % LDW, r = (e / LDW) % crp, k = e / (LDW * crp);
        v[u] = 0.f;
        if (e < total && r < Cred && c < Cres) v[u] = TRANS_W ? W[((size_t)k * Cres + c) * Cred + r] : W[((size_t)k * Cred + r) * Cres + c];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        int e = base + u * WS_WAVES * 64 + tid;
        if (e < total) {
          int c = e % LDW, r = (e / LDW) % crp, k = e / (LDW * crp);
          int cs = (NT == 2) ? (c ^ ((r & 1) << 4)) : c;
          Ws[((size_t)k * crp + r) * LDW + cs] = v[u];
        }
      }
    }
  }
  __syncthreads();

  const int n_tiles = (n_rows + 15) >> 4;
  const int steps = crp >> 2;
  for (int tile = blockIdx.x * WS_WAVES + wave; tile < n_tiles; tile += gridDim.x * WS_WAVES) {
    const int row0 = tile << 4;
    // neighbour rows of the tile (16 x K ints, contiguous) and the set of offsets that occur in it
    unsigned long long kmask = 0;
    {
      const long long gbase = (long long)row0 * K, gend = (long long)n_rows * K;
      for (int e = lane; e < 16 * K; e += 64) {
        const int kk = e % K;
        int v = (gbase + e < gend) ? nbr[mirror ? gbase + e - kk + (K - 1 - kk) : gbase + e] : -1;
        nb[e] = v;
        if (v >= 0) kmask |= 1ull << kk;
      }
      kmask = btc_wave_all_or(kmask);
    }
    __builtin_amdgcn_wave_barrier();
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    float va[WS_KB][QMAX], vb[WS_KB][QMAX];  // current / next group of A fragments
    int ka[WS_KB], kb_[WS_KB];
    unsigned long long rem = kmask;
    // take the next WS_KB active offsets off the mask and issue their gathers into `v`
#define WS_FETCH(v, kk)                                                                             \
  _Pragma("unroll") for (int g = 0; g < WS_KB; ++g) {                                               \
    kk[g] = rem ? (__ffsll((long long)rem) - 1) : -1;                                               \
    rem &= rem - 1;                                                                                 \
    const int j = (kk[g] >= 0) ? nb[lrow * K + kk[g]] : -1;                                         \
    const float* src = feat + (size_t)(j >= 0 ? j : 0) * Cred + kq;                                 \
    _Pragma("unroll") for (int q = 0; q < QMAX; ++q)                                                \
        v[g][q] = (j >= 0 && q * 4 + kq < Cred && q < steps) ? src[q * 4] : 0.f;                    \
  }
#define WS_MATH(v, kk)                                                                              \
  _Pragma("unroll") for (int g = 0; g < WS_KB; ++g) {                                               \
    if (kk[g] < 0) break;                                                                           \
    const float* Wk = Ws + (size_t)kk[g] * crp * LDW;                                               \
    _Pragma("unroll") for (int q = 0; q < QMAX; ++q) {                                              \
      if (q >= steps) break;                                                                        \
      const int r = q * 4 + kq;                                                                     \
      _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) {                                           \
        int c = nt * 16 + lrow;                                                                     \
        if (NT == 2) c ^= (r & 1) << 4;                                                             \
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[g][q], Wk[r * LDW + c], acc[nt], 0, 0, 0); \
      }                                                                                             \
    }                                                                                               \
  }
    WS_FETCH(va, ka)
    while (ka[0] >= 0) {
      WS_FETCH(vb, kb_)   // next group in flight during this group's MFMAs
      WS_MATH(va, ka)
      if (kb_[0] < 0) break;
      WS_FETCH(va, ka)
      WS_MATH(vb, kb_)
    }
#undef WS_FETCH
#undef WS_MATH
    // (this family keeps its own epilogue: through apply_tile_epilogue the two-tile instances allocate 3 registers fewer, and the bar for
    // sharing it is an unchanged allocation)
    float vals[NT][4];
    bool valid[4];
    constexpr bool ev = EV;
#pragma unroll
    for (int r = 0; r < 4; ++r) valid[r] = row0 + kq * 4 + r < n_rows;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int col = nt * 16 + lrow;
      const float bv0 = (bias && col < Cres) ? bias[col] : 0.f;
      BnEvalCol ec = {0.f, 0.f, 1.f, 0.f};
      if (ev) ec = bn_eval_col(bn, col);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + kq * 4 + r;
        vals[nt][r] = bias ? (acc[nt][r] + bv0) : acc[nt][r];
        if (ev) vals[nt][r] = bn_affine(vals[nt][r], ec.m, ec.rs, ec.g, ec.b, bn.ev_relu);
        if (col < Cres && row < n_rows) out[(size_t)row * Cres + col] = vals[nt][r];
      }
    }
    if (bn.slots) bn_fuse_wave<NT>(bn, vals, valid, 0, (int)(tile & (bn.nslots - 1)));
    __builtin_amdgcn_wave_barrier();
  }
  if (bn.slots) bn_fuse_finish(bn, (int*)smem, (double*)(smem + 16));
}


__global__ __launch_bounds__(256) void maxpool_fwd_k(const float* __restrict__ feat, const int32_t* __restrict__ nbr,
                                                     int n_out, int K, int C, float* __restrict__ out) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)n_out * C) return;
  int i = (int)(t / C), c = (int)(t % C);
  float m = 0.f;
  for (int k = 0; k < K; ++k) {
    int j = nbr[(size_t)i * K + k];
    if (j >= 0) m = fmaxf(m, feat[(size_t)j * C + c]);
  }
  out[t] = m;
}

__global__ __launch_bounds__(256) void maxpool_bwd_k(const float* __restrict__ feat, const float* __restrict__ out,
                                                     const float* __restrict__ dout, const int32_t* __restrict__ nbr_in,
                                                     int n_in, int K, int C, float* __restrict__ din) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)n_in * C) return;
  int j = (int)(t / C), c = (int)(t % C);
  float v = feat[t], g = 0.f;
  for (int k = 0; k < K; ++k) {
    int i = nbr_in[(size_t)j * K + k];
    if (i >= 0 && out[(size_t)i * C + c] == v) g += dout[(size_t)i * C + c];
  }
  din[t] = g;
}

// dense[b][c][z][y][x] = feat[row][c]; consecutive threads take consecutive rows of one channel so the
// dense writes coalesce for (b,z,y,x)-sorted tensors (feature reads are strided but L2 resident)
__global__ __launch_bounds__(256) void dense_fwd_k(const float* __restrict__ feat, const int4* __restrict__ idx, int n, int C,
                                                   int D, int H, int Wd, float* __restrict__ dense) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)n * C) return;
  int c = (int)(t / n), i = (int)(t % n);  // consecutive threads -> consecutive rows of one channel
  int4 q = idx[i];
  size_t vol = (size_t)D * H * Wd;
  dense[((size_t)q.x * C + c) * vol + ((size_t)q.y * H + q.z) * Wd + q.w] = feat[(size_t)i * C + c];
}

__global__ __launch_bounds__(256) void dense_bwd_k(const float* __restrict__ ddense, const int4* __restrict__ idx, int n, int C,
                                                   int D, int H, int Wd, float* __restrict__ dfeat) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)n * C) return;
  int c = (int)(t / n), i = (int)(t % n);
  int4 q = idx[i];
  size_t vol = (size_t)D * H * Wd;
  dfeat[(size_t)i * C + c] = ddense[((size_t)q.x * C + c) * vol + ((size_t)q.y * H + q.z) * Wd + q.w];
}

// (the map tile is TM x K int32: past ~148 offsets a launch wants more than 64 KB of LDS, K = BTC_CONV_K_MAX: 157 KB.  Through
// apply_launch every instance raises its limit on its first launch per device, not only the launches that need it.)
template <int NT, bool TRANS_W, int THREADS>
int launch_apply_t(dim3 grid, size_t lds, hipStream_t stream, bool vec, const float* feat, const float* W, const float* bias,
                   const int32_t* nbr, int n_rows, int K, int Cred, int Cres, float* out, int mirror, const BnFuse& bn) {
  if (vec) return apply_launch<conv_apply<NT, TRANS_W, true, 1, THREADS>>("conv_apply", grid, THREADS, lds, stream, feat, W, bias, nbr, n_rows, K, Cred, Cres, out, mirror, bn);
  return apply_launch<conv_apply<NT, TRANS_W, false, 1, THREADS>>("conv_apply", grid, THREADS, lds, stream, feat, W, bias, nbr, n_rows, K, Cred, Cres, out, mirror, bn);
}

template <bool TRANS_W, bool EV>
int launch_ws(int nt, int wgs, size_t lds, hipStream_t stream, const float* feat, const float* W, const float* bias, const int32_t* nbr, int n_rows,
              int K, int Cred, int Cres, float* out, int mirror, const BnFuse& bn) {
  if (nt == 1) return apply_launch<conv_apply_ws<1, TRANS_W, EV>>("conv_apply_ws", wgs, WS_WAVES * 64, lds, stream, feat, W, bias, nbr, n_rows, K, Cred, Cres, out, mirror, bn);
  return apply_launch<conv_apply_ws<2, TRANS_W, EV>>("conv_apply_ws", wgs, WS_WAVES * 64, lds, stream, feat, W, bias, nbr, n_rows, K, Cred, Cres, out, mirror, bn);
}

template <bool TRANS_W>
int launch_apply(const float* feat, const float* W, const float* bias, const int32_t* nbr, int n_rows, int K, int Cred,
                 int Cres, float* out, hipStream_t stream, bool bf = false, const int32_t* order = nullptr, int mirror = 0,
                 const BnFuse* bn_ = nullptr) {
  const BnFuse bn = bn_ ? *bn_ : btc_bn_fuse_none();   // batch statistics of the result in the epilogue (every kernel family below has it)
  // order: optional row-order hint (row_order.hip); only the LDS-DMA kernel tiles by it, the others ignore it (same results)
  // bf: feat / out are bfloat16 (passed through the float* parameters); only the LDS-DMA kernel has that variant
  if (n_rows <= 0) return BTC_OK;
  BTC_CHECK_ARG(!bf || btc_apply_glds_supported(K, Cred, Cres),
                "bf16 activations need channel counts that are multiples of 16 (K=%d, %d -> %d): convert to fp32", K, Cred, Cres);
  int nt = Cres <= 16 ? 1 : (Cres <= 32 ? 2 : (Cres <= 64 ? 4 : 8));
  const int t_kernel = btc_tune_get(BTC_TUNE_APPLY_KERNEL), t_nt = btc_tune_get(BTC_TUNE_APPLY_NT);
  // LDS-DMA pipelined kernel (conv_apply_glds.hip) for every layer whose channel counts are multiples of 16, except the
  // 200 K-row occupancy-branch layers where the register-staged kernel below measures 5-10 % faster.  Wave shapes from
  // tools/conv_bench.py on MI355X (us per launch, register-staged -> LDS-DMA): 14 K rows 64->64: 80 -> 53, 128->128: 225 -> 158,
  // 256->128: 456 -> 309; 3 K rows 64->64: 65 -> 40; 30 K rows 64->64: 119 -> 99.
  // (the 100 K-row exception is about the 32-channel occupancy-branch layers; wide layers -- the ROI head's 128-channel
  // micro-scene pyramid at 130 K rows -- stay on the LDS-DMA kernel at any row count)
  if (bf || (t_kernel != 1 && btc_apply_glds_supported(K, Cred, Cres) && (t_kernel == 2 || n_rows < 100000 || (Cred >= 64 && Cres >= 64)))) {
    int shape, kc = (Cred % 64 == 0) ? 64 : ((Cred % 32 == 0) ? 32 : 16);
    // Wave shapes from a row-count sweep on MI355X (fp32, K = 27, a 7.7-pairs-per-row SubM map cut to n rows; us per launch).
    // The time of a shape is a staircase in n with a step at every multiple of 256 CUs x TM rows, so the best TM depends on
    // where n falls: 256 -> 128 at 4 K rows 296 (424) vs 148 (222), at 10 K rows 301 vs 196 (242), at 16 K rows 306 (424, one
    // full round) vs 353, at 18 K rows 467 (424: a second, nearly empty round) vs 383 (242); 64 -> 64 at 10 K rows 52 (422)
    // vs 37 (141), from 18 K rows on 80-133 (422) vs 67-122 (241); 32 -> 64 from 18 K rows on 50-76 (422) vs 41-71 (222).
    if (bf) {
      if (Cres % 128 == 0) shape = 424;                       // 64 rows x 128 columns, 8 waves
      else if (Cres % 64 == 0) shape = n_rows < 8192 ? 141 : 422;  // few rows: 16-row workgroups, 4 waves across the columns
      else if (Cres % 32 == 0) shape = 221;
      else shape = 411;
    } else if (Cres % 128 == 0) {
      shape = n_rows < 7000 ? 222 : (n_rows < 13000 ? 242 : (n_rows <= 16384 ? 424 : (n_rows < 19500 ? 242 : 424)));
    } else if (Cres % 64 == 0) {
      if (kc == 64) shape = n_rows < 11000 ? 141 : 241;
      else shape = n_rows < 13000 ? 141 : 222;
    } else if (Cres % 32 == 0) {
      shape = 221;
    } else {
      shape = 411;
    }
    if (t_nt > 8 && !bf) {  // tuning run: BTC_TUNE_APPLY_NT carries the wave shape WR*100 + WC*10 + NTW
      int wc = (t_nt / 10) % 10, ntw = t_nt % 10;
      while (ntw > 1 && Cres % (16 * wc * ntw)) ntw >>= 1;
      while (wc > 1 && Cres % (16 * wc * ntw)) wc >>= 1;
      const int cand = (t_nt / 100) * 100 + wc * 10 + ntw;
      if (btc_apply_glds_has_shape(cand)) shape = cand;
    }
    const int t_kc = btc_tune_get(BTC_TUNE_APPLY_KC);
    if (t_kc && Cred % t_kc == 0) kc = t_kc;
    while (kc > 16 && btc_apply_glds_lds_bytes(shape, kc, K, bf) > 160 * 1024) kc >>= 1;  // 3-stage ring + map tile
    return btc_launch_apply_glds(TRANS_W, shape, kc, apply_flags(mirror), bf, feat, W, bias, nbr, order, n_rows, K, Cred, Cres, out, stream, &bn);
  }
  // weight-stationary persistent kernel (one 16-wave workgroup per CU).  Measured on MI355X: its dword-granular register
  // gather wins 2.5x for Cred <= 8 (the dgrad of the 2/3-channel occupancy heads, the 4/6-channel input layers) and loses
  // 2x at Cred = 32 (load-issue bound), so wider layers stay on the LDS-staged float4 kernel below.
  if (t_kernel != 1 && Cred <= 4 * WS_Q && Cres <= 32 && K <= 64 && n_rows >= 2048 && ws_lds_bytes(K, Cred, nt) <= 160 * 1024) {
    const int n_tiles16 = btc_cdiv(n_rows, 16);
    int wgs = btc_cdiv(n_tiles16, WS_WAVES);
    if (wgs > 256) wgs = 256;
    size_t lds = ws_lds_bytes(K, Cred, nt);
    // the statistics epilogue's last arriver shares the slot sums through 16 + 16 bytes x threads of (by then dead) LDS
    // (bn_fuse_finish's s_part): few offsets x few channels -- K = 8 with 4 input channels is 10 KB -- would leave it short
    if (bn.slots && lds < 16 + (size_t)16 * WS_WAVES * 64) lds = 16 + (size_t)16 * WS_WAVES * 64;
    if constexpr (!TRANS_W) {   // eval-mode BatchNorm (+ ReLU) in the epilogue: the instances compiled for it
      if (bn.ev_mean) return launch_ws<false, true>(nt, wgs, lds, stream, feat, W, bias, nbr, n_rows, K, Cred, Cres, out, mirror, bn);
    }
    return launch_ws<TRANS_W, false>(nt, wgs, lds, stream, feat, W, bias, nbr, n_rows, K, Cred, Cres, out, mirror, bn);
  }
  // 64 rows per workgroup (256 threads).  Measured: 32- and 16-row workgroups of this register-staged kernel are ~2x SLOWER on
  // every BtcDet layer -- each workgroup re-reads all K weight panels, so L2->LDS weight traffic scales with the number of
  // workgroups (the template keeps the THREADS parameter; only the 256-thread instances are built).
  const int tm = 64;
  const int n_tiles = btc_cdiv(n_rows, tm);
  // still too few workgroups (deep, narrow levels): also split the result channels
  while (nt > 2 && (long long)n_tiles * btc_cdiv(Cres, nt * 16) < 512) nt >>= 1;
  if (t_nt && t_nt <= 8) nt = t_nt;
  dim3 grid(n_tiles, btc_cdiv(Cres, nt * 16));
  size_t lds = (size_t)(tm * LDA + KC * ldb_of(nt)) * sizeof(float) + (size_t)(tm * K + K + 1) * sizeof(int32_t);
  const bool vec = (Cred & 3) == 0;
#define BTC_APPLY(NT_) launch_apply_t<NT_, TRANS_W, 256>(grid, lds, stream, vec, feat, W, bias, nbr, n_rows, K, Cred, Cres, out, mirror, bn)
  switch (nt) {
    case 1: return BTC_APPLY(1);
    case 2: return BTC_APPLY(2);
    case 4: return BTC_APPLY(4);
    default: return BTC_APPLY(8);
  }
#undef BTC_APPLY
}

// split operands: the kernel gathers through 32-bit byte offsets -- the HOST refuses a source it cannot reach (or whose size it was not
// told), nothing traps on the device
int split_source_ok(const char* who, long long src_rows, int Cred) {
  BTC_CHECK_ARG(src_rows >= 0, "%s: BTC_OPERANDS_F32_SPLIT needs the row count of src (btc_conv_apply_src / btc_conv_bn_relu_fwd_src)", who);
  BTC_CHECK_ARG(src_rows * Cred * 4 < 0xFFFFFF00LL, "%s: a source of %lld rows x %d channels is past the 32-bit gather offsets of the split-operand "
                "kernel (4 GB): use BTC_OPERANDS_F32", who, src_rows, Cred);
  return BTC_OK;
}

}  // namespace

// The ONE way from (pass, operands) to a kernel family: every extern "C" apply entry point, here and in bn.hip, is a wrapper over it and
// holds only the checks that are its own.  who: the entry point, for the error texts.  src_rows: rows of src (read for split operands
// only; < 0 = not told).  bn: the epilogue of a forward pass -- batch statistics or the eval-mode BatchNorm (bn_fuse.h) -- or NULL.
int btc_apply(const char* who, int pass, int operands, const void* src, long long src_rows, const void* W, const float* bias, const int32_t* nbr,
              const int32_t* order, int n_rows, int K, int Cin, int Cout, void* dst, hipStream_t stream, const BnFuse* bn) {
  BTC_CHECK_ARG((pass == BTC_PASS_FWD || pass == BTC_PASS_DGRAD || pass == BTC_PASS_DGRAD_MIRROR) && operands >= BTC_OPERANDS_F32 &&
                    operands <= BTC_OPERANDS_F32_SPLIT, "%s: pass=%d operands=%d", who, pass, operands);
  // BTC_PASS_DGRAD_MIRROR: dgrad of a submanifold layer through its FORWARD map -- nbr_in[j][k] == nbr_out[j][K-1-k] there, so the
  // kernels read column K-1-k for offset k and the backward map never exists (same bits as the explicit map: tests)
  const int mirror = pass == BTC_PASS_DGRAD_MIRROR;
  const bool fwd = pass == BTC_PASS_FWD;
  BTC_CHECK_ARG(K <= BTC_CONV_K_MAX, "%s: K=%d offsets, more than BTC_CONV_K_MAX = %d", who, K, BTC_CONV_K_MAX);
  // (the entry points that take pass and operands report sizes HERE, behind K; the fixed-operand wrappers below repeat the check in front)
  BTC_CHECK_ARG(K >= 1 && Cin >= 1 && Cout >= 1 && n_rows >= 0, "%s: bad sizes", who);
  BTC_CHECK_ARG(fwd || bias == nullptr, "%s: dgrad takes no bias", who);
  BTC_CHECK_ARG(!bn || Cout <= BN_FUSE_CMAX, "%s: more than %d channels", who, BN_FUSE_CMAX);
  const int Cred = fwd ? Cin : Cout, Cres = fwd ? Cout : Cin;
  if (operands == BTC_OPERANDS_BF16) {   // W = the bf16 copy of btc_weights_to_bf16 for this pass
    const bool ok = btc_conv_bf16w_supported(K, Cred, Cres);
    // (error texts are part of the entry points' contract: the BatchNorm ones word this refusal in Cin / Cout, without the values)
    if (bn) BTC_CHECK_ARG(ok, "%s: bf16 operands need K <= 64, Cin %% 32 == 0, Cout %% 16 == 0", who);
    else BTC_CHECK_ARG(ok, "%s: bf16 operands need K <= 64, Cred %% 32 == 0, Cres %% 16 == 0 (K=%d, %d -> %d)", who, K, Cin, Cout);
    return btc_apply_bf16w(src, W, bias, nbr, order, n_rows, K, Cred, Cres, dst, stream, mirror, bn);
  }
  if (operands == BTC_OPERANDS_F32_SPLIT) {
    if (n_rows > 0) {
      const int rc = split_source_ok(who, src_rows, Cred);
      if (rc) return rc;
    }
    return btc_apply_split((const float*)src, W, bias, nbr, order, n_rows, K, Cred, Cres, (float*)dst, stream, mirror, bn);
  }
  const bool bf = operands == BTC_OPERANDS_BF16_ACT;
  if (fwd) return launch_apply<false>((const float*)src, (const float*)W, bias, nbr, n_rows, K, Cred, Cres, (float*)dst, stream, bf, order, 0, bn);
  return launch_apply<true>((const float*)src, (const float*)W, nullptr, nbr, n_rows, K, Cred, Cres, (float*)dst, stream, bf, order, mirror, bn);
}

// The fixed-operand entry points.  Theirs alone: "bad sizes" is reported before a K past BTC_CONV_K_MAX, and for the two bf16 pairs a call
// without rows is done once its own check has passed, whatever K and the channel counts are.
#define BTC_SIZES_OK(who, n) BTC_CHECK_ARG(K >= 1 && Cin >= 1 && Cout >= 1 && (n) >= 0, who ": bad sizes")

extern "C" int btc_conv_fwd(const float* feat, const float* W, const float* bias, const int32_t* nbr_out, int n_out, int K,
                            int Cin, int Cout, float* out, void* stream) {
  BTC_SIZES_OK("btc_conv_fwd", n_out);
  return btc_apply("btc_conv_fwd", BTC_PASS_FWD, BTC_OPERANDS_F32, feat, -1LL, W, bias, nbr_out, nullptr, n_out, K, Cin, Cout, out, (hipStream_t)stream, nullptr);
}

extern "C" int btc_conv_dgrad(const float* dout, const float* W, const int32_t* nbr_in, int n_in, int K, int Cin, int Cout,
                              float* din, void* stream) {
  BTC_SIZES_OK("btc_conv_dgrad", n_in);
  return btc_apply("btc_conv_dgrad", BTC_PASS_DGRAD, BTC_OPERANDS_F32, dout, -1LL, W, nullptr, nbr_in, nullptr, n_in, K, Cin, Cout, din, (hipStream_t)stream, nullptr);
}

extern "C" int btc_conv_fwd_bf16(const void* feat, const float* W, const float* bias, const int32_t* nbr_out, int n_out, int K,
                                 int Cin, int Cout, void* out, void* stream) {
  BTC_SIZES_OK("btc_conv_fwd_bf16", n_out);
  if (n_out == 0) return BTC_OK;
  return btc_apply("btc_conv_fwd_bf16", BTC_PASS_FWD, BTC_OPERANDS_BF16_ACT, feat, -1LL, W, bias, nbr_out, nullptr, n_out, K, Cin, Cout, out, (hipStream_t)stream, nullptr);
}

extern "C" int btc_conv_dgrad_bf16(const void* dout, const float* W, const int32_t* nbr_in, int n_in, int K, int Cin, int Cout,
                                   void* din, void* stream) {
  BTC_SIZES_OK("btc_conv_dgrad_bf16", n_in);
  if (n_in == 0) return BTC_OK;
  return btc_apply("btc_conv_dgrad_bf16", BTC_PASS_DGRAD, BTC_OPERANDS_BF16_ACT, dout, -1LL, W, nullptr, nbr_in, nullptr, n_in, K, Cin, Cout, din, (hipStream_t)stream, nullptr);
}
#undef BTC_SIZES_OK

// bf16 operands (W = a copy of btc_weights_to_bf16); their one combined refusal keeps its text
extern "C" int btc_conv_fwd_bf16w(const void* feat, const void* wt_bf16, const float* bias, const int32_t* nbr_out, int n_out, int K, int Cin,
                                  int Cout, void* out, void* stream) {
  BTC_CHECK_ARG(n_out >= 0 && btc_conv_bf16w_supported(K, Cin, Cout), "btc_conv_fwd_bf16w: needs K <= 64, Cin %% 32 == 0, Cout %% 16 == 0 (K=%d, %d -> %d)",
                K, Cin, Cout);
  if (n_out == 0) return BTC_OK;
  return btc_apply("btc_conv_fwd_bf16w", BTC_PASS_FWD, BTC_OPERANDS_BF16, feat, -1LL, wt_bf16, bias, nbr_out, nullptr, n_out, K, Cin, Cout, out, (hipStream_t)stream, nullptr);
}

extern "C" int btc_conv_dgrad_bf16w(const void* dout, const void* w_bf16, const int32_t* nbr_in, int n_in, int K, int Cin, int Cout, void* din,
                                    void* stream) {
  BTC_CHECK_ARG(n_in >= 0 && btc_conv_bf16w_supported(K, Cout, Cin), "btc_conv_dgrad_bf16w: needs K <= 64, Cout %% 32 == 0, Cin %% 16 == 0 (K=%d, %d -> %d)",
                K, Cin, Cout);
  if (n_in == 0) return BTC_OK;
  return btc_apply("btc_conv_dgrad_bf16w", BTC_PASS_DGRAD, BTC_OPERANDS_BF16, dout, -1LL, w_bf16, nullptr, nbr_in, nullptr, n_in, K, Cin, Cout, din, (hipStream_t)stream, nullptr);
}

extern "C" int btc_conv_apply_ordered(int pass, int operands, const void* src, const void* W, const float* bias, const int32_t* nbr,
                                      const int32_t* order, int n_rows, int K, int Cin, int Cout, void* dst, void* stream) {
  // (a submanifold layer's source has as many rows as its result; any other source's size is the caller's to state)
  return btc_apply("btc_conv_apply_ordered", pass, operands, src, pass == BTC_PASS_DGRAD_MIRROR ? (long long)n_rows : -1LL, W, bias, nbr, order, n_rows,
                   K, Cin, Cout, dst, (hipStream_t)stream, nullptr);
}

extern "C" int btc_conv_apply_src(int pass, int operands, const void* src, long long src_rows, const void* W, const float* bias, const int32_t* nbr,
                                  const int32_t* order, int n_rows, int K, int Cin, int Cout, void* dst, void* stream) {
  return btc_apply("btc_conv_apply_src", pass, operands, src, src_rows, W, bias, nbr, order, n_rows, K, Cin, Cout, dst, (hipStream_t)stream, nullptr);
}

extern "C" int btc_maxpool_fwd(const float* feat, const int32_t* nbr_out, int n_out, int K, int C, float* out, void* stream) {
  if (n_out <= 0) return BTC_OK;
  maxpool_fwd_k<<<btc_cdiv((long long)n_out * C, 256), 256, 0, (hipStream_t)stream>>>(feat, nbr_out, n_out, K, C, out);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}

extern "C" int btc_maxpool_bwd(const float* feat, const float* out, const float* dout, const int32_t* nbr_in, int n_in, int K,
                               int C, float* din, void* stream) {
  if (n_in <= 0) return BTC_OK;
  maxpool_bwd_k<<<btc_cdiv((long long)n_in * C, 256), 256, 0, (hipStream_t)stream>>>(feat, out, dout, nbr_in, n_in, K, C, din);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}

extern "C" int btc_dense_fwd(const float* feat, const int32_t* indices, int n, int C, const int32_t* h_shape, float* dense,
                             void* stream) {
  if (n <= 0) return BTC_OK;
  dense_fwd_k<<<btc_cdiv((long long)n * C, 256), 256, 0, (hipStream_t)stream>>>(feat, (const int4*)indices, n, C, h_shape[0],
                                                                               h_shape[1], h_shape[2], dense);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}

extern "C" int btc_dense_bwd(const float* ddense, const int32_t* indices, int n, int C, const int32_t* h_shape, float* dfeat,
                             void* stream) {
  if (n <= 0) return BTC_OK;
  dense_bwd_k<<<btc_cdiv((long long)n * C, 256), 256, 0, (hipStream_t)stream>>>(ddense, (const int4*)indices, n, C, h_shape[0],
                                                                               h_shape[1], h_shape[2], dfeat);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}
