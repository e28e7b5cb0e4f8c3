// Fused BatchNorm1d (+ReLU) over sparse-tensor features (N rows x C channels, fp32) for gfx950.
//
// The reference applies nn.BatchNorm1d(eps=1e-3, momentum=0.01) and nn.ReLU to `.features` after every sparse conv
// (spconv.SparseSequential, /root/reference/btcdet/models/backbones_3d/spconv_backbone.py:33-43,96,634): on ROCm that is
// ~10 small launches per layer (statistics, running-stat updates, transform, clamp, and their backward twins), all
// latency bound at BtcDet's sizes.  Here: 2 launches forward, 2 backward.
//   bn_reduce               : the two-level, fixed-order channel reduction, stated once.  Every workgroup sums its rows per channel
//                             (fp64 accumulation) and publishes the partial sums; the LAST workgroup to arrive (btc_last_arriver,
//                             btc_common.h) adds every workgroup's partials in index order (deterministic), hands each channel's
//                             totals to the caller and leaves the arrival counter zero for the next launch
//   bn_stats / bn_bwd_stats / col_sum : bn_reduce with the kernel's own walk over a thread's rows (its unrolled and tail loops, its
//                             arithmetic) and its own finalisation: mean / rstd, the running statistics and num_batches_tracked;
//                             dgamma / dbeta; a plain sum.  The scalar and the 4-channels-per-thread path are one body (W = 1 / 4)
//   bn_apply / bn_bwd_apply : elementwise, float4
#include "btc_common.h"
#include "bn_fuse.h"
#include "../../include/btcdet_hip_infer.h"

#include <type_traits>

namespace {

constexpr int BN_T = 256;

struct BnShape {
  int N, C, cpow, rpi;  // cpow = pow2 >= min(C,256); rpi = rows per iteration of a workgroup
};

// a workgroup's partial sums are published with device-scope (sc1, write-through) stores: they are at the coherence point once the
// storing wave's vector-memory queue has drained -- no agent-scope release fence, i.e. no write-back of the XCD L2's dirty lines (all
// the activations the previous kernels wrote) once per workgroup (MI355X_MICROARCH.md, handoff-flag: `sc1` payload -> vmcnt(0) -> flag)
__device__ __forceinline__ void st_partial(double* p, double v) { btc_st_agent(p, v); }

// W adjacent channels of one row (W = 4: one float4, bf16: 8 bytes -- a quarter of the load instructions of W = 1 for the same bytes)
template <bool BF, int W>
__device__ __forceinline__ void bn_ld(const float* base, long long i, float (&e)[W]) {
  if constexpr (W == 4) {
    const float4 v = btc_ld4<BF>(base, i);
    e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
  } else {
    e[0] = btc_ld1<BF>(base, i);
  }
}

// one pass of a workgroup over the channel groups of shape S (W channels each, Q sums per channel): thread (cw, rr) fills its sums,
// the row lanes 0 .. rpi-1 of a channel group are combined over LDS in that order, and row lane 0 emits the group's sums
template <int W, int Q, int P, class Fill, class Emit>
__device__ __forceinline__ void bn_pass(const BnShape& S, double (&s)[Q][P], Fill fill, Emit emit) {
  const int tid = threadIdx.x;
  for (int c0 = 0; c0 < S.C; c0 += S.cpow) {
    const int cw = c0 + (tid % S.cpow), rr = tid / S.cpow;
    double acc[Q][W];
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
      for (int j = 0; j < W; ++j) acc[q][j] = 0.0;
    if (cw < S.C) fill(cw, rr, acc);
#pragma unroll
    for (int j = 0; j < W; ++j)
#pragma unroll
      for (int q = 0; q < Q; ++q) s[q][tid * W + j] = acc[q][j];
    __syncthreads();
    if (rr == 0 && cw < S.C) {
      for (int l = 1; l < S.rpi; ++l)
#pragma unroll
        for (int j = 0; j < W; ++j)   // (channel outermost: in the other order the compiler keeps fewer LDS reads in flight)
#pragma unroll
          for (int q = 0; q < Q; ++q) acc[q][j] += s[q][(tid + l * S.cpow) * W + j];
      emit(cw, acc);
    }
    __syncthreads();
  }
}

// The reduction of Q sums per channel over all N rows.  S = bn_shape(N, C), SW = bn_shape(N, C / W): a thread owns W adjacent channels.
//   rows(cw, r0, stride, acc) : adds rows r0, r0 + stride, ... (< N) of channels cw * W .. cw * W + W - 1 into acc[Q][W]
//   done(c, t)                : the last workgroup's thread of channel c receives the totals t[Q]
// partial[workgroup][q][c]; the last arriver's thread-row rr takes workgroups rr, rr + rpi, ... with D partials per sum in flight, added
// as a tree (the walk is a chain of L2 round trips: at 4 in flight and 512 workgroups it took longer than the pass over the data -- 22
// of the 45 us of a 210 K x 32 backward-statistics launch), then one at a time; the thread-rows are combined 0 .. rpi-1.
// -> true in the last workgroup (all of it), after done() has run for every channel: once-per-launch work belongs behind it
template <int W, int Q, int D, class Rows, class Done>
__device__ __forceinline__ bool bn_reduce(const BnShape& S, const BnShape& SW, double* __restrict__ partial, int32_t* __restrict__ counter,
                                          Rows rows, Done done) {
  __shared__ double s[Q][BN_T * W];
  const int G = (int)gridDim.x;
  auto at = [&](int g, int q, int c) { return &partial[((size_t)g * Q + q) * S.C + c]; };
  bn_pass<W>(SW, s,
             [&](int cw, int rr, double (&acc)[Q][W]) { rows(cw, (long long)blockIdx.x * SW.rpi + rr, (long long)G * SW.rpi, acc); },
             [&](int cw, double (&acc)[Q][W]) {
#pragma unroll
               for (int j = 0; j < W; ++j)
#pragma unroll
                 for (int q = 0; q < Q; ++q) st_partial(at(blockIdx.x, q, cw * W + j), acc[q][j]);
             });
  if (!btc_last_arriver(counter, G)) return false;
  bn_pass<1>(S, s,
             [&](int c, int rr, double (&acc)[Q][1]) {
               int g = rr;
               for (; g + (D - 1) * S.rpi < G; g += D * S.rpi) {
                 double v[Q][D];
#pragma unroll
                 for (int u = 0; u < D; ++u)
#pragma unroll
                   for (int q = 0; q < Q; ++q) v[q][u] = btc_ld_agent(at(g + u * S.rpi, q, c));
#pragma unroll
                 for (int q = 0; q < Q; ++q) {
#pragma unroll
                   for (int h = 1; h < D; h *= 2)   // D = 8: ((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7))
#pragma unroll
                     for (int u = 0; u < D; u += 2 * h) v[q][u] += v[q][u + h];
                   acc[q][0] += v[q][0];
                 }
               }
               for (; g < G; g += S.rpi)
#pragma unroll
                 for (int q = 0; q < Q; ++q) acc[q][0] += btc_ld_agent(at(g, q, c));
             },
             [&](int c, double (&acc)[Q][1]) {
               double t[Q];
#pragma unroll
               for (int q = 0; q < Q; ++q) t[q] = acc[q][0];
               done(c, t);
             });
  if (threadIdx.x == 0) __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next call on this stream
  return true;
}

// sum_x and sum_x^2 per channel; the last workgroup turns them into mean / rstd and the running statistics
template <bool BF, bool VEC>
__global__ __launch_bounds__(BN_T) void bn_stats(const float* __restrict__ x, BnShape S, BnShape SW, double* __restrict__ partial,
                                                 int32_t* __restrict__ counter, float momentum, float eps, float* __restrict__ running_mean,
                                                 float* __restrict__ running_var, long long* __restrict__ num_batches,
                                                 float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  constexpr int W = VEC ? 4 : 1;
  const bool last = bn_reduce<W, 2, 8>(
      S, SW, partial, counter,
      [&](int cw, long long r, long long stride, double (&acc)[2][W]) {
        const long long step = stride * S.C;   // elements between two of a thread's rows: uniform, so a thread keeps ONE element index
        long long i = r * S.C + cw * W;
        for (; r + 3 * stride < S.N; r += 4 * stride, i += 4 * step) {  // 4 independent loads (W = 4: of 16 bytes) in flight
          float e0[W], e1[W], e2[W], e3[W];
          bn_ld<BF>(x, i, e0);
          bn_ld<BF>(x, i + step, e1);
          bn_ld<BF>(x, i + 2 * step, e2);
          bn_ld<BF>(x, i + 3 * step, e3);
          // all four loads issue before the first is waited for (bf16 with W = 4: left alone, the scheduler waits for each load in turn
          // to stay at 8 waves per SIMD)
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int j = 0; j < W; ++j) {
            acc[0][j] += (double)e0[j] + (double)e1[j] + (double)e2[j] + (double)e3[j];
            acc[1][j] += (double)e0[j] * e0[j] + (double)e1[j] * e1[j] + (double)e2[j] * e2[j] + (double)e3[j] * e3[j];
          }
        }
        for (; r < S.N; r += stride, i += step) {
          float e[W];
          bn_ld<BF>(x, i, e);
#pragma unroll
          for (int j = 0; j < W; ++j) { acc[0][j] += e[j]; acc[1][j] += (double)e[j] * e[j]; }
        }
      },
      [&](int c, const double (&t)[2]) {
        double mean = t[0] / S.N;
        double var = t[1] / S.N - mean * mean;  // biased, as F.batch_norm normalises with
        if (var < 0.0) var = 0.0;
        mean_out[c] = (float)mean;
        rstd_out[c] = (float)(1.0 / sqrt(var + (double)eps));
        if (running_mean) {
          double unb = S.N > 1 ? var * ((double)S.N / (double)(S.N - 1)) : var;
          running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * mean);
          running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * unb);
        }
      });
  if (last && threadIdx.x == 0 && num_batches) *num_batches += 1;   // once per launch: the last workgroup only
}

__global__ __launch_bounds__(BN_T) void bn_eval_stats(const float* __restrict__ running_mean, const float* __restrict__ running_var,
                                                      int C, float eps, float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  mean_out[c] = running_mean[c];
  rstd_out[c] = bn_rstd_eval(running_var[c], eps);
}

template <bool VEC, bool BF>
__global__ __launch_bounds__(BN_T) void bn_apply(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                 const float* __restrict__ gamma, const float* __restrict__ beta, long long total, int C,
                                                 int relu, float* __restrict__ y) {
  long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * (VEC ? 4 : 1);
  if (i >= total) return;
  if (VEC) {
    int c = (int)(i % C);
    float4 v = btc_ld4<BF>(x, i);
    float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float g = gamma ? gamma[c + j] : 1.f, b = beta ? beta[c + j] : 0.f;
      o[j] = bn_affine(o[j], mean[c + j], rstd[c + j], g, b, relu);
    }
    btc_st4<BF>(y, i, o[0], o[1], o[2], o[3]);
  } else {
    int c = (int)(i % C);
    float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    btc_st1<BF>(y, i, bn_affine(btc_ld1<BF>(x, i), mean[c], rstd[c], g, b, relu));
  }
}

// sums of g = dy * (y > 0) and g * xhat per channel; the last workgroup turns them into dbeta / dgamma
template <bool BF, bool VEC>
__global__ __launch_bounds__(BN_T) void bn_bwd_stats(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dy,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd, BnShape S, BnShape SW, int relu,
                                                     double* __restrict__ partial, int32_t* __restrict__ counter,
                                                     float* __restrict__ dgamma, float* __restrict__ dbeta) {
  constexpr int W = VEC ? 4 : 1, U = VEC ? 2 : 4;   // U rows of three streams at once: 6 16-byte or 12 4-byte loads in flight (latency bound)
  bn_reduce<W, 2, 8>(
      S, SW, partial, counter,
      [&](int cw, long long r, long long stride, double (&acc)[2][W]) {
        float m[W], rs[W];
#pragma unroll
        for (int j = 0; j < W; ++j) { m[j] = mean[cw * W + j]; rs[j] = rstd[cw * W + j]; }
        const long long step = stride * S.C;   // (as in bn_stats)
        long long i = r * S.C + cw * W;
        for (; r + (U - 1) * stride < S.N; r += U * stride, i += U * step) {
          float gv[U][W], yv[U][W], xv[U][W];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            bn_ld<BF>(dy, i + u * step, gv[u]);
            bn_ld<BF>(y, i + u * step, yv[u]);
            bn_ld<BF>(x, i + u * step, xv[u]);
          }
          // (a row's terms are written out here and in the tail: through a shared lambda the bf16 W = 4 instance waits for four of its
          // six loads before it issues the last two)
#pragma unroll
          for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < W; ++j) {
              const float g = (relu && !(yv[u][j] > 0.f)) ? 0.f : gv[u][j];
              acc[0][j] += (double)g;
              acc[1][j] += (double)g * ((xv[u][j] - m[j]) * rs[j]);
            }
        }
        for (; r < S.N; r += stride, i += step) {
          float gv[W], yv[W], xv[W];
          bn_ld<BF>(dy, i, gv);
          bn_ld<BF>(y, i, yv);
          bn_ld<BF>(x, i, xv);
#pragma unroll
          for (int j = 0; j < W; ++j) {
            const float g = (relu && !(yv[j] > 0.f)) ? 0.f : gv[j];
            acc[0][j] += (double)g;
            acc[1][j] += (double)g * ((xv[j] - m[j]) * rs[j]);
          }
        }
      },
      [&](int c, const double (&t)[2]) {
        dbeta[c] = (float)t[0];
        dgamma[c] = (float)t[1];
      });
}

template <bool VEC, bool BF>
__global__ __launch_bounds__(BN_T) void bn_bwd_apply(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dy,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                     const float* __restrict__ dbeta, long long total, int C, int N, int relu, int training,
                                                     float* __restrict__ dx) {
  long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * (VEC ? 4 : 1);
  if (i >= total) return;
  const float invn = 1.0f / (float)N;
  constexpr int W = VEC ? 4 : 1;
  float xv[W], yv[W], gv[W];
  if (VEC) {
    float4 a = btc_ld4<BF>(x, i), b = btc_ld4<BF>(y, i), c4 = btc_ld4<BF>(dy, i);
    xv[0] = a.x; xv[W > 1 ? 1 : 0] = a.y; xv[W > 2 ? 2 : 0] = a.z; xv[W > 3 ? 3 : 0] = a.w;
    yv[0] = b.x; yv[W > 1 ? 1 : 0] = b.y; yv[W > 2 ? 2 : 0] = b.z; yv[W > 3 ? 3 : 0] = b.w;
    gv[0] = c4.x; gv[W > 1 ? 1 : 0] = c4.y; gv[W > 2 ? 2 : 0] = c4.z; gv[W > 3 ? 3 : 0] = c4.w;
  } else {
    xv[0] = btc_ld1<BF>(x, i); yv[0] = btc_ld1<BF>(y, i); gv[0] = btc_ld1<BF>(dy, i);
  }
  const int c = (int)(i % C);
  float o[W];
#pragma unroll
  for (int j = 0; j < W; ++j) {
    float g = gv[j];
    if (relu && !(yv[j] > 0.f)) g = 0.f;
    const float gm = gamma ? gamma[c + j] : 1.f, rs = rstd[c + j];
    if (training) {
      float xh = (xv[j] - mean[c + j]) * rs;
      o[j] = gm * rs * (g - dbeta[c + j] * invn - xh * dgamma[c + j] * invn);
    } else {
      o[j] = gm * rs * g;
    }
  }
  if (VEC) btc_st4<BF>(dx, i, o[0], o[W > 1 ? 1 : 0], o[W > 2 ? 2 : 0], o[W > 3 ? 3 : 0]);
  else btc_st1<BF>(dx, i, o[0]);
}

// column sums of an (N, C) matrix (the bias gradient of a sparse conv): bn_reduce with one sum per channel, one partial in flight
template <bool BF>
__global__ __launch_bounds__(BN_T) void col_sum(const float* __restrict__ x, BnShape S, double* __restrict__ partial,
                                                int32_t* __restrict__ counter, float* __restrict__ out) {
  bn_reduce<1, 1, 1>(
      S, S, partial, counter,
      [&](int c, long long r, long long stride, double (&acc)[1][1]) {
        for (; r + 3 * stride < S.N; r += 4 * stride) {
          float v0 = btc_ld1<BF>(x, r * S.C + c), v1 = btc_ld1<BF>(x, (r + stride) * S.C + c), v2 = btc_ld1<BF>(x, (r + 2 * stride) * S.C + c),
                v3 = btc_ld1<BF>(x, (r + 3 * stride) * S.C + c);
          acc[0][0] += ((double)v0 + (double)v1) + ((double)v2 + (double)v3);
        }
        for (; r < S.N; r += stride) acc[0][0] += (double)btc_ld1<BF>(x, r * S.C + c);
      },
      [&](int c, const double (&t)[1]) { out[c] = (float)t[0]; });
}

BnShape bn_shape(int N, int C) {
  BnShape S;
  S.N = N;
  S.C = C;
  int cp = 1;
  while (cp < C && cp < BN_T) cp <<= 1;
  S.cpow = cp;
  S.rpi = BN_T / cp;
  return S;
}

// bwd: three input streams per row and no dependent second pass behind it -> more, thinner workgroups
int bn_grid_bwd(int N, const BnShape& S) {
  int g = btc_cdiv(N, S.rpi * 16);
  if (g > 512) g = 512;
  if (g < 1) g = 1;
  return g;
}

int bn_grid(int N, const BnShape& S) {
  int g = btc_cdiv(N, S.rpi * 64);  // >= 64 rows per thread-row before adding another workgroup: the last-arriver
  if (g > 256) g = 256;            // reduction walks all partials, so few, fat workgroups win at BtcDet's sizes
  if (g < 1) g = 1;
  return g;
}

// vectorised statistics passes: one workgroup per `kb` KB of input (tuning keys override), at most one per CU.  Few, fat
// workgroups: the last arriver walks every workgroup's partial sums, and that walk -- not the pass over the data -- bounds
// these launches at BtcDet's sizes (tools/bn_bench.py)
int bn_grid_bytes(long long bytes, int tune_key, int kb_default) {
  const int t = btc_tune_get(tune_key);
  const long long per = 1024LL * (t > 0 ? t : kb_default);
  long long g = (bytes + per - 1) / per;
  return (int)(g > 256 ? 256 : (g < 1 ? 1 : g));
}

// the workspace of every entry point below (btc_bn_ws_bytes): the first 256 bytes hold the arrival counter, zero on entry and zero on
// exit; the partial sums behind it may hold anything
struct BnWs {
  int32_t* counter;
  double* partial;
  explicit BnWs(void* ws) : counter((int32_t*)ws), partial((double*)((char*)ws + 256)) {}
};

// the one choice of channels per thread: W = 4 when C % 4 == 0 (16-byte moves, bf16: 8), else 1.  f(W as a constant, SW) launches
template <class F>
int bn_by_width(int N, int C, F&& f) {
  if ((C & 3) == 0) return f(std::integral_constant<int, 4>(), bn_shape(N, C >> 2));
  return f(std::integral_constant<int, 1>(), bn_shape(N, C));
}

}  // namespace

extern "C" size_t btc_bn_ws_bytes(int C) { return 256 + btc_align((size_t)512 * 2 * C * sizeof(double)); }

template <bool BF>
static int bn_fwd_impl(const float* x, int N, int C, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, long long* num_batches_tracked, float momentum, float eps, int training, int relu,
                               float* y, float* save_mean, float* save_rstd, void* ws_, size_t ws_bytes, void* stream_, bool have_stats = false) {
  // have_stats: save_mean / save_rstd (and the running statistics) were produced by the conv kernel's epilogue (bn_fuse.h): apply only
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(N >= 1 && C >= 1, "btc_bn_relu_fwd: empty input");
  BTC_CHECK_ARG(ws_bytes >= btc_bn_ws_bytes(C), "btc_bn_relu_fwd: workspace too small");
  BTC_CHECK_ARG(training || (running_mean && running_var), "btc_bn_relu_fwd: eval mode needs running statistics");
  const BnWs ws(ws_);
  const BnShape S = bn_shape(N, C);
  const long long total = (long long)N * C;
  return bn_by_width(N, C, [&](auto w, const BnShape& SW) {
    constexpr int W = decltype(w)::value;
    if (!have_stats && training) {
      const int g = W == 4 ? bn_grid_bytes(total * (BF ? 2 : 4), BTC_TUNE_BN_FWD_KB, 64) : bn_grid(N, S);
      bn_stats<BF, W == 4><<<g, BN_T, 0, stream>>>(x, S, SW, ws.partial, ws.counter, momentum, eps, running_mean, running_var,
                                                    num_batches_tracked, save_mean, save_rstd);
    } else if (!have_stats) {
      bn_eval_stats<<<btc_cdiv(C, BN_T), BN_T, 0, stream>>>(running_mean, running_var, C, eps, save_mean, save_rstd);
    }
    BTC_LAUNCH_CHECK();
    bn_apply<W == 4, BF><<<btc_cdiv(total / W, BN_T), BN_T, 0, stream>>>(x, save_mean, save_rstd, gamma, beta, total, C, relu, y);
    BTC_LAUNCH_CHECK();
    return BTC_OK;
  });
}

template <bool BF>
static int bn_bwd_impl(const float* x, const float* y, const float* dy, int N, int C, const float* gamma, const float* save_mean,
                               const float* save_rstd, int training, int relu, float* dx, float* dgamma, float* dbeta, void* ws_,
                               size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(N >= 1 && C >= 1, "btc_bn_relu_bwd: empty input");
  BTC_CHECK_ARG(ws_bytes >= btc_bn_ws_bytes(C), "btc_bn_relu_bwd: workspace too small");
  const BnWs ws(ws_);
  const BnShape S = bn_shape(N, C);
  const long long total = (long long)N * C;
  return bn_by_width(N, C, [&](auto w, const BnShape& SW) {
    constexpr int W = decltype(w)::value;
    const int g = W == 4 ? bn_grid_bytes(total * (BF ? 6 : 12), BTC_TUNE_BN_BWD_KB, 128) : bn_grid_bwd(N, S);
    bn_bwd_stats<BF, W == 4><<<g, BN_T, 0, stream>>>(x, y, dy, save_mean, save_rstd, S, SW, relu, ws.partial, ws.counter, dgamma, dbeta);
    BTC_LAUNCH_CHECK();
    bn_bwd_apply<W == 4, BF><<<btc_cdiv(total / W, BN_T), BN_T, 0, stream>>>(x, y, dy, save_mean, save_rstd, gamma, dgamma, dbeta, total, C, N,
                                                                             relu, training, dx);
    BTC_LAUNCH_CHECK();
    return BTC_OK;
  });
}

// out[c] = sum over rows of x[r][c] (fp64 accumulation, deterministic).  ws as for btc_bn_relu_fwd.
template <bool BF>
static int col_sum_impl(const float* x, int N, int C, float* out, void* ws_, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BTC_CHECK_ARG(N >= 1 && C >= 1, "btc_col_sum: empty input");
  BTC_CHECK_ARG(ws_bytes >= btc_bn_ws_bytes(C), "btc_col_sum: workspace too small");
  const BnWs ws(ws_);
  const BnShape S = bn_shape(N, C);
  col_sum<BF><<<bn_grid_bwd(N, S), BN_T, 0, stream>>>(x, S, ws.partial, ws.counter, out);
  BTC_LAUNCH_CHECK();
  return BTC_OK;
}

extern "C" int btc_col_sum(const float* x, int N, int C, float* out, void* ws, size_t ws_bytes, void* stream) {
  return col_sum_impl<false>(x, N, C, out, ws, ws_bytes, stream);
}

extern "C" int btc_col_sum_bf16(const void* x, int N, int C, float* out, void* ws, size_t ws_bytes, void* stream) {
  return col_sum_impl<true>((const float*)x, N, C, out, ws, ws_bytes, stream);
}

extern "C" int btc_bn_relu_fwd(const float* x, int N, int C, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, long long* num_batches_tracked, float momentum, float eps, int training, int relu,
                               float* y, float* save_mean, float* save_rstd, void* ws, size_t ws_bytes, void* stream) {
  return bn_fwd_impl<false>(x, N, C, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, training, relu, y, save_mean,
                            save_rstd, ws, ws_bytes, stream);
}

extern "C" int btc_bn_relu_bwd(const float* x, const float* y, const float* dy, int N, int C, const float* gamma, const float* save_mean,
                               const float* save_rstd, int training, int relu, float* dx, float* dgamma, float* dbeta, void* ws,
                               size_t ws_bytes, void* stream) {
  return bn_bwd_impl<false>(x, y, dy, N, C, gamma, save_mean, save_rstd, training, relu, dx, dgamma, dbeta, ws, ws_bytes, stream);
}

// bfloat16 activations (x, y, dy, dx); parameters, statistics and their gradients stay fp32
extern "C" int btc_bn_relu_fwd_bf16(const void* x, int N, int C, const float* gamma, const float* beta, float* running_mean,
                                    float* running_var, long long* num_batches_tracked, float momentum, float eps, int training, int relu,
                                    void* y, float* save_mean, float* save_rstd, void* ws, size_t ws_bytes, void* stream) {
  return bn_fwd_impl<true>((const float*)x, N, C, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, training, relu,
                           (float*)y, save_mean, save_rstd, ws, ws_bytes, stream);
}

extern "C" int btc_bn_relu_bwd_bf16(const void* x, const void* y, const void* dy, int N, int C, const float* gamma, const float* save_mean,
                                    const float* save_rstd, int training, int relu, void* dx, float* dgamma, float* dbeta, void* ws,
                                    size_t ws_bytes, void* stream) {
  return bn_bwd_impl<true>((const float*)x, (const float*)y, (const float*)dy, N, C, gamma, save_mean, save_rstd, training, relu, (float*)dx,
                           dgamma, dbeta, ws, ws_bytes, stream);
}

// ---- conv -> BatchNorm (training) -> ReLU with the statistics gathered in the conv's epilogue -------------------------------
extern "C" size_t btc_bn_fuse_ws_bytes(void) { return btc_bn_fuse_bytes(); }

extern "C" int btc_conv_bn_relu_fwd(int operands, const void* src, const void* W, const float* bias, const int32_t* nbr, const int32_t* order,
                                    int n_rows, int K, int Cin, int Cout, void* x, const float* gamma, const float* beta, float* running_mean,
                                    float* running_var, long long* num_batches_tracked, float momentum, float eps, int relu, void* y,
                                    float* save_mean, float* save_rstd, void* ws, size_t ws_bytes, void* fuse_ws, void* stream) {
  return btc_conv_bn_relu_fwd_src(operands, src, -1LL, W, bias, nbr, order, n_rows, K, Cin, Cout, x, gamma, beta, running_mean, running_var,
                                  num_batches_tracked, momentum, eps, relu, y, save_mean, save_rstd, ws, ws_bytes, fuse_ws, stream);
}

extern "C" int btc_conv_bn_relu_fwd_src(int operands, const void* src, long long src_rows, const void* W, const float* bias, const int32_t* nbr,
                                        const int32_t* order, int n_rows, int K, int Cin, int Cout, void* x, const float* gamma, const float* beta,
                                        float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps, int relu,
                                        void* y, float* save_mean, float* save_rstd, void* ws, size_t ws_bytes, void* fuse_ws, void* stream) {
  BTC_CHECK_ARG(n_rows >= 1, "btc_conv_bn_relu_fwd: empty input");
  BTC_CHECK_ARG(operands >= BTC_OPERANDS_F32 && operands <= BTC_OPERANDS_F32_SPLIT, "btc_conv_bn_relu_fwd: operands=%d", operands);
  const bool bf = operands == BTC_OPERANDS_BF16_ACT || operands == BTC_OPERANDS_BF16;
  const bool fused = fuse_ws && Cout <= BN_FUSE_CMAX && btc_tune_get(BTC_TUNE_BN_FUSE) != 1;
  BnFuse bn = btc_bn_fuse_none();   // (statistics mode: the eval-mode fields stay null)
  if (fused) {
    bn.counter = (int32_t*)fuse_ws;
    bn.slots = (double*)((char*)fuse_ws + 256);
    bn.mean_out = save_mean; bn.rstd_out = save_rstd;
    bn.running_mean = running_mean; bn.running_var = running_var; bn.num_batches = num_batches_tracked;
    bn.momentum = momentum; bn.eps = eps; bn.N = n_rows; bn.C = Cout; bn.nslots = btc_bn_fuse_nslots(n_rows);
  }
  const int rc = btc_apply("btc_conv_bn_relu_fwd_src", BTC_PASS_FWD, operands, src, src_rows, W, bias, nbr, order, n_rows, K, Cin, Cout, x,
                           (hipStream_t)stream, fused ? &bn : nullptr);
  if (rc) return rc;
  if (bf)
    return bn_fwd_impl<true>((const float*)x, n_rows, Cout, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, 1, relu,
                             (float*)y, save_mean, save_rstd, ws, ws_bytes, stream, fused);
  return bn_fwd_impl<false>((const float*)x, n_rows, Cout, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, 1, relu,
                            (float*)y, save_mean, save_rstd, ws, ws_bytes, stream, fused);
}

// ---- conv -> BatchNorm (eval: running statistics) -> ReLU in ONE launch: the affine and the ReLU in the conv's epilogue, only y is written
// (bn_fuse.h, second mode; a z-split launch of the split-operand kernel applies them in its reduction)
extern "C" int btc_conv_bn_eval_fwd(int operands, const void* src, long long src_rows, const void* W, const float* bias, const int32_t* nbr,
                                    const int32_t* order, int n_rows, int K, int Cin, int Cout, const float* gamma, const float* beta,
                                    const float* running_mean, const float* running_var, float eps, int relu, void* y, void* stream) {
  BTC_CHECK_ARG(n_rows >= 1, "btc_conv_bn_eval_fwd: empty input");
  BTC_CHECK_ARG(operands >= BTC_OPERANDS_F32 && operands <= BTC_OPERANDS_F32_SPLIT, "btc_conv_bn_eval_fwd: operands=%d", operands);
  BTC_CHECK_ARG(running_mean && running_var, "btc_conv_bn_eval_fwd: eval mode needs running statistics");
  BTC_CHECK_ARG(src && W && nbr && y, "btc_conv_bn_eval_fwd: null operand");
  BnFuse bn = btc_bn_fuse_none();
  bn.ev_mean = running_mean; bn.ev_var = running_var; bn.ev_gamma = gamma; bn.ev_beta = beta; bn.ev_relu = relu ? 1 : 0;
  bn.eps = eps; bn.N = n_rows; bn.C = Cout;
  return btc_apply("btc_conv_bn_eval_fwd", BTC_PASS_FWD, operands, src, src_rows, W, bias, nbr, order, n_rows, K, Cin, Cout, y, (hipStream_t)stream, &bn);
}
