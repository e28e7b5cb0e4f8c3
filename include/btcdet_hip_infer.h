/* btcdet_hip_infer.h -- inference entry points of libbtcdet_hip.so (gfx950), the second public header beside btcdet_hip.h.
 *
 * Same common rules as btcdet_hip.h: every pointer is a DEVICE pointer unless its name starts with h_; the caller allocates every
 * buffer; `stream` is a hipStream_t (NULL = the default stream) and every call only enqueues work on it; an entry point returns
 * BTC_OK or a BTC_E* code, with the text in btc_last_error(), and never exits the process.  The constants (BTC_OK, BTC_OPERANDS_*)
 * are those of btcdet_hip.h. */
#ifndef BTCDET_HIP_INFER_H
#define BTCDET_HIP_INFER_H

#include <stddef.h>
#include <stdint.h>

#include "btcdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sparse conv -> BatchNorm1d in EVAL mode (running statistics) -> optional ReLU as ONE launch, for a forward pass nobody
 * differentiates: the conv kernel applies
 *
 *     y[r][c] = relu?( (v - running_mean[c]) * rstd[c] * gamma[c] + beta[c] ),   rstd[c] = 1.0f / sqrtf(running_var[c] + eps)
 *
 * in its epilogue, to the result tile it holds in registers, where v is the value btc_conv_apply_src would have stored in its
 * result (bias added; for bf16 activations rounded to bf16 and widened again).  Only y [n_rows][Cout] (activation type of
 * `operands`) is written: no conv result, no saved statistics, no BatchNorm workspace.  y is bit-identical to
 * btc_conv_apply_src(BTC_PASS_FWD, ...) followed by btc_bn_relu_fwd[_bf16](training = 0) on the same inputs.
 *
 *   operands, src, src_rows, W, bias, nbr, order, n_rows, K, Cin, Cout : as btc_conv_apply_src with pass = BTC_PASS_FWD (every
 *       operand kind; src_rows is required for BTC_OPERANDS_F32_SPLIT; order may be NULL).  n_rows >= 1.
 *   gamma, beta   : [Cout] fp32, each may be NULL (1 / 0)
 *   running_mean, running_var : [Cout] fp32, READ ONLY (num_batches_tracked is not an argument: nothing is tracked)
 *   Cout <= 1024. */
int btc_conv_bn_eval_fwd(int operands, const void* src, long long src_rows, const void* W, const float* bias, const int32_t* nbr,
                         const int32_t* order, int n_rows, int K, int Cin, int Cout, const float* gamma, const float* beta,
                         const float* running_mean, const float* running_var, float eps, int relu, void* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BTCDET_HIP_INFER_H */
