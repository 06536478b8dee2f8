/*
 * scsfm_enc.h -- C ABI of libscsfm_enc.so: the memory-bound glue of the ResNet encoder (models/resnet_encoder.py) as
 * hand-written HIP kernels for gfx950 (MI355X): train-mode BatchNorm fused with the residual add and the ReLU that
 * follow it, forward and backward, and the stem's 3x3 / stride 2 / pad 1 max-pool with a one-byte argmax.  The
 * convolutions stay MIOpen's.
 *
 * Conventions (as include/scsfm_nets.h)
 *  - All pointers are DEVICE pointers; activations are contiguous NCHW fp32, per-channel vectors are fp32[C]; the
 *    caller owns every buffer; nothing is retained.  Every array has fewer than 2^31 elements.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_ERR_ARG (-1) for a rejected argument (nothing is launched then), otherwise the
 *    hipError_t of the failed launch.  Every output is stored (overwritten), never accumulated; the running statistics
 *    and the batch counter are the only arrays updated in place.
 *  - `ws` is scratch of at least scsfm_enc_bn_workspace_bytes(B, C, H, W) bytes, 8-byte aligned, private to the call
 *    until it has run; its contents before and after are meaningless.
 *  - mode: 0  y = bn(x);  1  y = relu(bn(x));  2  y = relu(bn(x) + identity).
 *    bn(x) = fmaf((x - mean) * invstd, gamma, beta) with the batch's per-channel mean and biased variance over
 *    N = B*H*W >= 2 entries, invstd = 1 / sqrt(var + eps).  relu(v) = v > 0 ? v : 0, a NaN is passed on.
 *  - All sums (batch statistics, dgamma, dbeta) are accumulated in fp64 in a fixed order: two calls on the same input
 *    give the same bits.  No floating-point atomics anywhere.
 */
#ifndef SCSFM_ENC_H_
#define SCSFM_ENC_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 (first version) */
int scsfm_enc_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: enc_source_id) into buf, NUL-terminated */
int scsfm_enc_source_id(char* buf, size_t n);

/* bytes of scratch the two BatchNorm entry points need for x[B,C,H,W]; 0 for a shape they reject */
size_t scsfm_enc_bn_workspace_bytes(int B, int C, int H, int W);

/* y[B,C,H,W] by `mode` from x (and identity[B,C,H,W], mode 2 only; otherwise unused, may be NULL).
   stat[3*C]: mean (rounded to fp32), invstd, and the part of the fp64 mean its fp32 rounding lost -- what the backward
   needs.  running_mean / running_var[C] <- (1 - momentum) * running + momentum * (mean | var * N / (N - 1));
   num_batches_tracked[0] (int64) += 1. */
int scsfm_enc_bn_fwd_f32(int B, int C, int H, int W, int mode, double eps, double momentum, const float* x,
                         const float* identity, const float* gamma, const float* beta, float* y, float* stat,
                         float* running_mean, float* running_var, long long* num_batches_tracked, void* ws,
                         size_t ws_bytes, void* stream);

/* The backward of the above for the gradient g[B,C,H,W] of y.  g' = g where y > 0 (mode 0: everywhere); the mask is
   recomputed from x with the forward's expression in mode 1 and read from y (the forward's output) in mode 2; y is
   unused (may be NULL) otherwise.  dbeta[C] = sum g', dgamma[C] = sum g' * xhat,
   dx = gamma * invstd * (g' - dbeta / N - xhat * dgamma / N), and d_identity[B,C,H,W] = g' in mode 2 (unused, may be
   NULL, otherwise). */
int scsfm_enc_bn_bwd_f32(int B, int C, int H, int W, int mode, const float* g, const float* x, const float* y,
                         const float* gamma, const float* beta, const float* stat, float* dx, float* d_identity,
                         float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);

/* out[B,C,PH,PW] = max-pool 3x3 / stride 2 / pad 1 of x[B,C,H,W], PH = (H - 1) / 2 + 1, PW = (W - 1) / 2 + 1, and
   arg[B,C,PH,PW] (one byte each): the winner's position 3 * dh + dw in its window (rows 2ph-1.., columns 2pw-1..).
   Row-major scan, the first maximum wins, a NaN wins (ATen's rule). */
int scsfm_enc_maxpool_fwd_f32(int B, int C, int H, int W, const float* x, float* out, unsigned char* arg, void* stream);
/* dx[B,C,H,W]: every entry is 0 plus the gradients g[B,C,PH,PW] of the (at most four) windows whose winner it is, in
   ascending (ph, pw) order */
int scsfm_enc_maxpool_bwd_f32(int B, int C, int H, int W, const float* g, const unsigned char* arg, float* dx,
                              void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_ENC_H_ */
