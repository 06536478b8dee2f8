/*
 * scsfm_enceval.h -- C ABI of libscsfm_enceval.so: the memory-bound glue of the ResNet encoder (models/resnet_encoder.py)
 * in EVAL mode as hand-written HIP kernels for gfx950 (MI355X): BatchNorm from the running statistics fused with the
 * residual add and the ReLU that follow it, the stem's BatchNorm / ReLU fused with its 3x3 / stride 2 / pad 1 max-pool,
 * and that max-pool alone.  Forward only: eval-mode BatchNorm is a per-channel affine map, there is no batch reduction,
 * no workspace and (here) no backward.  The convolutions stay MIOpen's; the training-mode glue is libscsfm_enc.so's and
 * libscsfm_stem.so's.
 *
 * Conventions (as include/scsfm_enc.h)
 *  - All pointers are DEVICE pointers; activations are contiguous NCHW fp32, per-channel vectors are fp32[C]; the
 *    caller owns every buffer; nothing is retained.  Every array has fewer than 2^31 elements.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates, and there
 *    are no atomics.
 *  - Return value: 0 on success, SCSFM_ERR_ARG (-1) for a rejected argument (nothing is launched then), otherwise the
 *    hipError_t of the failed launch.  Every output is stored (overwritten); no input is written -- the running
 *    statistics, gamma and beta are read only.  Outputs must not alias inputs.
 *  - Rejected: a non-positive dimension, 2^31 or more elements, a NULL required pointer, a mode outside 0..2, an eps
 *    that is negative or not finite.
 *  - mode: 0  y = bn(x);  1  y = relu(bn(x));  2  y = relu(bn(x) + identity).
 *    bn(x) = fmaf((x - running_mean[c]) * invstd[c], gamma[c], beta[c]) with
 *    invstd[c] = 1.0f / sqrtf(running_var[c] + (float)eps): libscsfm_enc.so's expression with the running statistics in
 *    place of the batch's.  relu(v) = v > 0 ? v : 0, a NaN is passed on.
 *  - The max-pool scans its window row-major, the first maximum wins, a NaN wins (ATen's rule, as include/scsfm_enc.h);
 *    no argmax is stored.
 */
#ifndef SCSFM_ENCEVAL_H_
#define SCSFM_ENCEVAL_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 (first version) */
int scsfm_enceval_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: enceval_source_id) into buf, NUL-terminated */
int scsfm_enceval_source_id(char* buf, size_t n);

/* y[B,C,H,W] by `mode` from x (and identity[B,C,H,W], mode 2 only; otherwise unused, may be NULL) */
int scsfm_enceval_bn_f32(int B, int C, int H, int W, int mode, double eps, const float* x, const float* identity,
                         const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                         float* y, void* stream);

/* The stem: f0[B,C,H,W] = relu(bn(x)) and pooled[B,C,PH,PW] = max-pool 3x3 / stride 2 / pad 1 of f0,
   PH = (H - 1) / 2 + 1, PW = (W - 1) / 2 + 1, from one pass over x.  f0 has the bits of mode 1 above. */
int scsfm_enceval_bn_relu_pool_f32(int B, int C, int H, int W, double eps, const float* x, const float* gamma,
                                   const float* beta, const float* running_mean, const float* running_var, float* f0,
                                   float* pooled, void* stream);

/* out[B,C,PH,PW] = the same max-pool of x[B,C,H,W] */
int scsfm_enceval_maxpool_f32(int B, int C, int H, int W, const float* x, float* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_ENCEVAL_H_ */
