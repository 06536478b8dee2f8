/*
 * scsfm_fbn.h -- C ABI of libscsfm_fbn.so: the backward of the ResNet encoder's BatchNorm with FROZEN statistics
 * (train.py --freeze-bn; scsfm_hip/encoder_frozen.py) fused with the backward of the residual add and the ReLU behind it,
 * as hand-written HIP kernels for gfx950 (MI355X).  The forward of such a site is libscsfm_enceval.so's
 * scsfm_enceval_bn_f32: with the running statistics held, BatchNorm is a per-channel affine map, so the input gradient is
 * the masked upstream gradient times a per-channel factor and does not wait for any sum.  One launch streams the
 * gradient once, stores dx (and d_identity) and leaves the partial sums of the parameter gradients in a workspace; a
 * second, small launch adds them.
 *
 * Conventions (as include/scsfm_enceval.h)
 *  - All pointers are DEVICE pointers; activations are contiguous NCHW fp32, per-channel vectors are fp32[C]; the
 *    caller owns every buffer; nothing is retained.  Every array has fewer than 2^31 elements.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates, and there
 *    are no atomics: two calls on the same inputs give the same bits.
 *  - Return value: 0 on success, SCSFM_ERR_ARG (-1) for a rejected argument (nothing is launched then), otherwise the
 *    hipError_t of the failed launch.  Every output is stored (overwritten); no input is written -- the running
 *    statistics and gamma are read only.  Outputs must not alias inputs.
 *  - Rejected: a non-positive dimension, 2^31 or more elements, a NULL required pointer, a mode outside 0..2, an eps
 *    that is negative or not finite, parameter gradients given by halves (see below), a workspace that is too small.
 *  - mode names the forward, as include/scsfm_enceval.h:  0  y = bn(x);  1  y = relu(bn(x));  2  y = relu(bn(x) + identity).
 *    With g the gradient of y and  m = g (mode 0)  or  m = y <= 0 ? 0 : g (modes 1, 2: where y is a NaN the gradient
 *    passes, as in include/scsfm_enc.h):
 *        invstd[c]  = 1.0f / sqrtf(running_var[c] + (float)eps)          (libscsfm_enceval.so's expression)
 *        dx         = m * (gamma[c] * invstd[c])
 *        d_identity = m                                                   (mode 2)
 *        dbeta[c]   = sum over b, h, w of m
 *        dgamma[c]  = sum over b, h, w of m * ((x - running_mean[c]) * invstd[c])
 *    The sums are accumulated in double, in an order fixed by the shape and the pointers' alignment, and stored as fp32.
 */
#ifndef SCSFM_FBN_H_
#define SCSFM_FBN_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 (first version) */
int scsfm_fbn_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: fbn_source_id) into buf, NUL-terminated */
int scsfm_fbn_source_id(char* buf, size_t n);

/* bytes of workspace that scsfm_fbn_bn_bwd_f32 needs for the parameter gradients of this shape (0 for a rejected shape);
   the workspace must be 8-byte aligned and need not be initialised */
size_t scsfm_fbn_workspace_bytes(int B, int C, int H, int W);

/* dx[B,C,H,W] (and d_identity[B,C,H,W], mode 2 only; otherwise unused, may be NULL) from g[B,C,H,W] and y[B,C,H,W]
   (modes 1 and 2 only; otherwise unused, may be NULL).
   dgamma[C] and dbeta[C] are both NULL, or both given together with x[B,C,H,W] and ws of ws_bytes >=
   scsfm_fbn_workspace_bytes(B, C, H, W); anything in between is rejected.  With both NULL, x, running_mean and ws are
   unused and may be NULL, nothing is reduced and the call is one launch. */
int scsfm_fbn_bn_bwd_f32(int B, int C, int H, int W, int mode, double eps, const float* g, const float* x, const float* y,
                         const float* gamma, const float* running_mean, const float* running_var, float* dx,
                         float* d_identity, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_FBN_H_ */
