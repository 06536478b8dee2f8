/*
 * scsfm_stem.h -- C ABI of libscsfm_stem.so: the ResNet stem's train-mode BatchNorm + ReLU fused with the 3x3 / stride 2
 * / pad 1 max-pool behind it, forward and backward, as hand-written HIP kernels for gfx950 (MI355X).  One forward
 * writes f0 = relu(bn(x)), the pooled map and its one-byte argmax from a single read of x; the backward re-derives the
 * gradient of f0 from the pooled gradient, the argmax bytes and x, so the full-resolution pooling gradient and its sum
 * with the skip connection's gradient never exist in memory.
 *
 * Conventions (as include/scsfm_enc.h, whose rules these entry points keep to the bit)
 *  - All pointers are DEVICE pointers; activations are contiguous NCHW fp32, per-channel vectors are fp32[C]; the
 *    caller owns every buffer; nothing is retained.  Every array has fewer than 2^31 elements.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_ERR_ARG (-1) for a rejected argument (nothing is launched then), otherwise the
 *    hipError_t of the failed launch.  Every output is stored (overwritten), never accumulated; the running statistics
 *    and the batch counter are the only arrays updated in place.
 *  - `ws` is scratch of at least scsfm_stem_workspace_bytes(B, C, H, W) bytes, 8-byte aligned, private to the call
 *    until it has run; its contents before and after are meaningless.
 *  - bn(x) = fmaf(xhat, gamma, beta), xhat = ((x - mean) - mean_lo) * invstd with the batch's per-channel mean and
 *    biased variance over N = B*H*W >= 2 entries; relu(v) = v > 0 ? v : 0, a NaN is passed on.
 *  - Pooling: PH = (H - 1) / 2 + 1, PW = (W - 1) / 2 + 1; window (ph, pw) covers rows 2ph-1.. and columns 2pw-1..,
 *    clipped to the plane; row-major scan, the first maximum wins, a NaN wins; arg = 3 * dh + dw.
 *  - All sums are accumulated in fp64 in a fixed order: two calls on the same input give the same bits.  No
 *    floating-point atomics anywhere.
 *  - Any H, W >= 1.  The fast kernels (16-byte accesses) run where W is a multiple of 4 and x, f0, g_f0 and dx are
 *    16-byte, the pooled fp32 maps 8-byte and the argmax 2-byte aligned; every other case takes the scalar kernels.
 */
#ifndef SCSFM_STEM_H_
#define SCSFM_STEM_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 (first version) */
int scsfm_stem_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: stem_source_id) into buf, NUL-terminated */
int scsfm_stem_source_id(char* buf, size_t n);

/* bytes of scratch the two entry points need for x[B,C,H,W]; 0 for a shape they reject */
size_t scsfm_stem_workspace_bytes(int B, int C, int H, int W);

/* f0[B,C,H,W] = relu(bn(x)), out[B,C,PH,PW] = its max-pool and arg[B,C,PH,PW] (one byte each) the winners' positions.
   stat[3*C], running_mean / running_var[C] and num_batches_tracked[0] exactly as scsfm_enc_bn_fwd_f32 leaves them on
   the same input (same partition and summation tree); f0, out and arg are the bits of scsfm_enc_bn_fwd_f32 (mode 1)
   followed by scsfm_enc_maxpool_fwd_f32. */
int scsfm_stem_fwd_f32(int B, int C, int H, int W, double eps, double momentum, const float* x, const float* gamma,
                       const float* beta, float* f0, float* out, unsigned char* arg, float* stat, float* running_mean,
                       float* running_var, long long* num_batches_tracked, void* ws, size_t ws_bytes, void* stream);

/* The backward of the above for the gradients g_pool[B,C,PH,PW] of out and g_f0[B,C,H,W] of f0 (NULL: f0 has no
   gradient, nothing is read for it).  Per entry i of f0: p = 0 plus g_pool of the (at most four) windows whose winner
   i is, in ascending (ph, pw) order; t = p + g_f0[i]; g' = t where the forward's ReLU let the value through (mask
   recomputed from x with the forward's expression; a NaN passes).  dbeta[C] = sum g', dgamma[C] = sum g' * xhat,
   dx = gamma * invstd * (g' - dbeta / N - xhat * dgamma / N). */
int scsfm_stem_bwd_f32(int B, int C, int H, int W, const float* g_pool, const float* g_f0, const unsigned char* arg,
                       const float* x, const float* gamma, const float* beta, const float* stat, float* dx,
                       float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_STEM_H_ */
