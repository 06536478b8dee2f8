/*
 * scsfm_pw.h -- C ABI of libscsfm_pw.so: the weight gradient and the stride-2 data gradient of the encoders' 1x1
 * ("pointwise") convolutions -- the down-sample branches of the ResNet stages and the pose decoder's squeeze -- as
 * hand-written HIP kernels for gfx950 (MI355X) on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32.
 *
 * With stride s in {1, 2}, x[B, Cin, H, W], Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1, dy[B, Cout, Ho, Wo] and
 * w[Cout, Cin] (the convolution's [Cout, Cin, 1, 1]):
 *
 * 1. The weight gradient
 *
 *     dW[co][ci] = sum over n, y, x of  dy[n][co][y][x] * x[n][ci][s y][s x]
 *
 * Both operands are read as they lie (NCHW), x at the sampled positions only.  The pixels are split over workgroups (and
 * the Cout x Cin tiles of 128 x 64 as well); every workgroup leaves one fp32 partial in `ws`, a second launch adds the
 * partials of an entry in fp64 in a fixed order and rounds once.  No transposed copy, no zero-fill, no atomics: the
 * same input gives the same bits, call after call.
 *
 * 2. The data gradient, s = 2 only
 *
 *     dx[n][ci][2 y][2 x] = sum over co of  w[co][ci] * dy[n][co][y][x],     dx = 0 at every other position
 *
 * The lane that holds the value of output pixel (y, x) writes the 2 x 2 cell of dx at (2 y, 2 x), cut at H and W: every
 * element of dx[B, Cin, H, W] is stored exactly once, no zero-fill pass, no workspace.
 *
 * Conventions (as include/scsfm_wrw.h)
 *  - All pointers are DEVICE pointers to contiguous NCHW fp32 arrays (4-byte aligned); the caller owns every buffer;
 *    nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_ERR_ARG (-1) for a rejected argument (nothing is launched then), otherwise the
 *    hipError_t of the failed launch.  Outputs are stored (overwritten), never accumulated.
 *  - Coverage (scsfm_pw_covers): Cin in {64, 128, 256, 512}, Cout in {128, 256, 512}, stride 1 or 2 (the data gradient:
 *    2), any B, H, W >= 1 for which every index fits a non-negative int.
 */
#ifndef SCSFM_PW_H_
#define SCSFM_PW_H_

#include <stddef.h>

#ifndef SCSFM_ERR_ARG
#define SCSFM_ERR_ARG (-1)
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* 1 (first version) */
int scsfm_pw_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: pw_source_id) into buf, NUL-terminated */
int scsfm_pw_source_id(char* buf, size_t n);
/* 1 when scsfm_pw_wrw_f32 takes these channel counts and this stride (scsfm_pw_dgrad_f32: with stride 2), else 0 */
int scsfm_pw_covers(int Cin, int Cout, int stride);
/* bytes of `ws` for one scsfm_pw_wrw_f32 call at this shape; 0 for a shape the call rejects */
size_t scsfm_pw_wrw_ws_bytes(int B, int Cin, int Cout, int H, int W, int stride);
/* dw[Cout, Cin] from x[B, Cin, H, W] and dy[B, Cout, Ho, Wo]; ws: at least scsfm_pw_wrw_ws_bytes(...) bytes */
int scsfm_pw_wrw_f32(int B, int Cin, int Cout, int H, int W, int stride, const float* x, const float* dy, float* dw,
                     void* ws, size_t ws_bytes, void* stream);
/* dx[B, Cin, H, W] of the stride-2 convolution from dy[B, Cout, Ho, Wo] and w[Cout, Cin] */
int scsfm_pw_dgrad_f32(int B, int Cin, int Cout, int H, int W, const float* dy, const float* w, float* dx,
                       void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_PW_H_ */
