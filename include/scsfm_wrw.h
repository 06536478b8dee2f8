/*
 * scsfm_wrw.h -- C ABI of libscsfm_wrw.so: the weight gradient of the depth decoder's low-channel 3x3 convolutions as a
 * hand-written HIP kernel for gfx950 (MI355X), on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32.
 *
 *     dW[co][ci][r][s] = sum over n, h, w of  dy[n][co][h][w] * x[n][ci][h + r][w + s]          r, s = 0..2
 *
 * for a 3x3, stride-1, dilation-1, padding-0 convolution.  x is the already reflection-padded input
 * [B, Cin, H + 2, W + 2] that the decoder's fused glue produces, dy the output gradient [B, Cout, H, W]; both are read
 * as they lie (NCHW), nothing is transposed and nothing is zero-filled.
 *
 * Conventions (as include/scsfm_nets.h)
 *  - All pointers are DEVICE pointers to contiguous NCHW fp32 arrays (ws: 4-byte aligned); the caller owns every buffer;
 *    nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_ERR_ARG (-1) for a rejected argument (nothing is written then), otherwise the
 *    hipError_t of the failed launch.  dW is stored (overwritten), never accumulated.
 *  - Coverage: Cout in {1, 16, 32}, Cin in {16, 32, 64, 96}, any B, H, W >= 1 (scsfm_wrw_conv3x3_covers); Cout = 1 (a
 *    disparity head) runs as one row of a 16-row block.
 *  - Order of summation: a grid whose size depends on the shape alone walks the 8 x 32 output tiles in a fixed order;
 *    every workgroup leaves one fp32 partial dW in `ws`, a second launch adds the partials of an entry in fp64 in a
 *    fixed order and rounds once.  No atomics: the same input gives the same bits, call after call.
 */
#ifndef SCSFM_WRW_H_
#define SCSFM_WRW_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 (first version) */
int scsfm_wrw_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: wrw_source_id) into buf, NUL-terminated */
int scsfm_wrw_source_id(char* buf, size_t n);
/* 1 when scsfm_wrw_conv3x3_f32 takes these channel counts, else 0 */
int scsfm_wrw_conv3x3_covers(int Cin, int Cout);
/* bytes of `ws` for one call at this shape; 0 for a shape the call rejects */
size_t scsfm_wrw_conv3x3_ws_bytes(int B, int Cin, int Cout, int H, int W);
/* dw[Cout,Cin,3,3] from x[B,Cin,H+2,W+2] and dy[B,Cout,H,W]; ws holds at least scsfm_wrw_conv3x3_ws_bytes(...) bytes */
int scsfm_wrw_conv3x3_f32(int B, int Cin, int Cout, int H, int W, const float* x, const float* dy, float* dw, void* ws,
                          size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_WRW_H_ */
