/*
 * scsfm_dgrad.h -- C ABI of libscsfm_dgrad.so: the backward of the depth decoder's full-resolution tail as one
 * hand-written HIP kernel for gfx950 (MI355X), and the data gradient of its low-channel 3x3 convolutions on the exact-fp32
 * matrix instruction v_mfma_f32_16x16x4_f32.
 *
 * 1. The tail.
 *
 * At level 0 the decoder computes  Q = R(E(b + bias)),  h = conv3x3(Q, w),  out = alpha * sigmoid(h + bias_h) + beta
 * (R: reflection pad by 1, E: ELU, w[1, C, 3, 3] the disparity head's weight) and Q has the head as its only consumer.
 * The backward of that tail is one streaming pass:
 *
 *     g[n][i][j]     = ((g_out * alpha) * (1 - y)) * y                        (y: the saved sigmoid; stored)
 *     gQ[n][c][p][q] = sum over r, s of  w[c][r][s] * g[n][p - r][q - s]      (over the padded grid, g = 0 outside the
 *                                                                              image; never stored)
 *     gE[n][c][i][j] = sum of gQ over the padded positions whose reflection source is (i, j)
 *     g_b[n][c][i][j] = E'(gE, E)  with  E = Q[n][c][i + 1][j + 1]  and  E'(g, r) = r <= 0 ? g * (r + 1) : g
 *     g_bias_b[c]    = sum over n, i, j of g_b[n][c][i][j]                    (where asked for)
 *     g_bias_head    = sum over n, i, j of g[n][i][j]                         (where asked for)
 *
 * 2. The data gradient of a 3x3, stride-1, dilation-1, padding-0 convolution with Cout = 16 and Cin = 16 or 32
 * (scsfm_dgrad_conv3x3_covers), any B, H, W >= 1:
 *
 *     dx[n][ci][p][q] = sum over co, r, s of  w[co][ci][r][s] * dy[n][co][p - r][q - s]
 *
 * with dx[B, Cin, H + 2, W + 2], dy[B, Cout, H, W] (zero outside) and w[Cout, Cin, 3, 3].  No workspace and no reduction
 * across workgroups: every element of dx is one k-ordered fp32 fma chain.
 *
 * Conventions (as include/scsfm_wrw.h)
 *  - All pointers are DEVICE pointers to contiguous NCHW fp32 arrays (ws: 8-byte aligned); the caller owns every
 *    buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_ERR_ARG (-1) for a rejected argument (nothing is written then), otherwise the
 *    hipError_t of the failed launch.  Outputs are stored (overwritten), never accumulated.
 *  - Coverage: C = 16, any B >= 1, H >= 2, W >= 2 (scsfm_dgrad_head_tail_covers).
 *  - Sums: a grid whose size depends on the shape alone; every workgroup leaves one fp64 partial per sum in `ws`, a
 *    second launch adds the partials of a sum in fp64 in a fixed order and rounds once.  No atomics: the same input
 *    gives the same bits, call after call.  With both g_bias_b and g_bias_head NULL neither `ws` nor the second launch
 *    is used.
 */
#ifndef SCSFM_DGRAD_H_
#define SCSFM_DGRAD_H_

#include <stddef.h>

#ifndef SCSFM_ERR_ARG
#define SCSFM_ERR_ARG (-1)
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* 1 (first version) */
int scsfm_dgrad_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: dgrad_source_id) into buf, NUL-terminated */
int scsfm_dgrad_source_id(char* buf, size_t n);
/* 1 when scsfm_dgrad_head_tail_bwd_f32 takes this channel count, else 0 */
int scsfm_dgrad_head_tail_covers(int C);
/* bytes of `ws` for one call at this shape; 0 for a shape the call rejects */
size_t scsfm_dgrad_head_tail_ws_bytes(int B, int C, int H, int W);
/* g[B,1,H,W] and g_b[B,C,H,W] from q[B,C,H+2,W+2], y[B,1,H,W] (NULL: g_out already is g), g_out[B,1,H,W] and
 * w[1,C,3,3]; g_bias_b[C] and g_bias_head[1] may each be NULL (that sum is then not stored); ws holds at least
 * scsfm_dgrad_head_tail_ws_bytes(...) bytes and may be NULL when both are */
int scsfm_dgrad_head_tail_bwd_f32(int B, int C, int H, int W, float alpha, const float* q, const float* y,
                                  const float* g_out, const float* w, float* g, float* g_b, void* ws, size_t ws_bytes,
                                  float* g_bias_b, float* g_bias_head, void* stream);

/* 1 when scsfm_dgrad_conv3x3_f32 takes these channel counts, else 0 */
int scsfm_dgrad_conv3x3_covers(int Cin, int Cout);
/* dx[B,Cin,H+2,W+2] from dy[B,Cout,H,W] and w[Cout,Cin,3,3] */
int scsfm_dgrad_conv3x3_f32(int B, int Cin, int Cout, int H, int W, const float* dy, const float* w, float* dx,
                            void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_DGRAD_H_ */
