/*
 * scsfm_decb.h -- C ABI of libscsfm_decb.so: the depth decoder's fused glue of include/scsfm_nets.h with the bias of the
 * convolution in front of it folded in, as hand-written HIP kernels for gfx950 (MI355X).  The convolution is called
 * without its bias; the forward adds bias[c] to its output before the ELU (or the sigmoid of a disparity head), where
 * ATen runs a broadcast add over the whole tensor, and the backward sums the gradient it stores per channel, where ATen
 * runs grad_output.sum((0, 2, 3)) over the whole tensor again.  Both ride on passes that touch every element anyway.
 *
 * Conventions (as include/scsfm_nets.h)
 *  - All pointers are DEVICE pointers to contiguous NCHW fp32 arrays (ws: 8-byte aligned); the caller owns every buffer;
 *    nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_ERR_ARG (-1) for a rejected argument (nothing is written then), otherwise the
 *    hipError_t of the failed launch.  Every output is stored (overwritten), never accumulated.
 *  - R, E, U and the backward's fold order, child order and ELU-gradient form g * (r + 1) are those of
 *    include/scsfm_nets.h: g_x, g_a and g_skip are bit for bit what scsfm_nets_pad_bwd_f32(elu = 1) and
 *    scsfm_nets_up_cat_pad_bwd_f32 store for the same gp and out.
 *  - Bias gradient: g_bias[c] = the sum over b, y, x of the gradient the call stores for channel c (g_x, g_a).  Every
 *    stored value is added in fp64 in a fixed order: a lane adds its (up to) four values, the wave adds its lanes by a
 *    fixed tree and leaves one fp64 partial per wave segment in `ws`, and a second launch with one workgroup per channel
 *    adds the channel's partials in a fixed order and rounds once to fp32.  No floating-point atomics: the same input
 *    gives the same bits, call after call.  `ws` holds scsfm_decb_ws_bytes(B, C, H, W) bytes for a summed gradient of
 *    shape [B, C, H, W] (8 * B * C * H * ceil(W / 256)); the head's is [B, C, 1, H * W].  With g_bias NULL the sum is
 *    skipped, `ws` may be NULL and is left untouched.
 */
#ifndef SCSFM_DECB_H_
#define SCSFM_DECB_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 (first version) */
int scsfm_decb_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: decb_source_id) into buf, NUL-terminated */
int scsfm_decb_source_id(char* buf, size_t n);
/* bytes of `ws` for a bias sum over a stored gradient of shape [B, C, H, W]; 0 for a non-positive size */
size_t scsfm_decb_ws_bytes(int B, int C, int H, int W);

/* out[B,C,H+2,W+2] = R(E(x + bias[c])), x[B,C,H,W], bias[C]; H, W >= 2 */
int scsfm_decb_bias_elu_pad_fwd_f32(int B, int C, int H, int W, const float* x, const float* bias, float* out,
                                    void* stream);
/* g_x[B,C,H,W] from gp[B,C,H+2,W+2] and out (the forward's output), as scsfm_nets_pad_bwd_f32(elu = 1);
   g_bias[C] = sum of g_x over b, y, x (NULL: no sum) */
int scsfm_decb_bias_elu_pad_bwd_f32(int B, int C, int H, int W, const float* gp, const float* out, float* g_x, void* ws,
                                    float* g_bias, void* stream);

/* out[B,Ca+Cs,2H+2,2W+2] = R(cat[U(E(a + bias[c])), skip]), a[B,Ca,H,W], bias[Ca], skip[B,Cs,2H,2W] (Cs = 0: NULL) */
int scsfm_decb_bias_up_cat_pad_fwd_f32(int B, int Ca, int Cs, int H, int W, const float* a, const float* bias,
                                       const float* skip, float* out, void* stream);
/* g_a[B,Ca,H,W] and g_skip[B,Cs,2H,2W] as scsfm_nets_up_cat_pad_bwd_f32; g_bias[Ca] = sum of g_a over b, y, x (NULL: no
   sum; ws: scsfm_decb_ws_bytes(B, Ca, H, W)) */
int scsfm_decb_bias_up_cat_pad_bwd_f32(int B, int Ca, int Cs, int H, int W, const float* gp, const float* out,
                                       float* g_a, float* g_skip, void* ws, float* g_bias, void* stream);

/* y[B,C,H,W] = 1 / (1 + expf(-(x + bias[c]))), out = alpha * y + beta: each step one fp32 operation, in the order of
   ATen's chain conv + bias -> sigmoid -> mul -> add */
int scsfm_decb_disp_head_fwd_f32(int B, int C, int H, int W, const float* x, const float* bias, float alpha, float beta,
                                 float* y, float* out, void* stream);
/* g_x = ((g_out * alpha) * (1 - y)) * y (ATen's mul backward, then sigmoid_backward); g_bias[C] = sum of g_x over
   b, y, x (NULL: no sum; ws: scsfm_decb_ws_bytes(B, C, 1, H * W)) */
int scsfm_decb_disp_head_bwd_f32(int B, int C, int H, int W, float alpha, const float* g_out, const float* y,
                                 float* g_x, void* ws, float* g_bias, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_DECB_H_ */
