/*
 * scsfm_nets.h -- C ABI of libscsfm_nets.so: fused glue of DispResNet's depth decoder as hand-written HIP kernels for
 * gfx950 (MI355X).  Each entry point replaces the ATen chain of reflection pad / ELU / 2x nearest upsampling / channel
 * concatenation between two of the decoder's 3x3 convolutions (models/DispResNet.py, DepthDecoder.forward), forward and
 * backward.  The convolutions themselves stay MIOpen's and see bit-identical inputs.
 *
 * Conventions (as include/scsfm_hip.h)
 *  - All pointers are DEVICE pointers to contiguous NCHW fp32 arrays; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_ERR_ARG (-1) for a rejected argument, otherwise the hipError_t of the failed
 *    launch.  Every output is stored (overwritten), never accumulated.
 *  - R(x): reflection pad by 1 (nn.ReflectionPad2d(1)); E(x): ELU with alpha 1 (x > 0 ? x : expm1f(x)); U(x): 2x
 *    nearest upsampling (F.interpolate(scale_factor=2, mode="nearest"): source index dst >> 1).  Every array has fewer
 *    than 2^31 elements.
 *  - Backward: `gp` is the gradient of the padded output.  The reflected border rows / columns fold onto rows and
 *    columns 1 and n-2 (two contributions each, four at the corners, summed in a fixed order); the four children of
 *    an upsampled element are summed row-major from (0,0), as ATen's upsample_nearest2d backward; the ELU gradient is
 *    ATen's result form, g * (r + 1) for r <= 0, with r read from the interior of the saved padded output.
 */
#ifndef SCSFM_NETS_H_
#define SCSFM_NETS_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 (first version) */
int scsfm_nets_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: nets_source_id) into buf, NUL-terminated */
int scsfm_nets_source_id(char* buf, size_t n);

/* out[B,C,H+2,W+2] = R(elu ? E(x) : x), x[B,C,H,W]; H, W >= 2 */
int scsfm_nets_pad_fwd_f32(int B, int C, int H, int W, int elu, const float* x, float* out, void* stream);
/* g_x[B,C,H,W] from gp[B,C,H+2,W+2]: the folded gradient, times the ELU gradient at r = out's interior when elu
   (out: the forward's output; unused, may be NULL, without elu) */
int scsfm_nets_pad_bwd_f32(int B, int C, int H, int W, int elu, const float* gp, const float* out, float* g_x,
                           void* stream);

/* out[B,Ca+Cs,2H+2,2W+2] = R(cat[U(E(a)), skip]), a[B,Ca,H,W], skip[B,Cs,2H,2W] (Cs = 0: no skip, skip NULL) */
int scsfm_nets_up_cat_pad_fwd_f32(int B, int Ca, int Cs, int H, int W, const float* a, const float* skip, float* out,
                                  void* stream);
/* g_a[B,Ca,H,W] and g_skip[B,Cs,2H,2W] from gp[B,Ca+Cs,2H+2,2W+2]; out: the forward's output */
int scsfm_nets_up_cat_pad_bwd_f32(int B, int Ca, int Cs, int H, int W, const float* gp, const float* out, float* g_a,
                                  float* g_skip, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_NETS_H_ */
