/*
 * scsfm_dvis.h -- C ABI of libscsfm_dvis.so: the per-pixel work of eval_depth.py --vis_dir as hand-written HIP kernels
 * for gfx950 (MI355X): the median-scaled prediction at the ground truth's size, the colour range of a depth map
 * (minimum and exact 95th percentile of the inverse depth) and the `magma` picture of a map in a given range -- what the
 * reference's evaluate_depth returns and its depth_visualizer / depth_pair_visualizer draw with numpy 2 and
 * matplotlib 3.10, bit for bit and byte for byte.
 *
 * Conventions (as include/scsfm_vis.h and include/scsfm_eval.h)
 *  - All pointers are DEVICE pointers; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_DVIS_ERR_ARG (-1) for a rejected argument (before any pointer is touched),
 *    otherwise the hipError_t of the failed launch.  Every output is stored (overwritten), never accumulated.
 *  - Ragged maps: image i of a set is H_i x W_i elements, row-major, at element offset off[i] of one buffer
 *    (off: long long [N], gh / gw: int [N], on the device).  The callers keep the offsets multiples of 4 elements as for
 *    libscsfm_eval.so; these kernels load one element per lane and accept any offset.  max_hw >= every H_i * W_i.
 *  - `*_f64` flags (0 or 1) select float or double; T below is the map's type.
 *  - No float atomics.  Order statistics are selected on order-preserving integer keys (LDS integer histograms), so
 *    they are exact, deterministic and independent of how a set is chunked into calls: an image's result depends on
 *    that image's data alone.
 *  - Every `/` is the correctly rounded IEEE division of the stated precision; contraction is off.
 *  - The colour table's index is clamped to [0, 255] whatever a pixel holds, so no value gives a wild access.
 *  - inv(x) below is T(1) / (x + T(1e-6)).
 */
#ifndef SCSFM_DVIS_H_
#define SCSFM_DVIS_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCSFM_DVIS_ERR_ARG (-1)

/* 1 (first version) */
int scsfm_dvis_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: dvis_source_id) into buf, NUL-terminated */
int scsfm_dvis_source_id(char* buf, size_t n);

/* ---- (a) the scaled prediction at the ground truth's size ----
   pred  P [N, h, w] (P = double when pred_f64, else float)
   ratio R [N]       (R = double when out_f64, else float; out_f64 = 0 needs pred_f64 = 0: R is numpy's promotion of
                      the GT's type and P, never narrower than P)
   out   R ragged: image i is gh[i] x gw[i] at out + off[i].  Per output pixel of image i, in P:
       inv   = inv(pred_i)                                      at the four neighbours
       r     = OpenCV INTER_LINEAR's generic path at (gw[i], gh[i]): source coordinate (d + 0.5) * scale - 0.5 with
               scale = 1 / (dst / src) in double, rounded to float and floored; below 0 -> index 0, weight 0; at or
               past src - 1 -> the last index, weight 0; float weights; rows first, then the two rows
               (include/scsfm_eval.h, tests/depth_eval_oracle.py: resize_linear)
       depth = P(1) / (r + P(1e-6))
       out   = R(depth) * ratio[i]                              one rounding in R
   which is the reference's `pred_depth * ratio` of evaluate_depth.  A NaN ratio (an empty mask) gives a NaN map. */
int scsfm_dvis_scaled_depth(int N, int h, int w, int pred_f64, const void* pred, int out_f64, const void* ratio,
                            const long long* off, const int* gh, const int* gw, int max_hw, void* out, void* stream);

/* bytes of workspace scsfm_dvis_range needs for a ragged buffer of `total` elements (the last image's offset plus its
   size): the inverse depths, stored once.  0 for total == 0 or total >= 2^40. */
size_t scsfm_dvis_range_workspace_bytes(size_t total, int f64);

/* ---- (b) the colour range of every map ----
   maps  T ragged (off, gh, gw as above), `total` elements in all
   lo, hi int [N], t T [N]: the percentile's two order statistics and its weight, which depend on n = H_i * W_i and T
       only and are formed on the host with numpy scalars of type T, as numpy 2.2's np.percentile(., 95) forms them:
       q = T(95) / T(100); vi = T(n - 1) * q; lo = floor(vi); hi = min(lo + 1, n - 1); t = vi - T(lo)
       0 <= lo <= hi < n is the caller's duty; an index outside [0, n) is clamped into it.
   range double [N, 2]: (vmin, vmax), each the exact widening of a T value:
       vmin = min(inv(x))                                       (-0 orders below +0)
       a = sorted(inv)[lo], b = sorted(inv)[hi], d = b - a
       vmax = t < 0.5 ? a + d * t : b - d * (T(1) - t)          in T
   A NaN anywhere in inv(map) makes both NaN.  One workgroup per image: the inverse depths are stored in the workspace
   while their minimum is folded on integer keys; a radix select (11-bit digits, most significant first) finds the
   lo-th key, and the next key above it when hi is not among its duplicates. */
int scsfm_dvis_range(int N, int f64, const void* maps, const long long* off, const int* gh, const int* gw,
                     size_t total, const int* lo, const int* hi, const void* t, void* workspace,
                     size_t workspace_bytes, double* range, void* stream);

/* ---- (c) the picture of every map ----
   maps  T ragged (off, gh, gw as above)
   range double [N, 2]: (vmin, vmax) of image i, possibly another map's (the ground truth's range colours the
         prediction on NYU)
   table uint8 [256, 3]: entry k is uint8(float64(lut[k]) * 255) of matplotlib's magma
   out   uint8: pixel (y, x) of image i is three bytes at out + out_off[i] + y * out_pitch[i] + 3 * x  (bytes), so a
         picture can be written straight into its panel of a wider canvas.  Per pixel:
       v  = 0                                                   when vmin == vmax, otherwise
       v  = T(double(inv(x)) - vmin);  v = T(double(v) / (vmax - vmin))
       xa = v * T(256)
       xa is NaN -> (0, 0, 0);  xa < 0 -> table[0];  xa >= 256 (xa == 256 and +inf included) -> table[255];
       otherwise table[(int) xa]
   which is matplotlib 3.10's Normalize (in-place -= and /= with float64 scalars under numpy 2) and
   Colormap.__call__ with magma's under / over / bad colours, then (rgb * 255).astype(uint8).  A NaN in the range
   blacks the whole picture.  matplotlib raises for vmin > vmax; here the same two steps are taken. */
int scsfm_dvis_colourise(int N, int f64, const void* maps, const long long* off, const int* gh, const int* gw,
                         int max_hw, const double* range, const unsigned char* table, unsigned char* out,
                         const long long* out_off, const int* out_pitch, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_DVIS_H_ */
