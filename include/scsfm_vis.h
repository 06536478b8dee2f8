/*
 * scsfm_vis.h -- C ABI of libscsfm_vis.so: the per-image work of run_inference.py as hand-written HIP kernels for
 * gfx950 (MI355X): the input normalisation, the per-image maximum of a disparity map and the colour-mapped pictures
 * that utils.tensor2array and matplotlib's Colormap.__call__ produce, byte for byte.
 *
 * Conventions (as include/scsfm_prep.h)
 *  - All pointers are DEVICE pointers; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_VIS_ERR_ARG (-1) for a rejected argument (before any pointer is touched),
 *    otherwise the hipError_t of the failed launch.  Every output is stored (overwritten), never accumulated.
 *  - No float atomics.  The maximum is formed from order-preserving 32-bit integer keys (wave shuffles, then one integer
 *    atomicMax per block), so it is exact and does not depend on the order of arrival.
 *  - Every division is IEEE float32 `/`, correctly rounded; nothing is replaced by a reciprocal multiply.
 *  - A colour table lives on the device and cannot be checked by the return value; the index into it is clamped to
 *    [0, table_n - 1] whatever the pixel holds, so no value of a map gives a wild access.
 */
#ifndef SCSFM_VIS_H_
#define SCSFM_VIS_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCSFM_VIS_ERR_ARG (-1)

/* 1 (first version) */
int scsfm_vis_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: vis_source_id) into buf, NUL-terminated */
int scsfm_vis_source_id(char* buf, size_t n);

/* ---- (a) the network's input ----
   in  uint8 [N, H, W, 3] (interleaved RGB)  ->  out float [N, 3, H, W]:
       out = ((float) x / 255.0f - 0.45f) / 0.225f                          (two roundings of `/`, one of `-`)
   which is the torch CPU expression (x / 255 - 0.45) / 0.225 on a float32 tensor, bit for bit. */
int scsfm_vis_normalise_u8(int N, int H, int W, const unsigned char* in, float* out, void* stream);

/* ---- (b) the maximum of every image ----
   in float [N, HW] -> out float [N].  An image that holds a NaN gives NaN; -0 and +0 compare equal and either may be
   returned.  Three steps on the stream: clear `out`, collect the keys into it (integer atomicMax), decode it in place;
   no workspace. */
int scsfm_vis_image_max(int N, int HW, const float* in, float* out, void* stream);

/* ---- (c) a map as a picture ----
   in    float [N, H, W]
   table uint8 [table_n, 4] (RGBA), 4-byte aligned: entry i is read and stored as one 32-bit word
   out   uint8 [N, H, W, 4]
   divisors float [N] on the device, or NULL: then every image is divided by the host value max_value (converted to
   float32 first).  Per pixel x of image n, all in float32:
       v  = reciprocal ? 1.0f / x : x
       xa = (v / d_n) * (float) table_n
       xa is NaN                      -> (0, 0, 0, 0)
       xa < 0                         -> table[0]
       xa >= table_n                  -> table[table_n - 1]            (xa == table_n included; +inf too)
       otherwise                      -> table[(int) xa]               (truncation toward zero)
   This is matplotlib's Colormap.__call__ on a float32 array with the under colour table[0], the over colour
   table[table_n - 1] and the bad colour (0, 0, 0, 0), followed by uint8(255 * float32(rgba)) when the table holds
   uint8(float32(255) * float32(lut)).  A NaN divisor (an image that holds a NaN) or 0 / 0 blanks the picture.
   Pixels are handled four per lane with 16-byte loads and stores where `in` and `out` are 16-byte aligned; the rest,
   or all of them otherwise, one per lane.  N * H * W < 2^29. */
int scsfm_vis_colourise(int N, int H, int W, const float* in, const unsigned char* table, int table_n,
                        const float* divisors, double max_value, int reciprocal, unsigned char* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_VIS_H_ */
