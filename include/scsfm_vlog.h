/*
 * scsfm_vlog.h -- C ABI of libscsfm_vlog.so: the validation pictures of train.py --log-output as hand-written HIP
 * kernels for gfx950 (MI355X): the float arrays that utils.tensor2array of the reference returns (the de-normalised
 * input, a map looked up in a colour table with matplotlib's under / over / bad rules), the same pictures as bytes,
 * the per-image maximum that divides a map and the target-disparity picture of a ground-truth depth.
 *
 * Conventions (as include/scsfm_vis.h)
 *  - All pointers are DEVICE pointers; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_VLOG_ERR_ARG (-1) for a rejected argument (before any pointer is touched),
 *    otherwise the hipError_t of the failed launch.  Every output is stored (overwritten), never accumulated.
 *  - No float atomics.  The maximum is formed from order-preserving 32-bit integer keys (wave shuffles, then one integer
 *    atomicMax per block), so it is exact and does not depend on the order of arrival.
 *  - Every division is IEEE float32 `/`, correctly rounded; no multiply and add are contracted into one operation.
 *  - A colour table lives on the device and cannot be checked by the return value; the index into it is clamped to
 *    [0, table_n - 1] whatever the pixel holds, so no value of a map gives a wild access.
 *  - The byte of a float v, wherever a picture is also written as bytes:
 *        byte = (uint8) min(max(255.0f * v, 0), 255)          (truncation toward zero; a NaN gives 0)
 */
#ifndef SCSFM_VLOG_H_
#define SCSFM_VLOG_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCSFM_VLOG_ERR_ARG (-1)

/* 1 (first version) */
int scsfm_vlog_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: vlog_source_id) into buf, NUL-terminated */
int scsfm_vlog_source_id(char* buf, size_t n);

/* ---- (a) the input picture ----
   in float [N, 3, H, W] (the normalised batch)  ->  v = 0.45f + x * 0.225f: the multiply is rounded, then the add (a
   fused multiply-add gives other bits), which is 0.45 + tensor.numpy() * 0.225 on a float32 array.
   out_f  float [N, 3, H, W] (planar), or NULL
   out_u8 uint8 [N, H, W, 3] (interleaved RGB, the byte rule above), or NULL
   At least one output.  N * H * W < 2^29. */
int scsfm_vlog_input_picture(int N, int H, int W, const float* in, float* out_f, unsigned char* out_u8, void* stream);

/* ---- (b) the target disparity of a ground-truth depth ----
   in float [N, HW] -> out float [N, HW]:
       d'  = (d == 0 ? 1000 : d)                                   (-0 is 0)
       out = min(max(1.0f / d', 0), 10)                            (a NaN stays a NaN, as torch.clamp leaves it)
   `in` is not written. */
int scsfm_vlog_target_disparity(int N, int HW, const float* in, float* out, void* stream);

/* ---- (c) the maximum of every image ----
   in float [N, HW] -> out float [N].  An image that holds a NaN gives NaN; -0 and +0 compare equal and either may be
   returned.  Three steps on the stream: clear `out`, collect the keys into it (integer atomicMax), decode it in place;
   no workspace. */
int scsfm_vlog_image_max(int N, int HW, const float* in, float* out, void* stream);

/* ---- (d) a map as a picture ----
   in    float [N, H, W]
   table float [table_n, 4] (RGBA), 16-byte aligned: entry i is read as one 16-byte word
   divisors float [N] on the device, or NULL: then every image is divided by the host value max_value (converted to
   float32 first).  Per pixel x of image n, all in float32:
       xa = (x / d_n) * (float) table_n
       xa is NaN                      -> (0, 0, 0, 0)
       xa < 0                         -> table[0]
       xa >= table_n                  -> table[table_n - 1]            (xa == table_n included; +inf too)
       otherwise                      -> table[(int) xa]               (truncation toward zero)
   This is matplotlib's Colormap.__call__ on a float32 array with the under colour table[0], the over colour
   table[table_n - 1] and the bad colour (0, 0, 0, 0), followed by .astype(float32), when the table holds
   float32(float64 lut).  A NaN divisor (an image that holds a NaN) or 0 / 0 blanks the picture.
   out_f  float [N, 4, H, W] (planar: what tensor2array returns), or NULL
   out_u8 uint8 [N, H, W, 4] (interleaved RGBA, the byte rule above), 4-byte aligned, or NULL
   At least one output.  N * H * W < 2^29. */
int scsfm_vlog_map_picture(int N, int H, int W, const float* in, const float* table, int table_n,
                           const float* divisors, double max_value, float* out_f, unsigned char* out_u8, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_VLOG_H_ */
