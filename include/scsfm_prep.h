/*
 * scsfm_prep.h -- C ABI of libscsfm_prep.so: the per-frame work of data/prepare_train_data.py as hand-written HIP
 * kernels for gfx950 (MI355X): Pillow's 8-bit bilinear resize, byte for byte, and the projection of Velodyne scans into
 * sparse depth maps as KittiRawLoader.generate_depth_map computes them.
 *
 * Conventions (as include/scsfm_snip.h)
 *  - All pointers are DEVICE pointers; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_PREP_ERR_ARG (-1) for a rejected argument (before any pointer is touched),
 *    otherwise the hipError_t of the failed launch.  Every output is stored (overwritten), never accumulated.
 *  - No float atomics.  The depth maps are resolved from values collected with 32-bit integer atomicMax / atomicAdd
 *    whose results do not depend on the order of arrival, so two runs give the same bits.
 *  - Tables that live on the device cannot be checked by the return value; an entry that points outside its array is
 *    not followed (the tap or the point is skipped), so a wrong table gives wrong numbers, never a wild access.
 */
#ifndef SCSFM_PREP_H_
#define SCSFM_PREP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCSFM_PREP_ERR_ARG (-1)

#define SCSFM_PREP_PRECISION_BITS 22 /* Pillow's fixed-point taps: 32 - 8 - 2 */

/* 1 (first version) */
int scsfm_prep_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: prep_source_id) into buf, NUL-terminated */
int scsfm_prep_source_id(char* buf, size_t n);

/* ---- (a) Pillow's Image.resize(..., BILINEAR) for 8 bits per channel ----
   in  uint8 [N, H, W, C], C in {1, 3, 4}: N frames of one size, channels interleaved and resampled independently.
   out uint8 [N, keep_rows, w, C]: the first keep_rows rows of the resized frames; the others are not computed.
   ImagingResample: a horizontal pass, then a vertical pass over its uint8 result; each output byte is
       clip8((2^21 + sum_i tap_i * pixel_i) >> 22)                                   (int32, arithmetic shift)
   An axis table is built on the host (scsfm_hip/prepare.py: axis_table).  `rows` holds three ints per output position
   (first source index, tap count, offset of its first tap in `taps`); `taps` holds n_taps 22-bit integers.
   A pass whose size does not change is skipped, not run with identity taps: hrows == NULL skips the horizontal pass
   (w must equal W), vrows == NULL skips the vertical pass (output row r is source row r; keep_rows <= H).  With both
   NULL the call is a copy of the kept rows.
   With both passes the horizontal pass resamples source rows [src_row0, src_row0 + src_rows) only -- the rows the
   kept output rows reach -- into the workspace, uint8 [N, src_rows, w, C]; otherwise src_row0 / src_rows are ignored
   and no workspace is needed (workspace may be NULL). */

/* bytes of workspace for the call (0 when it needs none); 0 also for rejected sizes */
size_t scsfm_prep_resize_workspace_bytes(int N, int C, int w, int src_rows, int both_passes);

int scsfm_prep_resize_u8(int N, int H, int W, int C, int keep_rows, int w, const unsigned char* in, const int* hrows,
                         const int* htaps, int n_htaps, const int* vrows, const int* vtaps, int n_vtaps, int src_row0,
                         int src_rows, unsigned char* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- (b) KittiRawLoader.generate_depth_map for F scans ----
   points   float [total, 4]: rows (forward, left, up, reflectance); the reflectance is read as 1
   scan_off int [F + 1]: scan f owns rows [scan_off[f], scan_off[f + 1]); scan_off[0] = 0, scan_off[F] = total
   P        double [F, 3, 4]: velodyne -> image, formed on the host (scsfm_hip/prepare.py: velo_projection)
   depth    float [F, h, w]
   bound_u, bound_v: the real bounds img_width / ratio, img_height / ratio; 0 < bound_u <= w, 0 < bound_v <= h.
   Per point i of a scan, in double with separate roundings, each sum left to right:
       q_r = ((P_r0 x + P_r1 y) + P_r2 z) + P_r3,   u = rint(q_0 / q_2) - 1,   v = rint(q_1 / q_2) - 1
   (rint: half to even).  The point is kept when float x >= 0, 0 <= u < bound_u and 0 <= v < bound_v; NaN fails.
     1. every kept point writes (float) q_2 to pixel (v, u); the point with the highest index wins;
     2. kept points are grouped by key = v (w - 1) + u - 1 (NOT the pixel index: column w - 1 of row r shares its key
        with column 0 of row r + 1); for every key held by more than one point, the pixel of the group's lowest-index
        point receives the minimum depth of the whole group;
     3. negative depths become 0.
   Three launches: clear (the workspace), collect (one lane per point: per pixel the highest index; per key the
   lowest index, the count and the minimum depth as an order-preserving uint32, all by atomicMax / atomicAdd on
   uint32), resolve (one lane per pixel, stores only). */

/* bytes of workspace; 0 for a rejected size (F, h or w < 1, or too large) */
size_t scsfm_prep_velo_workspace_bytes(int F, int h, int w);

int scsfm_prep_velo_depth(int F, int h, int w, double bound_u, double bound_v, const float* points, size_t total,
                          const int* scan_off, const double* P, float* depth, void* workspace, size_t workspace_bytes,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_PREP_H_ */
