/*
 * scsfm_fuse.h -- C ABI of libscsfm_fuse.so: dense voxel reconstruction from the predicted depth and poses (TSDF fusion
 * and the extraction of surface points) as hand-written HIP kernels for gfx950 (MI355X).
 *
 * Conventions (as include/scsfm_odom.h)
 *  - All pointers are DEVICE pointers; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_FUSE_ERR_ARG (-1) for a rejected argument (before any pointer is touched),
 *    otherwise the hipError_t of the failed launch.  Every output is stored (overwritten), never accumulated.
 *  - No float atomics: a voxel belongs to one thread, and the extracted points are placed by an integer scan, so
 *    results are bit-identical from run to run.
 *  - Sizes whose products would overflow int are rejected.
 *
 * Volume.  nx x ny x nz voxels, x fastest (voxel (x, y, z) has the linear index (z ny + y) nx + x), any positive sizes
 * with nvox = nx ny nz <= 2^29.  Five fp32 planes of nvox each, one after another: tsdf, weight, r, g, b.  An all-zero
 * buffer is the empty volume: weight 0 is "never seen", and (t 0 + t') / 1 ignores the old value.  The centre of voxel
 * i on an axis with origin o and voxel size s is  fl(o + fl(fl(float(i) + 0.5f) s)).
 *
 * Arithmetic.  fp32 unless stated, one rounding per operation (no fused multiply-add), `/` correctly rounded,
 * denormals kept.  fl() marks a rounding where the nesting alone might not show it.
 *
 * Camera record (16 floats per frame): R row-major (r0 .. r8), t (t0 t1 t2), fx, fy, cx, cy -- world to camera.
 *
 * Integration.  For every voxel with centre (x, y, z), for the frames f = 0 .. F-1 in that order:
 *   1. q_x = ((r0 x + r1 y) + r2 z) + t0,  q_y = ((r3 x + r4 y) + r5 z) + t1,  q_z = ((r6 x + r7 y) + r8 z) + t2.
 *      The frame is skipped unless q_z > near.
 *   2. u = fl(fl(fx q_x) / q_z) + cx,  v = fl(fl(fy q_y) / q_z) + cy.
 *   3. a = fl(u + 0.5f), b = fl(v + 0.5f); skipped unless a >= 0 && a < float(W) && b >= 0 && b < float(H) (a NaN fails);
 *      px = int(a), py = int(b).
 *   4. d = depth[f, py, px]; with is_disp, d = 1.0f / depth[f, py, px].  Skipped unless d > 0 && d <= max_depth.
 *   5. sdf = d - q_z.  Skipped if sdf < -trunc.
 *   6. tn = min(1.0f, sdf / trunc).
 *   7. tsdf <- (tsdf w + tn) / (w + 1.0f)                         (w: the voxel's weight before this frame)
 *   8. with an image, per channel: c = fl(image[f, ch, py, px] 0.225f) + 0.45f (the image is the net's normalised
 *      input), colour <- (colour w + c) / (w + 1.0f).  Without an image the colour planes are neither read nor written.
 *   9. w <- min(w + 1.0f, max_weight).
 * The frames of a call are applied in registers: a voxel is read once and written once per launch, so one call with F
 * frames leaves the bits of F calls with one frame each.  A workgroup's tile of voxels (32 x 8 x 4) is tested, as a
 * sphere, against every frame's frustum and [near, max_depth + trunc]; the tile skips the frames it cannot meet and
 * neither loads nor stores when it meets none.  The test is conservative, so the result does not depend on it.
 *
 * Extraction.  The surface points are the sign changes of tsdf along the grid's edges, in a fixed order: by the linear
 * index of voxel a, then its +x, +y, +z edge.  The edge from a to its positive neighbour b (inside the volume) is a
 * crossing when  w_a >= min_weight && w_b >= min_weight && (t_a < 0) != (t_b < 0).  Then
 *   frac = t_a / fl(t_a - t_b)
 *   the coordinate along the edge's axis is fl(c_a + fl(frac voxel)), c_a a's centre; the other two are a's centre
 *   colour = fl(col_a + fl(frac fl(col_b - col_a))) per channel, c = colour >= 0 ? colour : 0 (a NaN becomes 0),
 *   c = c <= 1 ? c : 1, byte = uint8(fl(fl(c 255.0f) + 0.5f)).
 */
#ifndef SCSFM_FUSE_H_
#define SCSFM_FUSE_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCSFM_FUSE_ERR_ARG (-1)
#define SCSFM_FUSE_MAX_VOXELS (1 << 29)
#define SCSFM_FUSE_PLANES 5      /* tsdf, weight, r, g, b */
#define SCSFM_FUSE_CAM 16        /* floats per camera record */
#define SCSFM_FUSE_CHUNK 1024    /* consecutive voxels (by linear index) per extraction chunk */

/* 1 (first version) */
int scsfm_fuse_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: fuse_source_id) into buf, NUL-terminated */
int scsfm_fuse_source_id(char* buf, size_t n);

/* bytes of a volume of nx x ny x nz voxels (20 per voxel); 0 for a rejected argument (a size <= 0, nvox > 2^29) */
size_t scsfm_fuse_volume_bytes(int nx, int ny, int nz);

/* c2w [n, 12] doubles (what scsfm_odom_chain writes: camera to world), K [9] floats (row-major 3 x 3, shared by the
   frames) -> cam [n, 16].  World to camera is the GENERAL inverse of (A, t) in double, exactly as include/scsfm_odom.h
   defines it (adjugate / determinant with det = (a00 C00 + a01 C01) + a02 C02, then -(A^-1 t) with each dot product
   summed left to right), rounded once to fp32; fx = K[0], fy = K[4], cx = K[2], cy = K[5]. */
int scsfm_fuse_cameras(int n, const double* c2w, const float* K, float* cam, void* stream);

/* Integrates F frames (see above).  depth [F, H, W]; image [F, 3, H, W] or NULL; volume: the five planes.
   Rejected: a size <= 0, nvox > 2^29, F <= 0, F 3 H W past int, voxel <= 0, trunc <= 0, near < 0, max_depth <= 0,
   max_weight < 1 (or any of them NaN or infinite), a NULL cam, depth or volume, a volume not aligned to 4 bytes. */
int scsfm_fuse_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, float trunc, float near_z,
                         float max_depth, float max_weight, int F, int H, int W, const float* cam, const float* depth,
                         int is_disp, const float* image, float* volume, void* stream);

/* bytes of the workspace of scsfm_fuse_count and scsfm_fuse_extract; 0 for a rejected argument.  Its layout, in ints:
   [0] the number of crossings, [1 .. 3] unused, then the count of every chunk of SCSFM_FUSE_CHUNK voxels, then the
   exclusive scan of those counts. */
size_t scsfm_fuse_extract_ws_bytes(int nx, int ny, int nz);

/* Counts the crossings of every chunk, scans the counts and stores the total, all into ws (16-byte aligned,
   ws_bytes >= scsfm_fuse_extract_ws_bytes).  The host reads ws[0] once to size xyz and rgb.  min_weight >= 1. */
int scsfm_fuse_count(int nx, int ny, int nz, const float* volume, float min_weight, void* ws, size_t ws_bytes,
                     void* stream);

/* Writes the crossings in their order: point k < capacity to xyz[k, 3] and rgb[k, 3]; nothing at or past capacity.
   ws is what scsfm_fuse_count left for the same volume and min_weight.  capacity >= 0 (0: xyz and rgb may be NULL). */
int scsfm_fuse_extract(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, const float* volume,
                       float min_weight, const void* ws, size_t ws_bytes, int capacity, float* xyz, unsigned char* rgb,
                       void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_FUSE_H_ */
