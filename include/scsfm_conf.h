/*
 * scsfm_conf.h -- C ABI of libscsfm_conf.so: the depth consistency of a frame with its neighbours as a per-pixel
 * confidence (one minus the training loss's depth inconsistency, the self-discovered mask), and the TSDF integration
 * that weighs every observation by it, as hand-written HIP kernels for gfx950 (MI355X).
 *
 * Conventions (as include/scsfm_fuse.h)
 *  - All pointers are DEVICE pointers; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_CONF_ERR_ARG (-1) for a rejected argument (before any pointer is touched),
 *    otherwise the hipError_t of the failed launch.  Every output is stored (overwritten), never accumulated.
 *  - No float atomics: a pixel and a voxel belong to one thread, so results are bit-identical from run to run.
 *  - Sizes whose products would overflow int are rejected.  float pointers must be aligned to 4 bytes, c2w to 8.
 *
 * Arithmetic.  fp32 unless stated, one rounding per operation (no fused multiply-add), `/` correctly rounded,
 * denormals kept.  fl() marks a rounding where the nesting alone might not show it.
 *
 * Pair record (16 floats): R row-major (r0 .. r8), t (t0 t1 t2), fx, fy, cx, cy -- the camera of frame i to the camera
 * of its neighbour j, and the intrinsics the two share.  An absent neighbour is sixteen zeros; a record counts as
 * present when its fx > 0 and its j lies inside 0 .. n - 1.
 *
 * Pairs.  Slot s = 0 .. 2 radius - 1 of frame i is frame j = i + o, o running over -radius .. -1, 1 .. radius in that
 * order.  With (A_i, a_i) and (A_j, a_j) the 3 x 3 and the translation of c2w_i and c2w_j, in double:
 *   Z = A_j^-1, the GENERAL inverse exactly as include/scsfm_fuse.h's scsfm_fuse_cameras forms it (adjugate / determinant
 *   with det = (a00 C00 + a01 C01) + a02 C02), and z = -(Z a_j) with each dot product summed left to right;
 *   R[r][c] = (Z[r][0] A_i[0][c] + Z[r][1] A_i[1][c]) + Z[r][2] A_i[2][c],
 *   t[r]    = ((Z[r][0] a_i[0] + Z[r][1] a_i[1]) + Z[r][2] a_i[2]) + z[r],
 * each rounded once to fp32; fx = K[0], fy = K[4], cx = K[2], cy = K[5].  A slot whose j is outside 0 .. n - 1 is
 * sixteen zeros.
 *
 * Weights.  For pixel (px, py) of frame i (the centre of pixel px is at u = px, as step 3 of the integration implies):
 *   1. d = depth[i, py, px]; with is_disp, d = 1.0f / depth[i, py, px].  Unless d > 0 && d <= max_depth (a NaN fails) the
 *      weight is 0.
 *   2. count = 0, sum = 0.0f, best = 0.0f.  For the slots s = 0 .. 2 radius - 1 in that order, skipping the absent ones,
 *      with the slot's record (r, t, fx, fy, cx, cy) and j its frame:
 *      a. X = fl(fl(fl(float(px) - cx) / fx) d),  Y = fl(fl(fl(float(py) - cy) / fy) d),  Z = d.
 *      b. q_x = ((r0 X + r1 Y) + r2 Z) + t0,  q_y = ((r3 X + r4 Y) + r5 Z) + t1,  q_z = ((r6 X + r7 Y) + r8 Z) + t2.
 *         The neighbour is skipped unless q_z > 0.
 *      c. u = fl(fl(fx q_x) / q_z) + cx,  v = fl(fl(fy q_y) / q_z) + cy.
 *      d. g = floor(u), h = floor(v) (the true floor: -0.3 gives -1).  Skipped unless g >= 0 && g < float(W) &&
 *         h >= 0 && h < float(H) (a NaN fails); x0 = int(g), y0 = int(h); skipped unless x0 <= W - 2 && y0 <= H - 2.
 *      e. d00 = depth[j, y0, x0], d01 = depth[j, y0, x0 + 1], d10 = depth[j, y0 + 1, x0], d11 = depth[j, y0 + 1, x0 + 1];
 *         with is_disp each is inverted first (1.0f / tap).  Skipped unless all four are > 0 (a NaN fails).
 *      f. a = u - g, b = v - h;  top = d00 + fl(a fl(d01 - d00)),  bot = d10 + fl(a fl(d11 - d10)),
 *         p = top + fl(b fl(bot - top)).
 *      g. m = 1.0f - fl(fabs(q_z - p) / fl(q_z + p)).
 *      h. count += 1;  sum = sum + m;  best = m > best ? m : best (a NaN is never taken).
 *   3. c = count >= min_views ? (reduce == 0 ? sum / float(count) : best) : 0.0f;  c = c >= floor ? c : 0.0f (a NaN
 *      becomes 0);  weight[i, py, px] = c.  So 0 <= c <= 1 always.
 * One launch covers all frames; a pixel's depth is read once and its weight written once; the frame's records sit in
 * LDS.  Where W is a multiple of 4 and depth and weight are aligned to 16 bytes a thread takes four pixels in x.
 *
 * Integration.  The volume, the camera records (world to camera, what scsfm_fuse_cameras writes) and the steps are
 * those of include/scsfm_fuse.h, restated here in full.  nx x ny x nz voxels, x fastest, nvox <= 2^29, five fp32 planes
 * (tsdf, weight, r, g, b); the centre of voxel i on an axis with origin o and voxel size s is
 * fl(o + fl(fl(float(i) + 0.5f) s)).  For every voxel with centre (x, y, z), for the frames f = 0 .. F-1 in that order:
 *   1. q_x = ((r0 x + r1 y) + r2 z) + t0,  q_y = ((r3 x + r4 y) + r5 z) + t1,  q_z = ((r6 x + r7 y) + r8 z) + t2.
 *      The frame is skipped unless q_z > near.
 *   2. u = fl(fl(fx q_x) / q_z) + cx,  v = fl(fl(fy q_y) / q_z) + cy.
 *   3. a = fl(u + 0.5f), b = fl(v + 0.5f); skipped unless a >= 0 && a < float(W) && b >= 0 && b < float(H) (a NaN fails);
 *      px = int(a), py = int(b).
 *   4. d = depth[f, py, px]; with is_disp, d = 1.0f / depth[f, py, px].  Skipped unless d > 0 && d <= max_depth.
 *   4c. c = weight[f, py, px].  Skipped unless c > 0 && c <= 1 (a NaN fails).
 *   5. sdf = d - q_z.  Skipped if sdf < -trunc.
 *   6. tn = min(1.0f, sdf / trunc).
 *   7. tsdf <- (tsdf w + fl(tn c)) / (w + c)                      (w: the voxel's weight before this frame)
 *   8. with an image, per channel: col = fl(image[f, ch, py, px] 0.225f) + 0.45f,
 *      colour <- (colour w + fl(col c)) / (w + c).  Without an image the colour planes are neither read nor written.
 *   9. w <- min(w + c, max_weight).
 * tn 1.0f and w + 1.0f are what scsfm_fuse_integrate computes, so a weight of all ones leaves its bits.  The frames of a
 * call are applied in registers (up to 32 per launch), so one call with F frames leaves the bits of F calls with one
 * frame each; a workgroup's tile of voxels (32 x 8 x 4) skips the frames whose frustum and [near, max_depth + trunc] it
 * cannot meet, a conservative test that changes no bit.
 */
#ifndef SCSFM_CONF_H_
#define SCSFM_CONF_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCSFM_CONF_ERR_ARG (-1)
#define SCSFM_CONF_MAX_RADIUS 4
#define SCSFM_CONF_MAX_VOXELS (1 << 29)
#define SCSFM_CONF_REC 16        /* floats per pair record and per camera record */
#define SCSFM_CONF_MEAN 0        /* reduce: the mean over the neighbours that count */
#define SCSFM_CONF_MAX 1         /* reduce: the best neighbour */

/* 1 (first version) */
int scsfm_conf_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: conf_source_id) into buf, NUL-terminated */
int scsfm_conf_source_id(char* buf, size_t n);

/* c2w [n, 12] doubles (camera to world), K [9] floats -> pair [n, 2 radius, 16] (see Pairs).  One lane per (frame,
   slot).  Rejected: n <= 0, radius outside 1 .. SCSFM_CONF_MAX_RADIUS, n 2 radius 16 past int, a NULL or misaligned
   pointer. */
int scsfm_conf_pairs(int n, int radius, const double* c2w, const float* K, float* pair, void* stream);

/* depth [n, H, W], pair [n, 2 radius, 16] -> weight [n, H, W] (see Weights).  Rejected: a size <= 0, n H W or
   n 2 radius 16 past int, radius outside 1 .. SCSFM_CONF_MAX_RADIUS, max_depth <= 0, min_views < 1, floor outside 0 .. 1
   (or a NaN or infinite scalar), reduce other than 0 and 1, a NULL or misaligned pointer. */
int scsfm_conf_weights(int n, int radius, int H, int W, const float* depth, int is_disp, const float* pair,
                       float max_depth, int min_views, float floor, int reduce, float* weight, void* stream);

/* Integrates F frames, each observation weighed by weight [F, H, W] (see Integration).  depth [F, H, W]; image
   [F, 3, H, W] or NULL; volume: the five planes.  Rejected: what scsfm_fuse_integrate rejects (a size <= 0, nvox >
   2^29, F <= 0, F 3 H W past int, voxel <= 0, trunc <= 0, near < 0, max_depth <= 0, max_weight < 1, or any of them NaN
   or infinite, a NULL cam, depth or volume, a misaligned pointer) and a NULL weight. */
int scsfm_conf_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, float trunc, float near_z,
                         float max_depth, float max_weight, int F, int H, int W, const float* cam, const float* depth,
                         const float* weight, int is_disp, const float* image, float* volume, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_CONF_H_ */
