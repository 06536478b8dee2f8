/*
 * scsfm_track.h -- C ABI of libscsfm_track.so: frame-to-model tracking.  A frame's depth map is aligned to the depth and
 * normal maps that libscsfm_cast.so cast from the fused volume (include/scsfm_cast.h) by point-to-plane ICP (iterative
 * closest point): a projective association per pixel, 29 double-precision sums per frame, a 6 x 6 solve and a pose update,
 * all on the device, as hand-written HIP kernels for gfx950 (MI355X).  The tracker takes the maps and never sees the
 * volume.
 *
 * Conventions (as include/scsfm_cast.h)
 *  - All pointers are DEVICE pointers; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_TRACK_ERR_ARG (-1) for a rejected argument (before any pointer is touched),
 *    otherwise the hipError_t of the failed launch.
 *  - No floating-point atomics: every sum has one stated order, so results are bit-identical from run to run.
 *  - Sizes whose products would overflow int are rejected.
 *
 * Arithmetic.  fp32 in the pair of a pixel, double in the sums, the solve and the state; one rounding per operation (no
 * fused multiply-add, in either precision), `/` and sqrt correctly rounded, denormals kept.  fl() marks a rounding where
 * the nesting alone might not show it; sums and differences of several terms are formed from left to right as the
 * parentheses show.  No library function (sin, cos, exp ...) is used anywhere: they do not give the same bits on every
 * machine.
 *
 * State (SCSFM_TRACK_STATE = 7 doubles per frame): a unit quaternion (w, x, y, z) and the camera centre (c0, c1, c2),
 * camera to world.
 *
 * The matrix of a quaternion, in double: with xx = x x, yy, zz, xy = x y, xz, yz, wx = w x, wy, wz,
 *     R00 = 1 - 2 (yy + zz)   R01 = 2 (xy - wz)       R02 = 2 (xz + wy)
 *     R10 = 2 (xy + wz)       R11 = 1 - 2 (xx + zz)   R12 = 2 (yz - wx)
 *     R20 = 2 (xz - wy)       R21 = 2 (yz + wx)       R22 = 1 - 2 (xx + yy)
 * scsfm_track_poses writes the rows (R_i0 R_i1 R_i2 c_i), 12 doubles a frame, as scsfm_odom_chain writes them.
 *
 * Pose record (16 floats per frame, scsfm_cast.h's view record): A row-major (a0 .. a8), the centre (c0 c1 c2), fx, fy,
 * cx, cy.  A is the matrix above and c the centre, each of the twelve doubles rounded once to fp32; fx = K[0], fy = K[4],
 * cx = K[2], cy = K[5] are written by scsfm_track_init and kept.  Whenever a state changes, the first twelve floats of
 * its record are rewritten on the device.
 *
 * scsfm_track_init: c2w [V, 12] doubles (rows m_i0 m_i1 m_i2 c_i) -> states and records.  Shepperd's branch, with
 * tr = (m00 + m11) + m22:
 *     tr >= m00, m11 and m22:      r = sqrt(1 + tr);                 w = r / 2; f = 0.5 / r;
 *                                  x = (m21 - m12) f; y = (m02 - m20) f; z = (m10 - m01) f
 *     else m00 >= m11 and m22:     r = sqrt(((1 + m00) - m11) - m22); x = r / 2; f = 0.5 / r;
 *                                  w = (m21 - m12) f; y = (m01 + m10) f; z = (m02 + m20) f
 *     else m11 >= m22:             r = sqrt(((1 + m11) - m00) - m22); y = r / 2; f = 0.5 / r;
 *                                  w = (m02 - m20) f; x = (m01 + m10) f; z = (m12 + m21) f
 *     else:                        r = sqrt(((1 + m22) - m00) - m11); z = r / 2; f = 0.5 / r;
 *                                  w = (m10 - m01) f; x = (m02 + m20) f; y = (m12 + m21) f
 * then NORMALISE: len = sqrt(((w w + x x) + y y) + z z), each component divided by len.  The centre is copied.
 *
 * The pair of pixel (px, py) of frame v, in fp32.  a_ij, c, fx .. cy are the frame's record (the estimate); r_ij, c',
 * fx' .. cy' the reference record ref[v]; M [V, H, W] and N [V, 3, H, W] the model's depth and world normals that
 * scsfm_cast_cast wrote for ref[v].
 *  1. d = depth[v, py, px], or 1.0f / depth[v, py, px] with is_disp.  The pixel is a CANDIDATE iff d > near &&
 *     d <= max_depth (a NaN fails).
 *  2. dx = fl((float(px) - cx) / fx), dy = fl((float(py) - cy) / fy): the cast's ray.  q = (fl(dx d), fl(dy d), d);
 *     u_i = (a_i0 q_0 + a_i1 q_1) + a_i2 q_2; p_i = c_i + u_i.  u is what "p - c" means below.
 *  3. e_i = p_i - c'_i; x' = (r_00 e_0 + r_10 e_1) + r_20 e_2, y' and z' with columns 1 and 2.  Require z' > near &&
 *     z' > 0.  a = fl(fl(fl(fx' x') / z') + cx') + 0.5f, b = fl(fl(fl(fy' y') / z') + cy') + 0.5f.  Require a >= 0 &&
 *     a < float(W) && b >= 0 && b < float(H), on the floats, before any conversion (the integration's pixel
 *     convention).  px' = int(a), py' = int(b).
 *  4. s = M[v, py', px']; require s > 0.  n_i = N[v, i, py', px']; require (n_0 n_0 + n_1 n_1) + n_2 n_2 > 0.  A NaN
 *     fails either test.
 *  5. dx' = fl((float(px') - cx') / fx'), dy' likewise; w_i = (r_i0 dx' + r_i1 dy') + r_i2; m_i = c'_i + fl(s w_i): the
 *     model's point, the cast's arithmetic.
 *  6. delta_i = p_i - m_i.  Require (delta_0 delta_0 + delta_1 delta_1) + delta_2 delta_2 <= fl(max_dist max_dist), and
 *     (n_0 u_0 + n_1 u_1) + n_2 u_2 < 0: the model's surface faces the estimate's camera.  A NaN fails either test.
 *  7. r = (n_0 delta_0 + n_1 delta_1) + n_2 delta_2.  J = (n_0, n_1, n_2, fl(u_1 n_2) - fl(u_2 n_1),
 *     fl(u_2 n_0) - fl(u_0 n_2), fl(u_0 n_1) - fl(u_1 n_0)): the twist (t, w) about the estimate's own centre,
 *     p -> c + t + (I + [w]x)(p - c).
 *  8. J and r are converted to double.  The pixel's 29 TERMS are the 21 products J_i J_j (i <= j; (0,0) (0,1) .. (0,5)
 *     (1,1) .. (5,5)), the 6 products J_i r, then r r, then 1.  A product of two fp32 values is exact in double.  A pixel
 *     that is no pair has 29 terms of +0.0.
 *
 * The sums (SCSFM_TRACK_SUMS = 29 doubles per frame), in double.  Pixels are numbered i = py W + px.  Workgroup g of a
 * frame (256 threads: 4 waves of 64 lanes) has the SCSFM_TRACK_TILE = 1024 pixels from 1024 g; n_groups =
 * ceil(H W / 1024).
 *  - Thread t starts from +0.0 and adds the terms of pixels 1024 g + t, + 256, + 512, + 768, in this order (a pixel at or
 *    past H W has terms of +0.0).
 *  - Inside a wave: six butterfly steps with lane masks 32, 16, 8, 4, 2, 1 in this order; in a step every lane l replaces
 *    its value by value(l) + value(l xor mask).  Addition commutes, so afterwards all lanes hold the same bits.
 *  - Across the four waves of a workgroup: ((wave 0 + wave 1) + wave 2) + wave 3, stored to the slab
 *    ws[v, g, 0 .. 28].  Every workgroup stores all 29 values: the slab needs no clearing.
 *  - Across workgroups: the solve kernel starts from +0.0 and adds ws[v, g, k] for g = 0 .. n_groups - 1 in index order
 *    (the launch-boundary reduce).
 * scsfm_track_ws_bytes(V, H, W) = V n_groups 29 sizeof(double).
 *
 * The solve, in double, one per frame.  S_0 .. S_28 are the sums; H is the symmetric 6 x 6 matrix of S_0 .. S_20,
 * g_i = S_21+i, count = S_28.
 *  - count < min_pairs: STATUS 1; the pivot ratio reported is 0.
 *  - else top = the largest of H_00 .. H_55 (top = H_00; then for i = 1 .. 5: if H_ii > top, top = H_ii).  Unless
 *    top > 0 (a NaN fails): STATUS 2, ratio 0.
 *  - else LDL^T, for j = 0 .. 5: D_j = H_jj, then for k = 0 .. j - 1 in order D_j = D_j - fl(fl(L_jk L_jk) D_k).  The
 *    ratio of the pivot is D_j / top, and the smallest ratio so far is kept (ratio < smallest; it starts from the first).
 *    Unless D_j > fl(SCSFM_TRACK_PIVOT_EPS top): STATUS 2, and the factorisation stops there.  Else for i = j + 1 .. 5:
 *    L_ij = H_ij, then for k = 0 .. j - 1 in order L_ij = L_ij - fl(fl(L_ik L_jk) D_k), then L_ij = L_ij / D_j.
 *  - H x = -g: y_i = -g_i, then for k = 0 .. i - 1 in order y_i = y_i - fl(L_ik y_k) (i = 0 .. 5); z_i = y_i / D_i;
 *    x_i = z_i, then for k = i + 1 .. 5 in order x_i = x_i - fl(L_ki x_k) (i = 5 .. 0).  t = (x_0 x_1 x_2),
 *    w = (x_3 x_4 x_5).  A component with x_i - x_i != 0 (an infinity or a NaN): STATUS 2.
 *  - STATUS 1 or 2 leaves the state and its record bit for bit as they were.
 *  - STATUS 0: c_i = c_i + t_i.  h_i = 0.5 w_i; len = sqrt(((1 + h_0 h_0) + h_1 h_1) + h_2 h_2);
 *    dq = (1 / len, h_0 / len, h_1 / len, h_2 / len) =: (dw dx dy dz).  The Hamilton product dq (x) q:
 *        w' = ((dw w - dx x) - dy y) - dz z        x' = ((dw x + dx w) + dy z) - dz y
 *        y' = ((dw y - dx z) + dy w) + dz x        z' = ((dw z + dx y) - dy x) + dz w
 *    then NORMALISE as above.  A rational retraction: the same fixed points as the exponential map, no trigonometry.
 *    The record's first twelve floats are rewritten from the new state.
 *  - The report row report[v, iteration, 0 .. 3]: count, S_27 (the sum of r r), the status, the smallest pivot ratio --
 *    the values before the update.
 */
#ifndef SCSFM_TRACK_H_
#define SCSFM_TRACK_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCSFM_TRACK_ERR_ARG (-1)
#define SCSFM_TRACK_STATE 7          /* doubles per state */
#define SCSFM_TRACK_RECORD 16        /* floats per pose record (SCSFM_CAST_VIEW) */
#define SCSFM_TRACK_SUMS 29          /* doubles per frame and workgroup */
#define SCSFM_TRACK_TILE 1024        /* pixels per workgroup */
#define SCSFM_TRACK_REPORT 4         /* doubles per frame and iteration */
#define SCSFM_TRACK_MAX_ITERS 64
#define SCSFM_TRACK_PIVOT_EPS 1e-8

/* 1 (first version) */
int scsfm_track_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: track_source_id) into buf, NUL-terminated */
int scsfm_track_source_id(char* buf, size_t n);

/* bytes of the slab of partial sums; 0 for a rejected argument (a size <= 0, H W or V n_groups 29 past int) */
size_t scsfm_track_ws_bytes(int V, int H, int W);

/* c2w [V, 12] doubles, K [9] floats (row-major 3 x 3) -> state [V, 7] doubles and est [V, 16] floats, all sixteen.
   Rejected: V <= 0, V 16 past int, a NULL pointer, c2w or state not aligned to 8 bytes, K or est to 4. */
int scsfm_track_init(int V, const double* c2w, const float* K, double* state, float* est, void* stream);

/* state [V, 7] -> c2w [V, 12] doubles.  Rejected: V <= 0, V 16 past int, a NULL or misaligned (8 bytes) pointer. */
int scsfm_track_poses(int V, const double* state, double* c2w, void* stream);

/* Enqueues n_iters x (accumulate, solve): 2 n_iters launches for all V frames, see above.  depth [V, H, W] fp32 (the
   nets' disparity with is_disp != 0); ref [V, 16]; model_depth [V, H, W]; model_normal [V, 3, H, W]; state [V, 7] and
   est [V, 16], read and updated; ws: scsfm_track_ws_bytes(V, H, W) bytes; report [V, n_iters, 4] doubles.  Rejected: a
   size <= 0, H W, V 3 H W or V n_groups 29 past int, max_dist or max_depth not positive and finite, near < 0 (or NaN or
   infinite), n_iters outside 1 .. 64, min_pairs < 6, a NULL pointer, a float pointer not aligned to 4 bytes, a double
   pointer not aligned to 8. */
int scsfm_track_iterate(int V, int H, int W, const float* depth, int is_disp, float near_d, float max_depth,
                        const float* ref, const float* model_depth, const float* model_normal, float max_dist,
                        int min_pairs, int n_iters, double* state, float* est, double* ws, double* report,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_TRACK_H_ */
