/*
 * scsfm_sim3.h -- C ABI of libscsfm_sim3.so: frame-to-model tracking with a scale.  A frame's depth map, times a scale of
 * its own, is aligned to the depth and normal maps that libscsfm_cast.so cast from the fused volume (include/scsfm_cast.h)
 * by point-to-plane ICP (iterative closest point) over seven degrees of freedom: the six of a rigid motion and the
 * logarithm of the frame's depth scale.  A projective association per pixel, 37 double-precision sums per frame, a 7 x 7
 * solve whose last unknown, the scale, is solved only where its pivot says it is observable, and a pose and scale update,
 * all on the device, as hand-written HIP kernels for gfx950 (MI355X).  The library takes the maps and never sees the volume.
 * It states the rigid tracker of include/scsfm_track.h again in full, with the scale, and the two libraries are built from
 * one core (sc-sfmlearner-release_amd/csrc_icp/scsfm_icp.h): with a scale of 1 that is never solved (min_scale_pivot = +inf)
 * every pose it gives has the bits of libscsfm_track.so's.
 *
 * Conventions (as include/scsfm_cast.h)
 *  - All pointers are DEVICE pointers; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_SIM3_ERR_ARG (-1) for a rejected argument (before any pointer is touched),
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
 * State (SCSFM_SIM3_STATE = 8 doubles per frame): a unit quaternion (w, x, y, z), the camera centre (c0, c1, c2), camera to
 * world, and the scale sigma of the frame's depth.  Beside the states lies sigma_f [V], one float per frame: sigma rounded
 * once to fp32, rewritten whenever sigma changes.  It is the scale the pair of a pixel and scsfm_sim3_scale multiply with.
 *
 * The matrix of a quaternion, in double: with xx = x x, yy, zz, xy = x y, xz, yz, wx = w x, wy, wz,
 *     R00 = 1 - 2 (yy + zz)   R01 = 2 (xy - wz)       R02 = 2 (xz + wy)
 *     R10 = 2 (xy + wz)       R11 = 1 - 2 (xx + zz)   R12 = 2 (yz - wx)
 *     R20 = 2 (xz - wy)       R21 = 2 (yz + wx)       R22 = 1 - 2 (xx + yy)
 * scsfm_sim3_poses writes the rows (R_i0 R_i1 R_i2 c_i), 12 doubles a frame, and copies sigma to scale [V].
 *
 * Pose record (16 floats per frame, scsfm_cast.h's view record): A row-major (a0 .. a8), the centre (c0 c1 c2), fx, fy,
 * cx, cy.  A is the matrix above and c the centre, each of the twelve doubles rounded once to fp32; fx = K[0], fy = K[4],
 * cx = K[2], cy = K[5] are written by scsfm_sim3_init and kept.  Whenever a state's pose changes, the first twelve floats
 * of its record are rewritten on the device.  The scale is no part of the record.
 *
 * scsfm_sim3_init: c2w [V, 12] doubles (rows m_i0 m_i1 m_i2 c_i) and scale0 [V] doubles -> states, records and sigma_f.
 * Shepperd's branch, with tr = (m00 + m11) + m22:
 *     tr >= m00, m11 and m22:      r = sqrt(1 + tr);                 w = r / 2; f = 0.5 / r;
 *                                  x = (m21 - m12) f; y = (m02 - m20) f; z = (m10 - m01) f
 *     else m00 >= m11 and m22:     r = sqrt(((1 + m00) - m11) - m22); x = r / 2; f = 0.5 / r;
 *                                  w = (m21 - m12) f; y = (m01 + m10) f; z = (m02 + m20) f
 *     else m11 >= m22:             r = sqrt(((1 + m11) - m00) - m22); y = r / 2; f = 0.5 / r;
 *                                  w = (m02 - m20) f; x = (m01 + m10) f; z = (m12 + m21) f
 *     else:                        r = sqrt(((1 + m22) - m00) - m11); z = r / 2; f = 0.5 / r;
 *                                  w = (m10 - m01) f; x = (m02 + m20) f; y = (m12 + m21) f
 * then NORMALISE: len = sqrt(((w w + x x) + y y) + z z), each component divided by len.  The centre is copied;
 * sigma = scale0[v], whatever it holds (the solve answers a scale that is not positive and finite), sigma_f = float(sigma).
 *
 * The pair of pixel (px, py) of frame v, in fp32.  a_ij, c, fx .. cy are the frame's record (the estimate); r_ij, c',
 * fx' .. cy' the reference record ref[v]; M [V, H, W] and N [V, 3, H, W] the model's depth and world normals that
 * scsfm_cast_cast wrote for ref[v].
 *  1. d0 = depth[v, py, px], or 1.0f / depth[v, py, px] with is_disp; d = fl(sigma_f[v] d0).  The pixel is a CANDIDATE iff
 *     d > near && d <= max_depth (a NaN fails).
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
 *     nu = (n_0 u_0 + n_1 u_1) + n_2 u_2 < 0: the model's surface faces the estimate's camera.  A NaN fails either test.
 *  7. r = (n_0 delta_0 + n_1 delta_1) + n_2 delta_2.  J = (n_0, n_1, n_2, fl(u_1 n_2) - fl(u_2 n_1),
 *     fl(u_2 n_0) - fl(u_0 n_2), fl(u_0 n_1) - fl(u_1 n_0), nu): the twist (t, w) about the estimate's own centre and the
 *     relative change lambda of the scale, p -> c + t + (I + [w]x)((1 + lambda)(p - c)).  Under sigma -> sigma (1 + lambda)
 *     the point moves by lambda u, so the residual's derivative J_6 is n . u: the very value step 6 tests.
 *  8. J and r are converted to double.  The pixel's 37 TERMS are the 28 products J_i J_j (i <= j; (0,0) (0,1) .. (0,6)
 *     (1,1) .. (6,6)), the 7 products J_i r, then r r, then 1.  A product of two fp32 values is exact in double.  A pixel
 *     that is no pair has 37 terms of +0.0.
 *
 * The sums (SCSFM_SIM3_SUMS = 37 doubles per frame), in double.  Pixels are numbered i = py W + px.  Workgroup g of a
 * frame (256 threads: 4 waves of 64 lanes) has the SCSFM_SIM3_TILE = 1024 pixels from 1024 g; n_groups =
 * ceil(H W / 1024).
 *  - Thread t starts from +0.0 and adds the terms of pixels 1024 g + t, + 256, + 512, + 768, in this order (a pixel at or
 *    past H W has terms of +0.0).
 *  - Inside a wave: six butterfly steps with lane masks 32, 16, 8, 4, 2, 1 in this order; in a step every lane l replaces
 *    its value by value(l) + value(l xor mask).  Addition commutes, so afterwards all lanes hold the same bits.
 *  - Across the four waves of a workgroup: ((wave 0 + wave 1) + wave 2) + wave 3, stored to the slab
 *    ws[v, g, 0 .. 36].  Every workgroup stores all 37 values: the slab needs no clearing.
 *  - Across workgroups: the solve kernel starts from +0.0 and adds ws[v, g, k] for g = 0 .. n_groups - 1 in index order
 *    (the launch-boundary reduce).
 * scsfm_sim3_ws_bytes(V, H, W) = V n_groups 37 sizeof(double).
 *
 * The solve, in double, one per frame.  S_0 .. S_36 are the sums; H is the symmetric 7 x 7 matrix of S_0 .. S_27,
 * g_i = S_28+i, count = S_36.  The scale is the LAST unknown, so the factors L_ij, the pivots D_j and the intermediate y_i
 * and z_i with i, j <= 5 are those of the rigid 6 x 6 system, whatever becomes of the scale.
 *  - Unless sigma > 0 && sigma - sigma == 0 (positive and finite; a NaN fails): STATUS 2; both ratios reported are 0.
 *  - else count < min_pairs: STATUS 1; both ratios are 0.
 *  - else top6 = the largest of H_00 .. H_55 (top6 = H_00; then for i = 1 .. 5: if H_ii > top6, top6 = H_ii).  Unless
 *    top6 > 0 (a NaN fails): STATUS 2, both ratios 0.  top = H_66 if H_66 > top6, else top6: the largest of H_00 .. H_66.
 *    The pose's pivots are judged against top6 and the scale's against top, so that the rigid part of the rule does not
 *    depend on the scale's column at all.
 *  - else LDL^T, for j = 0 .. 5: D_j = H_jj, then for k = 0 .. j - 1 in order D_j = D_j - fl(fl(L_jk L_jk) D_k).  The
 *    ratio of the pivot is D_j / top6, and the smallest ratio so far is kept (ratio < smallest; it starts from the first).
 *    Unless D_j > fl(SCSFM_SIM3_PIVOT_EPS top6): STATUS 2, the factorisation stops there and the scale's ratio is 0.  Else
 *    for i = j + 1 .. 6: L_ij = H_ij, then for k = 0 .. j - 1 in order L_ij = L_ij - fl(fl(L_ik L_jk) D_k), then
 *    L_ij = L_ij / D_j.
 *  - Pivot 6: D_6 = H_66, then for k = 0 .. 5 in order D_6 = D_6 - fl(fl(L_6k L_6k) D_k); its ratio is D_6 / top.  The
 *    scale is HELD unless D_6 > fl(min_scale_pivot top) (a NaN fails; min_scale_pivot = +inf holds every scale).
 *  - y_i = -g_i, then for k = 0 .. i - 1 in order y_i = y_i - fl(L_ik y_k) (i = 0 .. 6); z_i = y_i / D_i (i = 0 .. 6).
 *  - Unless z_6 > -1 && z_6 < 1 (a NaN fails) the scale is HELD after all.
 *  - Not held: x_6 = z_6, and for i = 5 .. 0: x_i = z_i, then for k = i + 1 .. 6 in order x_i = x_i - fl(L_ki x_k).
 *    Held: x_6 = 0, and for i = 5 .. 0: x_i = z_i, then for k = i + 1 .. 5 in order x_i = x_i - fl(L_ki x_k) -- the term of
 *    k = 6 is not formed: the step is the step of the 6 x 6 system, bit for bit.
 *    t = (x_0 x_1 x_2), w = (x_3 x_4 x_5), lambda = x_6.  A component with x_i - x_i != 0 (an infinity or a NaN): STATUS 2.
 *  - else STATUS 3 when the scale was held, for whichever reason, and STATUS 0 when it was not.
 *  - STATUS 1 or 2 leaves the state, its record and sigma_f bit for bit as they were.
 *  - STATUS 0 and 3: c_i = c_i + t_i.  h_i = 0.5 w_i; len = sqrt(((1 + h_0 h_0) + h_1 h_1) + h_2 h_2);
 *    dq = (1 / len, h_0 / len, h_1 / len, h_2 / len) =: (dw dx dy dz).  The Hamilton product dq (x) q:
 *        w' = ((dw w - dx x) - dy y) - dz z        x' = ((dw x + dx w) + dy z) - dz y
 *        y' = ((dw y - dx z) + dy w) + dz x        z' = ((dw z + dx y) - dy x) + dz w
 *    then NORMALISE as above.  A rational retraction: the same fixed points as the exponential map, no trigonometry.
 *    The record's first twelve floats are rewritten from the new state.
 *  - STATUS 0 also: h = 0.5 lambda; sigma = fl(fl(sigma fl(1 + h)) / fl(1 - h)); sigma_f = float(sigma).  The rational
 *    retraction of exp(lambda): positive for |h| < 1, and |h| < 0.5 here.  STATUS 3 leaves sigma and sigma_f their bits.
 *  - The report row report[v, iteration, 0 .. 5]: count, S_35 (the sum of r r), the status, the smallest ratio of pivots
 *    0 .. 5, the ratio of pivot 6 (0 when it was not reached), sigma -- the values before the update.
 */
#ifndef SCSFM_SIM3_H_
#define SCSFM_SIM3_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCSFM_SIM3_ERR_ARG (-1)
#define SCSFM_SIM3_STATE 8           /* doubles per state */
#define SCSFM_SIM3_RECORD 16         /* floats per pose record (SCSFM_CAST_VIEW) */
#define SCSFM_SIM3_SUMS 37           /* doubles per frame and workgroup */
#define SCSFM_SIM3_TILE 1024         /* pixels per workgroup */
#define SCSFM_SIM3_REPORT 6          /* doubles per frame and iteration */
#define SCSFM_SIM3_MAX_ITERS 64
#define SCSFM_SIM3_PIVOT_EPS 1e-8

/* 1 (first version) */
int scsfm_sim3_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: sim3_source_id) into buf, NUL-terminated */
int scsfm_sim3_source_id(char* buf, size_t n);

/* bytes of the slab of partial sums; 0 for a rejected argument (a size <= 0, H W or V n_groups 37 past int) */
size_t scsfm_sim3_ws_bytes(int V, int H, int W);

/* c2w [V, 12] doubles, scale0 [V] doubles, K [9] floats (row-major 3 x 3) -> state [V, 8] doubles, est [V, 16] floats, all
   sixteen, and sigma_f [V] floats.  Rejected: V <= 0, V 16 past int, a NULL pointer, c2w, scale0 or state not aligned to 8
   bytes, K, est or sigma_f to 4. */
int scsfm_sim3_init(int V, const double* c2w, const double* scale0, const float* K, double* state, float* est,
                    float* sigma_f, void* stream);

/* state [V, 8] -> c2w [V, 12] doubles and scale [V] doubles.  Rejected: V <= 0, V 16 past int, a NULL or misaligned (8
   bytes) pointer. */
int scsfm_sim3_poses(int V, const double* state, double* c2w, double* scale, void* stream);

/* Enqueues n_iters x (accumulate, solve): 2 n_iters launches for all V frames, see above.  depth [V, H, W] fp32 (the
   nets' disparity with is_disp != 0); ref [V, 16]; model_depth [V, H, W]; model_normal [V, 3, H, W]; state [V, 8], est
   [V, 16] and sigma_f [V], read and updated; ws: scsfm_sim3_ws_bytes(V, H, W) bytes; report [V, n_iters, 6] doubles.
   Rejected: a size <= 0, H W, V 3 H W or V n_groups 37 past int, max_dist or max_depth not positive and finite, near < 0
   (or NaN or infinite), min_scale_pivot not > 0 (a NaN; +inf is taken: no scale is ever solved), n_iters outside 1 .. 64,
   min_pairs < 7, a NULL pointer, a float pointer not aligned to 4 bytes, a double pointer not aligned to 8. */
int scsfm_sim3_iterate(int V, int H, int W, const float* depth, int is_disp, float near_d, float max_depth,
                       const float* ref, const float* model_depth, const float* model_normal, float max_dist,
                       int min_pairs, double min_scale_pivot, int n_iters, double* state, float* est, float* sigma_f,
                       double* ws, double* report, void* stream);

/* out[v, i] = fl(sigma_f[v] d0), d0 = depth[v, i] or 1.0f / depth[v, i] with is_disp, for depth and out [V, H, W] fp32:
   step 1's d, bit for bit -- the depth the tracker saw, which is what is integrated (as a depth, not a disparity) at the
   refined pose.  One pass over the frames.  out may not overlap depth.  Rejected: a size <= 0, V H W above 2^31 - 1 - 1024
   (a launch's last thread must index inside int), a NULL pointer or one not aligned to 4 bytes. */
int scsfm_sim3_scale(int V, int H, int W, const float* depth, int is_disp, const float* sigma_f, float* out,
                     void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_SIM3_H_ */
