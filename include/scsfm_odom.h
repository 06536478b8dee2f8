/*
 * scsfm_odom.h -- C ABI of libscsfm_odom.so: KITTI visual odometry testing and evaluation (test_vo.py's pose fold and
 * kitti_eval/kitti_odometry.py's KittiEvalOdom.eval) as hand-written HIP kernels for gfx950 (MI355X).
 *
 * Conventions (as include/scsfm_hip.h, include/scsfm_nets.h and include/scsfm_eval.h)
 *  - All pointers are DEVICE pointers; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_ODOM_ERR_ARG (-1) for a rejected argument (before any pointer is touched),
 *    otherwise the hipError_t of the failed launch.  Every output is stored (overwritten), never accumulated.
 *  - Ragged sets: sequence s owns rows [off[s], off[s] + len[s]) of every packed per-row buffer of the call.  A pose is
 *    a row of 12 doubles: the upper 3x4 of a 4x4 transform, row-major (KITTI's text format).
 *  - No float atomics: every sum is reduced in a fixed order that depends only on the sequence's own data, so results
 *    are bit-identical from run to run and however the sequences are grouped into calls.
 *
 * Arithmetic.  A pose is the affine map (A, t).  Products and inverses are written out with separate roundings
 * (no fused multiply-add), each dot product summed left to right:
 *    (A1, t1) (A2, t2) = (A1 A2, (A1 t2) + t1)          (A1 A2)_ij = (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j
 *    inv(A, t) = (adj(A) / det A, -(A^-1 t))              det A = (a00 C00 + a01 C01) + a02 C02 (cofactors of row 0)
 * The inverse is the GENERAL inverse (every adjugate entry divided by the determinant): KITTI's ground-truth rotations
 * are orthonormal only to 1e-7, so a transpose is not what numpy.linalg.inv returns.
 */
#ifndef SCSFM_ODOM_H_
#define SCSFM_ODOM_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCSFM_ODOM_ERR_ARG (-1)

/* rotation parametrisation of a pose vector (tx ty tz rx ry rz), as pose_vec2mat's rotation_mode */
#define SCSFM_ODOM_ROT_EULER 0
#define SCSFM_ODOM_ROT_QUAT 1

/* KittiEvalOdom.eval's `alignment` */
#define SCSFM_ODOM_ALIGN_NONE 0       /* None */
#define SCSFM_ODOM_ALIGN_SCALE 1      /* "scale":      translations *= sum(X Y) / sum(X^2) */
#define SCSFM_ODOM_ALIGN_SCALE_7DOF 2 /* "scale_7dof": Umeyama with scale, only the scale is applied */
#define SCSFM_ODOM_ALIGN_7DOF 3       /* "7dof":       Umeyama with scale, scale then [r|t] applied */
#define SCSFM_ODOM_ALIGN_6DOF 4       /* "6dof":       Umeyama without scale (c = 1), [r|t] applied */

#define SCSFM_ODOM_LENGTHS 8   /* segment lengths 100, 200, ..., 800 m */
#define SCSFM_ODOM_STEP 10     /* every 10th frame starts a segment */
#define SCSFM_ODOM_SUMMARY 7   /* doubles per sequence in `summary` */

/* 1 (first version) */
int scsfm_odom_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: odom_source_id) into buf, NUL-terminated */
int scsfm_odom_source_id(char* buf, size_t n);

/* bytes of workspace scsfm_odom_chain needs for S sequences whose longest has max_len pose vectors; 0 for a rejected
   argument */
size_t scsfm_odom_chain_workspace_bytes(int S, int max_len);

/* test_vo.py's fold.  Sequence s has len[s] >= 0 pose vectors, rows [off[s], off[s] + len[s]) of vec[total, 6]
   (float when vec_f64 == 0, double otherwise), and receives len[s] + 1 global poses, rows [out_off[s], out_off[s] +
   len[s] + 1) of poses (12 doubles each):
       T_k = pose_vec2mat(vec_k)     rotation (euler: R = Rx Ry Rz in closed form; quat: (1, x, y, z) normalised) and
                                     translation in the INPUT precision, exactly as scsfm_pose_vec2mat_fwd forms them
       G_0 = I,  G_k = G_{k-1} inv(T_k)    T_k lifted to double, general inverse and products as above
   The prefix product is a scan over the associative composition of affine maps: within a wave by shuffles, across the
   waves of a workgroup through LDS, across workgroups through `workspace` (three launches for any S and max_len).  The
   association differs from the sequential fold's, so a pose may differ from it by rounding (n eps max|position|).
   local: if not NULL, [total, 12] in the input precision, receives T_k (what pose_vec2mat returns).
   max_len >= every len[s]. */
int scsfm_odom_chain(int S, int max_len, int vec_f64, int rot_mode, const void* vec, const int* off, const int* len,
                     const int* out_off, void* local, double* poses, void* workspace, size_t workspace_bytes,
                     void* stream);

/* rows of the segment table per sequence that scsfm_odom_eval needs for a longest sequence of max_len frames:
   SCSFM_ODOM_LENGTHS * ceil(max_len / SCSFM_ODOM_STEP); 0 for a rejected argument */
size_t scsfm_odom_eval_max_segments(int max_len);
/* bytes of workspace scsfm_odom_eval needs; `total` is the number of packed rows; 0 for a rejected argument */
size_t scsfm_odom_eval_workspace_bytes(int S, int max_len, size_t total);

/* KittiEvalOdom.eval for S sequences.  gt and pred are packed [total, 12]; sequence s has len[s] >= 1 frames, rows
   [off[s], off[s] + len[s]) of both (frame i of the prediction belongs to frame i of the ground truth).  Five launches:
     1. both trajectories are re-based on their first frame, X_i <- inv(X_0) X_i; GT step lengths
        sqrt((dx^2 + dy^2) + dz^2) between consecutive re-based GT positions.
     2. per sequence: the cumulative GT distance (a scan; dist_0 = 0) and the alignment:
          scale:   c = sum(X Y) / sum(X^2) over the 3n coordinates of the predicted (X) and GT (Y) positions
          Umeyama: mean_x, mean_y = sums / n; sigma_x = (1 / n) sqrt(sum |x - mean_x|^2)^2; C = (1 / n) sum (y - mean_y)
                   (x - mean_x)^T; C = U D V^T by one-sided Jacobi in double, D descending; s = diag(1, 1, -1) if
                   det U det V^T < 0 else I; r = U s V^T; c = (1 / sigma_x) (d0 + d1 + s22 d2) (1 for 6dof);
                   t = mean_y - c (r mean_x)
     3. per frame: the predicted translation is multiplied by c, then (7dof, 6dof) the pose by [r|t] from the left;
        ATE and RPE terms of the frame.
     4. one lane per (first frame f = 0, 10, 20, ..; length L = 100 .. 800): the first frame l >= f with
        dist_l > dist_f + L (strict, in double; binary search on the non-decreasing distances); the pose error
        E = inv(inv(P_f) P_l) (inv(G_f) G_l), r_err = acos(clamp(0.5 (((E00 + E11) + E22) - 1))),
        t_err = sqrt((E03^2 + E13^2) + E23^2), speed = L / (0.1 (l - f + 1)).
     5. per sequence: the found segments compacted in the reference's order (by first frame, then by length) and the
        means.
   Outputs, per sequence s:
     summary[s*7 + 0..6] = mean t_err / L over the segments, mean r_err / L, ATE = sqrt(mean |g_i - p_i|^2),
                           RPE translation (mean), RPE rotation (mean; both of E = inv(inv(G_i) G_i+1) (inv(P_i) P_i+1),
                           NaN for a one-frame sequence), the alignment's scale c (1 for none), the number of segments.
                           The two segment means are 0 when there is no segment.
     per_length[s*24 + k*3 + 0..2] = mean t_err / L, mean r_err / L, count of the segments of length 100 (k + 1)
                           (0, 0, 0 when there is none)
     seg[(s * max_seg + j) * 5 + 0..4] = first_frame, r_err / L, t_err / L, L, speed of segment j < n_seg[s]; rows
                           j >= n_seg[s] are zero.  max_seg >= scsfm_odom_eval_max_segments(max_len).
     n_seg[s]
     gt_rel[total, 12], aligned[total, 12]: the re-based ground truth and the re-based, aligned prediction. */
int scsfm_odom_eval(int S, int max_len, size_t total, int align, const double* gt, const double* pred, const int* off,
                    const int* len, int max_seg, void* workspace, size_t workspace_bytes, double* summary,
                    double* per_length, double* seg, int* n_seg, double* gt_rel, double* aligned, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_ODOM_H_ */
