/*
 * scsfm_snip.h -- C ABI of libscsfm_snip.so: the 5-frame snippet protocol of test_pose.py with
 * kitti_eval/pose_evaluation_utils.py (ATE and RE, mean and std over every snippet of a set of KITTI odometry
 * sequences) as hand-written HIP kernels for gfx950 (MI355X).
 *
 * Conventions (as include/scsfm_odom.h)
 *  - All pointers are DEVICE pointers; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_SNIP_ERR_ARG (-1) for a rejected argument (before any pointer is touched),
 *    otherwise the hipError_t of the failed launch.  Every output is stored (overwritten), never accumulated.
 *  - No float atomics: every sum is reduced in a fixed order.  A snippet's numbers depend only on that snippet's own
 *    frames, so they are bit-identical from run to run and however the sequences are grouped into calls; the order
 *    in which `stats` is reduced depends only on n_snip.
 *
 * Arithmetic.  A pose is the affine map (A, t), a row of 12 doubles: the upper 3x4 of a 4x4 transform, row-major
 * (KITTI's text format).  Products and inverses are written out in double with separate roundings (no fused
 * multiply-add), each dot product summed left to right:
 *    (A1, t1) (A2, t2) = (A1 A2, (A1 t2) + t1)          (A1 A2)_ij = (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j
 *    inv(A, t) = (adj(A) / det A, -(A^-1 t))              det A = (a00 C00 + a01 C01) + a02 C02 (cofactors of row 0)
 * The inverse is the GENERAL inverse (every adjugate entry divided by the determinant): KITTI's ground-truth rotations
 * are orthonormal only to 1e-7, so a transpose is not what numpy.linalg.inv returns.  A sum over the translation
 * entries of a snippet runs frame after frame, x y z within a frame, left to right.
 */
#ifndef SCSFM_SNIP_H_
#define SCSFM_SNIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCSFM_SNIP_ERR_ARG (-1)

/* rotation parametrisation of a pose vector (tx ty tz rx ry rz), as pose_vec2mat's rotation_mode */
#define SCSFM_SNIP_ROT_EULER 0
#define SCSFM_SNIP_ROT_QUAT 1

#define SCSFM_SNIP_MIN_LEN 2   /* frames per snippet: 2 <= seq_len <= 16 */
#define SCSFM_SNIP_MAX_LEN 16
#define SCSFM_SNIP_STATS 4     /* doubles in `stats` */

/* 1 (first version) */
int scsfm_snip_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: snip_source_id) into buf, NUL-terminated */
int scsfm_snip_source_id(char* buf, size_t n);

/* bytes of workspace scsfm_snip_eval needs for S sequences of total_frames frames in all (12 doubles per frame: the
   inverted pair matrices); 0 for a rejected argument (S < 1, seq_len outside [2, 16], total_frames == 0 or too large) */
size_t scsfm_snip_workspace_bytes(int S, int seq_len, size_t total_frames);

/* test_pose.py's loop for every snippet of S sequences.
   Layout.  Sequence s has len[s] >= 0 frames.  Its ground-truth poses are rows [frame_off[s], frame_off[s] + len[s])
   of gt[total_frames, 12] (KITTI rows, double).  Its pair vectors are rows [frame_off[s], frame_off[s] + len[s] - 1)
   of vec[total_frames, 6] (float when vec_f64 == 0, double otherwise): row frame_off[s] + k is
   pose_net(img_k, img_{k+1}); the last row of each sequence is unused (it is read, its value reaches no output).
   Sequence s owns max(0, len[s] - seq_len + 1) snippets, numbered from snip_off[s]; snippet j of a sequence covers its
   frames j .. j + seq_len - 1.  n_snip is the total number of snippets; n_snip < 1 or n_snip > total_frames is rejected.
   (The tables live on the device, so a table that disagrees with n_snip cannot be rejected by the return value: a
   snippet number that the tables do not place inside a sequence and inside total_frames gets NaN errors, and its
   rows of pred / gt_comp are left as they were.)
   Three launches:
     1. one lane per row of vec: T_k = pose_vec2mat(vec_k) -- rotation (euler: R = Rx Ry Rz in closed form; quat:
        (1, x, y, z) normalised) and translation in the INPUT precision, in the closed forms of scsfm_pose_vec2mat_fwd
        -- lifted to double and inverted into the workspace, so that each inverse is formed once.
     2. one lane per snippet:
          P_0 = I, P_i = P_{i-1} inv(T_{j+i-1})          folded one after the other in this order (the reference's
                                                         own association)
          ground truth, as test_framework_KITTI.generator: t_i <- t_i - t_0 for every frame, then every 3x4 multiplied
          from the left by the general inverse of the first frame's 3x3
          compute_pose_error: scale = sum(gt_t pred_t) / sum(pred_t^2) over the 3 seq_len translation entries,
          ATE = sqrt(sum (gt_t - scale pred_t)^2) / seq_len; per frame R = gt_R inv(pred_R),
          s = sqrt(((R01 - R10)^2 + (R12 - R21)^2) + (R02 - R20)^2), c = ((R00 + R11) + R22) - 1,
          RE = sum atan2(s, c) / seq_len.  A zero denominator gives the NaN or inf numpy gives.
     3. one workgroup: the statistics over the errors ROUNDED TO FLOAT (the reference keeps them in a float32 array),
        accumulated in double: mean = sum / n_snip, std = sqrt(sum (x - mean)^2 / n_snip) (numpy.std, ddof 0, two
        passes); each sum thread-strided, then a wave's shuffle tree, then the waves in order.
   Outputs:
     pred[n_snip, seq_len, 12]      the folded poses P_i
     gt_comp[n_snip, seq_len, 12]   the compensated ground truth; may be NULL
     errors[n_snip, 2]              (ATE, RE), unrounded doubles
     stats[4]                       mean ATE, mean RE, std ATE, std RE */
int scsfm_snip_eval(int S, int seq_len, int vec_f64, int rot_mode, const void* vec, const double* gt,
                    const int* frame_off, const int* len, const int* snip_off, size_t total_frames, size_t n_snip,
                    double* pred, double* gt_comp, double* errors, double* stats, void* workspace,
                    size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_SNIP_H_ */
