/*
 * scsfm_eval.h -- C ABI of libscsfm_eval.so: monocular depth evaluation (eval_depth.py, DepthEvalEigen.evaluate_depth
 * with eval_mono=True) as hand-written HIP kernels for gfx950 (MI355X).  Per image: the prediction's inverse depth is
 * resized to the ground truth's own size (bilinear, OpenCV INTER_LINEAR's generic path), the valid GT pixels are
 * masked (and cropped for KITTI), both depths are median-scaled and the eight error sums are reduced.
 *
 * Conventions (as include/scsfm_hip.h and include/scsfm_nets.h)
 *  - All pointers are DEVICE pointers; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_EVAL_ERR_ARG (-1) for a rejected argument, otherwise the hipError_t of the
 *    failed launch.  Every output is stored (overwritten), never accumulated.
 *  - Ragged ground truth: image i's GT map is gt[gt_off[i] .. gt_off[i] + gt_h[i] * gt_w[i]) row-major.  Offsets that
 *    are multiples of 4 elements let the kernels use vector loads (others are read element by element).  Predictions
 *    are uniform: pred[N, h, w].  `pred_f64` / `gt_f64` select double (1) or float (0) elements.
 *  - Arithmetic follows numpy's promotion with R = promote(GT, pred): the resize runs in the prediction's precision,
 *    the mask compares in the GT's, the ratio is R(median gt) / R(median pred), the scaled prediction is
 *    pred(R(pred) * ratio), the element-wise error terms are in R except log(gt) / log10(gt) (GT precision) and
 *    log(pred) / log10(pred) (prediction precision).  The eight sums are accumulated in double in a fixed order.
 */
#ifndef SCSFM_EVAL_H_
#define SCSFM_EVAL_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCSFM_EVAL_ERR_ARG (-1)

/* 1 (first version) */
int scsfm_eval_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: eval_source_id) into buf, NUL-terminated */
int scsfm_eval_source_id(char* buf, size_t n);

/* bytes of workspace scsfm_eval_depth needs for N images whose largest GT map has max_hw pixels and whose packed GT
   buffer spans `total` elements; 0 for a rejected argument */
size_t scsfm_eval_workspace_bytes(int N, int max_hw, size_t total, int pred_f64, int gt_f64);

/* Evaluates N images.  crop: 1 applies the KITTI Eigen crop (rows [int(0.40810811 H), int(0.99189189 H)), columns
   [int(0.03594771 W), int(0.96405229 W))).  min_depth < max_depth bound the GT mask (gt > min, gt < max, compared in
   the GT's precision) and clamp the scaled prediction.
   Outputs, per image i:
     metrics[i*8 + 0..7] = abs_rel, sq_rel, rmse, rmse_log, log10, a1, a2, a3   (NaN when the mask is empty)
     stats[i*3 + 0..2]   = ratio, median(gt[mask]), median(pred[mask])       (each exact in its own precision)
     count[i]            = the number of valid pixels
     flag[i]             = 1 evaluated, 0 skipped (the prediction's mean, summed in double, is exactly -1; its other
                           outputs are then NaN)
   Medians are numpy's: the mean of the two middle order statistics for an even count, in the array's precision. */
int scsfm_eval_depth(int N, int h, int w, int pred_f64, const void* pred, int gt_f64, const void* gt,
                     const long long* gt_off, const int* gt_h, const int* gt_w, int max_hw, size_t total, int crop,
                     double min_depth, double max_depth, void* workspace, size_t workspace_bytes, double* metrics,
                     double* stats, int* count, int* flag, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_EVAL_H_ */
