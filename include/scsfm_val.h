/*
 * scsfm_val.h -- C ABI of libscsfm_val.so, ABI 2: the validation pass of training as hand-written HIP kernels for gfx950
 * (MI355X).  ABI 1 is the ground-truth validation metrics (train.py --with-gt: validate_with_gt's nearest resize and
 * loss_functions.compute_errors); ABI 2 adds the pass's table on the device (train.py --shard-validation), below.
 * Per image: the prediction (or 1 / disparity) is taken at the ground truth's size by nearest neighbour, the valid GT
 * pixels are masked and cropped, the prediction is clamped and scaled by median(gt) / median(pred) with torch.median's
 * lower middle element, and the six error terms are reduced.  Everything is fp32, as the reference's tensors are; only
 * the sums are double.
 *
 * Conventions (as include/scsfm_eval.h)
 *  - All pointers are DEVICE pointers; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_VAL_ERR_ARG (-1) for a rejected argument, otherwise the hipError_t of the
 *    failed launch.  Every output is stored (overwritten), never accumulated.  A rejected call writes nothing.
 *  - Results are bit-identical from run to run and however a batch is split into calls.
 */
#ifndef SCSFM_VAL_H_
#define SCSFM_VAL_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCSFM_VAL_ERR_ARG (-1)

/* 2 (1: the first version, everything up to scsfm_val_depth_errors; 2: the table of a validation pass) */
int scsfm_val_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: val_source_id) into buf, NUL-terminated */
int scsfm_val_source_id(char* buf, size_t n);

/* bytes of workspace scsfm_val_depth_errors needs for B ground-truth maps of H x W; 0 for a rejected argument */
size_t scsfm_val_workspace_bytes(int B, int H, int W);

/* Validation errors of B images.
     src[B, h, w]   fp32: the predicted depth, or with src_is_disp = 1 the network's disparity, of which the kernel
                    takes 1.0f / x (a correctly rounded fp32 division).  Where (h, w) != (H, W) the value at GT pixel
                    (y, x) is src[min((int)floorf(y * sy), h - 1), min((int)floorf(x * sx), w - 1)] with
                    sy = (float)h / (float)H and sx = (float)w / (float)W in fp32: F.interpolate's default (nearest).
     gt[B, H, W]    fp32.
     y1, y2, x1, x2 the crop box, 0 <= y1 <= y2 <= H and 0 <= x1 <= x2 <= W.
   A pixel is valid when gt > min_gt && gt < max_depth (fp32 comparisons: a NaN is invalid) inside the box.  With
   p = clamp(pred, clamp_lo, max_depth) (a NaN stays NaN), med_gt and med_pred the order statistics (n - 1) / 2 of the
   valid gt and p (torch.median), and p' = (p * med_gt) / med_pred, the fp32 terms |gt - p'|, |gt - p'| / gt,
   ((gt - p') * (gt - p')) / gt and t = max(gt / p', p' / gt) are summed in double in a fixed order.
   Outputs, per image i:
     metrics[i*6 + 0..5] = abs_diff, abs_rel, sq_rel, a1, a2, a3 (the means; a_k: the share of t < 1.25^k)
     medians[i*2 + 0..1] = med_gt, med_pred
     count[i]            = n, the number of valid pixels
   n == 0 gives six NaN, both medians NaN and count 0.  A NaN among the valid p gives med_pred = NaN and six NaN.
   Rejected: a size <= 0 (or B * H * W or h * w at or beyond 2^31), a crop box outside [0, H] x [0, W] or reversed,
   !(min_gt < max_depth), a null pointer, workspace_bytes < scsfm_val_workspace_bytes(B, H, W). */
int scsfm_val_depth_errors(int B, int h, int w, const float* src, int src_is_disp, int H, int W, const float* gt,
                           int y1, int y2, int x1, int x2, float min_gt, float max_depth, float clamp_lo,
                           void* workspace, size_t workspace_bytes, double* metrics, float* medians, int* count,
                           void* stream);

/* The table of a validation pass (ABI 2).
   A ROW is 8 doubles: columns 0..6 are values, column 7 is 1.0 for a row that is present.  The TABLE of a pass is
   [n_batches, 8] doubles, zeroed by the caller; row i belongs to batch i of the pass, and each call below stores one
   whole row (8 doubles).  A pass split over processes adds its tables up (every row is non-zero in one of them, and
   x + 0.0 == x) and reduces the sum with scsfm_val_table_mean: the result does not depend on the split. */

/* scsfm_val_depth_errors, bit for bit (the same metrics, medians and count), and behind it on the same stream
     row[k] = (metrics[0*6 + k] + metrics[1*6 + k] + ... + metrics[(B-1)*6 + k]) / (double)B   for k < 6,
   added in image order in double; row[6] = 0, row[7] = 1.  An image whose metrics are NaN makes the six columns NaN.
   Rejected: a null row, and everything scsfm_val_depth_errors rejects. */
int scsfm_val_depth_errors_row(int B, int h, int w, const float* src, int src_is_disp, int H, int W, const float* gt,
                               int y1, int y2, int x1, int x2, float min_gt, float max_depth, float clamp_lo,
                               void* workspace, size_t workspace_bytes, double* metrics, float* medians, int* count,
                               double* row, void* stream);

/* Three fp32 device scalars as a row: { (double)photo, (double)photo, (double)smooth, (double)geom, 0, 0, 0, 1 } -- the
   list validate_without_gt hands to its AverageMeter, whose first column repeats the photometric loss.
   Rejected: a null pointer. */
int scsfm_val_losses_row(const float* photo, const float* smooth, const float* geom, double* row, void* stream);

/* The mean of the present rows of table[n_rows, 8] into out[8]: for k < 7, out[k] is the sum of column k over the rows
   whose column 7 equals 1.0, added in row order in double starting from 0.0, divided by their number; out[7] is that
   number.  With no present row out[0..6] are 0.0.  (logger.AverageMeter's sum += v; avg = sum / count.)
   Rejected: n_rows <= 0, n_rows * 8 at or beyond 2^31, a null pointer. */
int scsfm_val_table_mean(int n_rows, const double* table, double* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_VAL_H_ */
