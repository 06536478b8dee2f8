// The validation pass's table on the device (include/scsfm_val.h, ABI 2): every batch leaves one row of 8 doubles --
// seven values and a 1.0 that marks the row as present -- and the pass is reduced once, at its end, by the arithmetic of
// logger.AverageMeter (sum += v; avg = sum / count) over the present rows in row order.
//
//  batch_row    the mean over a batch's images of scsfm_val_depth_errors' six metrics, behind that call's four launches
//               on the same stream: what scsfm_hip.validation.batch_mean computes on the host.
//  losses_row   three fp32 device scalars widened to double: the list validate_without_gt hands to its AverageMeter.
//  table_mean   the mean of the present rows and their number.
//
// Each kernel is one wave in which lane k owns column k: it adds its column in a fixed order in double and stores it with
// one vector store.  No lane reads what another wrote, so there is no barrier, no LDS and no atomic, and the order of
// every sum -- which is the contract -- is the loop's.  They run once per batch or once per pass on a few hundred bytes.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "scsfm_val.h"

#pragma clang fp contract(off)

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kCols = 8;     // doubles in a row
constexpr int kValues = 7;   // of which values; column 7 is the presence mark
constexpr int kMetrics = 6;  // values scsfm_val_depth_errors gives per image
constexpr int kLanes = 64;

__global__ __launch_bounds__(kLanes) void batch_row_kernel(int B, const double* __restrict__ metrics,
                                                           double* __restrict__ row) {
  const int k = threadIdx.x;
  if (k >= kCols) return;
  double v = k == kCols - 1 ? 1.0 : 0.0;
  if (k < kMetrics) {
    double s = metrics[k];
    for (int i = 1; i < B; ++i) s += metrics[(long long)i * kMetrics + k];
    v = s / (double)B;
  }
  row[k] = v;
}

__global__ __launch_bounds__(kLanes) void losses_row_kernel(const float* __restrict__ photo,
                                                            const float* __restrict__ smooth,
                                                            const float* __restrict__ geom, double* __restrict__ row) {
  const int k = threadIdx.x;
  if (k >= kCols) return;
  double v = k == kCols - 1 ? 1.0 : 0.0;
  if (k < 2) v = (double)photo[0];  // (the reference's 'Total loss' column repeats the photometric loss)
  if (k == 2) v = (double)smooth[0];
  if (k == 3) v = (double)geom[0];
  row[k] = v;
}

__global__ __launch_bounds__(kLanes) void table_mean_kernel(int n_rows, const double* __restrict__ table,
                                                            double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= kCols) return;
  double s = 0.0;
  int n = 0;
  for (int r = 0; r < n_rows; ++r) {
    const double* row = table + (long long)r * kCols;
    if (row[kCols - 1] == 1.0) {
      s += row[k];
      ++n;
    }
  }
  out[k] = k == kCols - 1 ? (double)n : (n > 0 ? s / (double)n : 0.0);
}

}  // namespace

extern "C" {

int scsfm_val_depth_errors_row(int B, int h, int w, const float* src, int src_is_disp, int H, int W, const float* gt,
                               int y1, int y2, int x1, int x2, float min_gt, float max_depth, float clamp_lo,
                               void* workspace, size_t workspace_bytes, double* metrics, float* medians, int* count,
                               double* row, void* stream) {
  if (!row) return SCSFM_VAL_ERR_ARG;
  // (rejects everything else before its first launch, B <= 0 included)
  const int rc = scsfm_val_depth_errors(B, h, w, src, src_is_disp, H, W, gt, y1, y2, x1, x2, min_gt, max_depth, clamp_lo,
                                        workspace, workspace_bytes, metrics, medians, count, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(batch_row_kernel, dim3(1), dim3(kLanes), 0, (hipStream_t)stream, B, metrics, row);
  return (int)hipGetLastError();
}

int scsfm_val_losses_row(const float* photo, const float* smooth, const float* geom, double* row, void* stream) {
  if (!photo || !smooth || !geom || !row) return SCSFM_VAL_ERR_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(losses_row_kernel, dim3(1), dim3(kLanes), 0, (hipStream_t)stream, photo, smooth, geom, row);
  return (int)hipGetLastError();
}

int scsfm_val_table_mean(int n_rows, const double* table, double* out, void* stream) {
  if (n_rows <= 0 || (long long)n_rows * kCols >= (1ll << 31) || !table || !out) return SCSFM_VAL_ERR_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(table_mean_kernel, dim3(1), dim3(kLanes), 0, (hipStream_t)stream, n_rows, table, out);
  return (int)hipGetLastError();
}

}  // extern "C"
