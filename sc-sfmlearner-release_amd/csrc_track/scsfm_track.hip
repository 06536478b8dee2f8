// Frame-to-model tracking by point-to-plane ICP on the maps of the ray cast (include/scsfm_track.h): the six degrees of
// freedom of a pose.  The arithmetic it shares with the scaled tracker of csrc_sim3/ -- the state, the pair of a pixel, the
// sums, the steps of the solve -- and the kernels' design are ../csrc_icp/scsfm_icp.h; here are the kernels and what is the
// rigid tracker's own.
//
//  init_kernel        one lane per frame: the state and the fp32 record of the pose.
//  poses_kernel       one lane per frame: the state back into twelve doubles.
//  accumulate_kernel  the shared core's own kernel, at six degrees of freedom: the 29 sums of every 1024 pixels of every
//                     frame to the slab.
//  solve_kernel       one wave per frame: the slab's rows added, then lane 0 factorises the 6 x 6 system, judging every
//                     pivot against the largest diagonal entry, solves, updates the state and rewrites the record.
#pragma clang fp contract(off)
#include "scsfm_track.h"

#include "../csrc_icp/scsfm_icp.h"

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kDof = 6;
constexpr int kState = SCSFM_TRACK_STATE;
constexpr int kSums = kSumsOf<kDof>;
constexpr int kReport = SCSFM_TRACK_REPORT;
static_assert(kTile == SCSFM_TRACK_TILE && kRecord == SCSFM_TRACK_RECORD && kSums == SCSFM_TRACK_SUMS,
              "the header's sizes");

__global__ __launch_bounds__(kThreads) void init_kernel(int V, const double* __restrict__ c2w,
                                                        const float* __restrict__ K, double* __restrict__ state,
                                                        float* __restrict__ est) {
  const int v = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (v >= V) return;
  const double* m = c2w + 12 * (size_t)v;
  double q[4];
  quaternion_of_pose(m, q);
  double* s = state + kState * (size_t)v;
  s[0] = q[0], s[1] = q[1], s[2] = q[2], s[3] = q[3];
  s[4] = m[3], s[5] = m[7], s[6] = m[11];
  float* rec = est + kRecord * (size_t)v;
  write_record(s, rec);
  rec[12] = K[0], rec[13] = K[4], rec[14] = K[2], rec[15] = K[5];
}

__global__ __launch_bounds__(kThreads) void poses_kernel(int V, const double* __restrict__ state,
                                                         double* __restrict__ c2w) {
  const int v = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (v >= V) return;
  pose_of_state(state + kState * (size_t)v, c2w + 12 * (size_t)v);
}

__global__ __launch_bounds__(64) void solve_kernel(int n_groups, int min_pairs, int n_iters, int iter,
                                                   const double* __restrict__ ws, double* __restrict__ state,
                                                   float* __restrict__ est, double* __restrict__ report) {
  __shared__ double s_sum[kSums];
  const int tid = (int)threadIdx.x, v = (int)blockIdx.x;
  reduce_slab<kSums>(tid, ws, v, n_groups, s_sum);
  if (tid != 0) return;
  double Hm[kDof][kDof], L[kDof][kDof], D[kDof], x[kDof];
  unpack(s_sum, Hm);
  const double count = s_sum[kSums - 1];
  int status = 0;
  double ratio = 0.0;
  if (count < (double)min_pairs) {
    status = 1;
  } else {
    double top = Hm[0][0];
#pragma unroll
    for (int i = 1; i < kDof; ++i)
      if (Hm[i][i] > top) top = Hm[i][i];
    if (!(top > 0.0)) {
      status = 2;
    } else {
      const double floor_d = SCSFM_TRACK_PIVOT_EPS * top;
      // (after a pivot has failed the loop runs on, on values nobody reads: the header's factorisation has stopped)
#pragma unroll
      for (int j = 0; j < kDof; ++j) {
        const double d = D[j] = ldl_pivot(j, Hm, L, D);
        if (status == 0) {
          const double rj = d / top;
          if (j == 0 || rj < ratio) ratio = rj;
          if (!(d > floor_d)) status = 2;
        }
        ldl_column(j, d, Hm, L, D);
      }
      solve_lower(s_sum + kProductsOf<kDof>, L, D, x);
#pragma unroll
      for (int i = kDof - 1; i >= 0; --i) x[i] = back_row(i, L, x);
      if (status == 0) {
#pragma unroll
        for (int i = 0; i < kDof; ++i)
          if (x[i] - x[i] != 0.0) status = 2;
      }
    }
  }
  double* rep = report + ((size_t)v * n_iters + iter) * kReport;
  rep[0] = count, rep[1] = s_sum[kSums - 2], rep[2] = (double)status, rep[3] = ratio;
  if (status != 0) return;
  double* s = state + kState * (size_t)v;
  retract(x, s);
  write_record(s, est + kRecord * (size_t)v);
}

}  // namespace

extern "C" {

int scsfm_track_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_track_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

size_t scsfm_track_ws_bytes(int V, int H, int W) {
  const long long n = groups_of(V, H, W, kSums);
  if (!n) return 0;
  return (size_t)V * (size_t)n * kSums * sizeof(double);
}

int scsfm_track_init(int V, const double* c2w, const float* K, double* state, float* est, void* stream) {
  if (V <= 0 || V > INT_MAX / kRecord || bad(c2w, 8) || bad(K, 4) || bad(state, 8) || bad(est, 4))
    return SCSFM_TRACK_ERR_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(init_kernel, dim3((unsigned)((V + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, V, c2w, K, state, est);
  return (int)hipGetLastError();
}

int scsfm_track_poses(int V, const double* state, double* c2w, void* stream) {
  if (V <= 0 || V > INT_MAX / kRecord || bad(state, 8) || bad(c2w, 8)) return SCSFM_TRACK_ERR_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(poses_kernel, dim3((unsigned)((V + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, V, state, c2w);
  return (int)hipGetLastError();
}

int scsfm_track_iterate(int V, int H, int W, const float* depth, int is_disp, float near_d, float max_depth,
                        const float* ref, const float* model_depth, const float* model_normal, float max_dist,
                        int min_pairs, int n_iters, double* state, float* est, double* ws, double* report,
                        void* stream) {
  const long long n_groups = groups_of(V, H, W, kSums);
  if (!n_groups || n_iters < 1 || n_iters > SCSFM_TRACK_MAX_ITERS || min_pairs < kDof) return SCSFM_TRACK_ERR_ARG;
  if (!positive(max_dist) || !positive(max_depth) || !(near_d >= 0.0f) || !std::isfinite(near_d))
    return SCSFM_TRACK_ERR_ARG;
  if (bad(depth, 4) || bad(ref, 4) || bad(model_depth, 4) || bad(model_normal, 4) || bad(state, 8) || bad(est, 4) ||
      bad(ws, 8) || bad(report, 8))
    return SCSFM_TRACK_ERR_ARG;
  const Frame fr = {V, H, W, (int)n_groups, is_disp != 0, near_d, max_depth, max_dist};
  (void)hipGetLastError();
  for (int it = 0; it < n_iters; ++it) {
    hipLaunchKernelGGL((accumulate_kernel<kDof>), dim3((unsigned)(n_groups * V)), dim3(kThreads), 0,
                       (hipStream_t)stream, fr, depth, est, ref, model_depth, model_normal, ws);
    hipLaunchKernelGGL(solve_kernel, dim3((unsigned)V), dim3(64), 0, (hipStream_t)stream, (int)n_groups, min_pairs,
                       n_iters, it, (const double*)ws, state, est, report);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  return 0;
}

}  // extern "C"
