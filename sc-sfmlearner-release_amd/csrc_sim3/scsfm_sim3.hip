// Frame-to-model tracking with a scale: point-to-plane ICP over seven degrees of freedom on the maps of the ray cast
// (include/scsfm_sim3.h).  The arithmetic it shares with the rigid tracker of csrc_track/ -- the state, the pair of a
// pixel, the sums, the steps of the solve -- and the kernels' design are ../csrc_icp/scsfm_icp.h; here are the kernels and
// what is the scale's own.
//
//  init_kernel        one lane per frame: the state, the fp32 record of the pose and the fp32 scale.
//  poses_kernel       one lane per frame: the state back into twelve doubles and the scale.
//  accumulate_kernel  the shared core's own kernel, at seven degrees of freedom: the 37 sums of every 1024 pixels of every
//                     frame to the slab.
//  solve_kernel       one wave per frame: the slab's rows added, then lane 0 factorises the 7 x 7 system with the scale
//                     last, judging the pose's six pivots as the rigid tracker does, decides from the last pivot whether
//                     the scale is solved or held, solves, updates the state and rewrites the record and the fp32 scale.
//  scale_kernel       streaming: a thread four consecutive floats of the frames, as one 16-byte load and store where the
//                     pointers allow it; the frame of an element is its index over H W.
#pragma clang fp contract(off)
#include "scsfm_sim3.h"

#include "../csrc_icp/scsfm_icp.h"

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kDof = 7;
constexpr int kState = SCSFM_SIM3_STATE;
constexpr int kSums = kSumsOf<kDof>;
constexpr int kReport = SCSFM_SIM3_REPORT;
static_assert(kTile == SCSFM_SIM3_TILE && kRecord == SCSFM_SIM3_RECORD && kSums == SCSFM_SIM3_SUMS,
              "the header's sizes");

__global__ __launch_bounds__(kThreads) void init_kernel(int V, const double* __restrict__ c2w,
                                                        const double* __restrict__ scale0, const float* __restrict__ K,
                                                        double* __restrict__ state, float* __restrict__ est,
                                                        float* __restrict__ sigma_f) {
  const int v = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (v >= V) return;
  const double* m = c2w + 12 * (size_t)v;
  double q[4];
  quaternion_of_pose(m, q);
  double* s = state + kState * (size_t)v;
  s[0] = q[0], s[1] = q[1], s[2] = q[2], s[3] = q[3];
  s[4] = m[3], s[5] = m[7], s[6] = m[11];
  const double sigma = scale0[v];
  s[7] = sigma;
  sigma_f[v] = (float)sigma;
  float* rec = est + kRecord * (size_t)v;
  write_record(s, rec);
  rec[12] = K[0], rec[13] = K[4], rec[14] = K[2], rec[15] = K[5];
}

__global__ __launch_bounds__(kThreads) void poses_kernel(int V, const double* __restrict__ state,
                                                         double* __restrict__ c2w, double* __restrict__ scale) {
  const int v = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (v >= V) return;
  const double* s = state + kState * (size_t)v;
  pose_of_state(s, c2w + 12 * (size_t)v);
  scale[v] = s[7];
}

__global__ __launch_bounds__(64) void solve_kernel(int n_groups, int min_pairs, double min_scale_pivot, int n_iters,
                                                   int iter, const double* __restrict__ ws, double* __restrict__ state,
                                                   float* __restrict__ est, float* __restrict__ sigma_f,
                                                   double* __restrict__ report) {
  __shared__ double s_sum[kSums];
  const int tid = (int)threadIdx.x, v = (int)blockIdx.x;
  reduce_slab<kSums>(tid, ws, v, n_groups, s_sum);
  if (tid != 0) return;
  double Hm[kDof][kDof], L[kDof][kDof], D[kDof], x[kDof];
  unpack(s_sum, Hm);
  double* s = state + kState * (size_t)v;
  const double count = s_sum[kSums - 1], sigma = s[7];
  int status = 0;
  bool held = false;
  double ratio = 0.0, ratio6 = 0.0;
  if (!(sigma > 0.0 && sigma - sigma == 0.0)) {
    status = 2;
  } else if (count < (double)min_pairs) {
    status = 1;
  } else {
    double top6 = Hm[0][0];
#pragma unroll
    for (int i = 1; i < 6; ++i)
      if (Hm[i][i] > top6) top6 = Hm[i][i];
    if (!(top6 > 0.0)) {
      status = 2;
    } else {
      const double top = Hm[6][6] > top6 ? Hm[6][6] : top6;
      const double floor_d = SCSFM_SIM3_PIVOT_EPS * top6;
      // (after a pivot has failed the loop runs on, on values nobody reads: the header's factorisation has stopped)
#pragma unroll
      for (int j = 0; j < kDof; ++j) {
        const double d = D[j] = ldl_pivot(j, Hm, L, D);
        if (j < 6) {
          if (status == 0) {
            const double rj = d / top6;
            if (j == 0 || rj < ratio) ratio = rj;
            if (!(d > floor_d)) status = 2;
          }
        } else if (status == 0) {
          ratio6 = d / top;
          const double need = min_scale_pivot * top;
          held = !(d > need);
        }
        ldl_column(j, d, Hm, L, D);
      }
      solve_lower(s_sum + kProductsOf<kDof>, L, D, x);
      if (!(x[6] > -1.0 && x[6] < 1.0)) held = true;
      if (held) x[6] = 0.0;
#pragma unroll
      for (int i = 5; i >= 0; --i) {
        double y = back_row(i, L, x);
        if (!held) {  // (a held scale's term is not formed: y - (-0.0) would turn a y of -0.0 into +0.0)
          const double t = L[6][i] * x[6];
          y = y - t;
        }
        x[i] = y;
      }
      if (status == 0) {
#pragma unroll
        for (int i = 0; i < kDof; ++i)
          if (x[i] - x[i] != 0.0) status = 2;
        if (status == 0 && held) status = 3;
      }
    }
  }
  double* rep = report + ((size_t)v * n_iters + iter) * kReport;
  rep[0] = count, rep[1] = s_sum[kSums - 2], rep[2] = (double)status, rep[3] = ratio;
  rep[4] = ratio6, rep[5] = sigma;
  if (status != 0 && status != 3) return;
  retract(x, s);
  write_record(s, est + kRecord * (size_t)v);
  if (status == 0) {
    const double h = 0.5 * x[6];
    const double up = 1.0 + h, down = 1.0 - h;
    double next = sigma * up;
    next = next / down;
    s[7] = next;
    sigma_f[v] = (float)next;
  }
}

// ---- the scaled depth ----

__device__ inline float scaled(float d, int is_disp, float sigma) {
  if (is_disp) d = 1.0f / d;
  return sigma * d;
}

__global__ __launch_bounds__(kThreads) void scale_kernel(int n, int hw, int is_disp, int vec,
                                                         const float* __restrict__ depth,
                                                         const float* __restrict__ sigma_f, float* __restrict__ out) {
  const long long at = 4LL * ((long long)blockIdx.x * kThreads + threadIdx.x);
  if (at >= n) return;
  const int i = (int)at;
  if (vec && i <= n - 4) {  // (both pointers are aligned to 16 bytes, and so is every fourth element)
    const float4 d = *reinterpret_cast<const float4*>(depth + i);
    float4 o;
    o.x = scaled(d.x, is_disp, sigma_f[i / hw]);
    o.y = scaled(d.y, is_disp, sigma_f[(i + 1) / hw]);
    o.z = scaled(d.z, is_disp, sigma_f[(i + 2) / hw]);
    o.w = scaled(d.w, is_disp, sigma_f[(i + 3) / hw]);
    *reinterpret_cast<float4*>(out + i) = o;
    return;
  }
  for (int k = i; k < n && k < i + 4; ++k) out[k] = scaled(depth[k], is_disp, sigma_f[k / hw]);
}

}  // namespace

extern "C" {

int scsfm_sim3_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_sim3_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

size_t scsfm_sim3_ws_bytes(int V, int H, int W) {
  const long long n = groups_of(V, H, W, kSums);
  if (!n) return 0;
  return (size_t)V * (size_t)n * kSums * sizeof(double);
}

int scsfm_sim3_init(int V, const double* c2w, const double* scale0, const float* K, double* state, float* est,
                    float* sigma_f, void* stream) {
  if (V <= 0 || V > INT_MAX / kRecord || bad(c2w, 8) || bad(scale0, 8) || bad(K, 4) || bad(state, 8) || bad(est, 4) ||
      bad(sigma_f, 4))
    return SCSFM_SIM3_ERR_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(init_kernel, dim3((unsigned)((V + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, V, c2w, scale0, K, state, est, sigma_f);
  return (int)hipGetLastError();
}

int scsfm_sim3_poses(int V, const double* state, double* c2w, double* scale, void* stream) {
  if (V <= 0 || V > INT_MAX / kRecord || bad(state, 8) || bad(c2w, 8) || bad(scale, 8)) return SCSFM_SIM3_ERR_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(poses_kernel, dim3((unsigned)((V + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, V, state, c2w, scale);
  return (int)hipGetLastError();
}

int scsfm_sim3_iterate(int V, int H, int W, const float* depth, int is_disp, float near_d, float max_depth,
                       const float* ref, const float* model_depth, const float* model_normal, float max_dist,
                       int min_pairs, double min_scale_pivot, int n_iters, double* state, float* est, float* sigma_f,
                       double* ws, double* report, void* stream) {
  const long long n_groups = groups_of(V, H, W, kSums);
  if (!n_groups || n_iters < 1 || n_iters > SCSFM_SIM3_MAX_ITERS || min_pairs < kDof) return SCSFM_SIM3_ERR_ARG;
  if (!positive(max_dist) || !positive(max_depth) || !(near_d >= 0.0f) || !std::isfinite(near_d) ||
      !(min_scale_pivot > 0.0))
    return SCSFM_SIM3_ERR_ARG;
  if (bad(depth, 4) || bad(ref, 4) || bad(model_depth, 4) || bad(model_normal, 4) || bad(state, 8) || bad(est, 4) ||
      bad(sigma_f, 4) || bad(ws, 8) || bad(report, 8))
    return SCSFM_SIM3_ERR_ARG;
  const Frame fr = {V, H, W, (int)n_groups, is_disp != 0, near_d, max_depth, max_dist};
  (void)hipGetLastError();
  for (int it = 0; it < n_iters; ++it) {
    hipLaunchKernelGGL((accumulate_kernel<kDof, const float* __restrict__>), dim3((unsigned)(n_groups * V)),
                       dim3(kThreads), 0, (hipStream_t)stream, fr, depth, (const float*)sigma_f, (const float*)est, ref,
                       model_depth, model_normal, ws);
    hipLaunchKernelGGL(solve_kernel, dim3((unsigned)V), dim3(64), 0, (hipStream_t)stream, (int)n_groups, min_pairs,
                       min_scale_pivot, n_iters, it, (const double*)ws, state, est, sigma_f, report);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  return 0;
}

int scsfm_sim3_scale(int V, int H, int W, const float* depth, int is_disp, const float* sigma_f, float* out,
                     void* stream) {
  if (V <= 0 || H <= 0 || W <= 0) return SCSFM_SIM3_ERR_ARG;
  const long long hw = (long long)H * W, n = hw * V;
  if (hw > INT_MAX || n > INT_MAX - 4 * kThreads) return SCSFM_SIM3_ERR_ARG;
  if (bad(depth, 4) || bad(sigma_f, 4) || bad(out, 4)) return SCSFM_SIM3_ERR_ARG;
  const int vec = !misaligned(depth, 16) && !misaligned(out, 16);
  const long long quads = (n + 3) / 4;
  (void)hipGetLastError();
  hipLaunchKernelGGL(scale_kernel, dim3((unsigned)((quads + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, (int)n, (int)hw, is_disp != 0, vec, depth, sigma_f, out);
  return (int)hipGetLastError();
}

}  // extern "C"
