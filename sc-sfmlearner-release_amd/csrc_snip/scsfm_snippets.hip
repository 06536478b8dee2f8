// The 5-frame snippet protocol of test_pose.py with kitti_eval/pose_evaluation_utils.py (include/scsfm_snip.h): ATE and
// RE of every snippet of a ragged set of sequences, and their mean and std, in three launches.
//
//  invert    one lane per pair vector: pose_vec2mat in the input precision, lifted to double, inverted into the
//            workspace.  Adjacent snippets share all but one of their pairs, so each inverse is formed once.
//  snippet   one lane per snippet, in four short walks over its frames so that no walk holds more than three 3x3
//            matrices (one walk for everything needs 164 vector registers): the sequential fold P_i = P_{i-1} inv(T)
//            into `pred`; the rotations (the ground truth's compensated by its first frame, the residual angle
//            against the fold's, read back from the lane's own rows of `pred`); the two sums of the scale factor; the
//            ATE residual, which needs the scale factor and forms the ground truth's translations again, by the same
//            operations on the same operands (2 x 16 x 3 doubles are not worth the registers).
//  stats     one workgroup: mean and population std of the errors rounded to float, accumulated in double.
//
// Determinism: no float atomics.  A snippet's numbers depend only on its own frames; the statistics are reduced
// thread-strided, then by a wave's shuffle tree, then over the waves in order, which depends only on n_snip.
// Exactness: contraction is off below the rotations, so products, inverses and error terms round as the numpy
// statements of the header do; the rotations above the pragma are compiled as csrc/scsfm_geom.h's, whose closed forms
// they repeat.
#include <hip/hip_runtime.h>

#include <math.h>

#include "scsfm_snip.h"

namespace {  // (internal linkage: the library exports exactly the header's symbols)

__device__ inline void sincos_t(float x, float* s, float* c) { *s = sinf(x); *c = cosf(x); }
__device__ inline void sincos_t(double x, double* s, double* c) { *s = sin(x); *c = cos(x); }
__device__ inline float sqrt_t(float x) { return sqrtf(x); }
__device__ inline double sqrt_t(double x) { return sqrt(x); }

// R = Rx(rx) Ry(ry) Rz(rz) in closed form, row-major (csrc/scsfm_geom.h: euler_to_R)
template <class T>
__device__ inline void euler_to_R(T rx, T ry, T rz, T* r) {
  T sx, cx, sy, cy, sz, cz;
  sincos_t(rx, &sx, &cx);
  sincos_t(ry, &sy, &cy);
  sincos_t(rz, &sz, &cz);
  r[0] = cy * cz;                 r[1] = -cy * sz;                r[2] = sy;
  r[3] = cx * sz + sx * sy * cz;  r[4] = cx * cz - sx * sy * sz;  r[5] = -sx * cy;
  r[6] = sx * sz - cx * sy * cz;  r[7] = sx * cz + cx * sy * sz;  r[8] = cx * cy;
}

// q = (1, x, y, z) / |(1, x, y, z)| (csrc/scsfm_geom.h: quat_to_R)
template <class T>
__device__ inline void quat_to_R(T qx, T qy, T qz, T* r) {
  T n = sqrt_t(T(1) + qx * qx + qy * qy + qz * qz);
  T w = T(1) / n, x = qx / n, y = qy / n, z = qz / n;
  r[0] = w * w + x * x - y * y - z * z;  r[1] = 2 * x * y - 2 * w * z;          r[2] = 2 * w * y + 2 * x * z;
  r[3] = 2 * w * z + 2 * x * y;          r[4] = w * w - x * x + y * y - z * z;  r[5] = 2 * y * z - 2 * w * x;
  r[6] = 2 * x * z - 2 * w * y;          r[7] = 2 * w * x + 2 * y * z;          r[8] = w * w - x * x - y * y + z * z;
}

#pragma clang fp contract(off)

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;

// ---- affine maps ----

struct Aff {
  double a[9], t[3];
};

__device__ inline Aff identity() {
  Aff x;
#pragma unroll
  for (int i = 0; i < 9; ++i) x.a[i] = (i % 4 == 0) ? 1.0 : 0.0;
  x.t[0] = x.t[1] = x.t[2] = 0.0;
  return x;
}

__device__ inline Aff load(const double* __restrict__ p) {
  Aff x;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    x.a[3 * i] = p[4 * i], x.a[3 * i + 1] = p[4 * i + 1], x.a[3 * i + 2] = p[4 * i + 2], x.t[i] = p[4 * i + 3];
  }
  return x;
}

__device__ inline void store(double* __restrict__ p, const Aff& x) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    p[4 * i] = x.a[3 * i], p[4 * i + 1] = x.a[3 * i + 1], p[4 * i + 2] = x.a[3 * i + 2], p[4 * i + 3] = x.t[i];
  }
}

// x y: first y, then x
__device__ inline Aff mul(const Aff& x, const Aff& y) {
  Aff z;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      z.a[3 * i + j] = (x.a[3 * i] * y.a[j] + x.a[3 * i + 1] * y.a[3 + j]) + x.a[3 * i + 2] * y.a[6 + j];
    z.t[i] = ((x.a[3 * i] * y.t[0] + x.a[3 * i + 1] * y.t[1]) + x.a[3 * i + 2] * y.t[2]) + x.t[i];
  }
  return z;
}

// the general inverse of a 3x3: adjugate / determinant
__device__ inline void inverse3(const double* __restrict__ a, double* __restrict__ z) {
  const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
  const double det = (a[0] * c0 + a[1] * c1) + a[2] * c2;
  z[0] = c0 / det;
  z[3] = c1 / det;
  z[6] = c2 / det;
  z[1] = (a[2] * a[7] - a[1] * a[8]) / det;
  z[4] = (a[0] * a[8] - a[2] * a[6]) / det;
  z[7] = (a[1] * a[6] - a[0] * a[7]) / det;
  z[2] = (a[1] * a[5] - a[2] * a[4]) / det;
  z[5] = (a[2] * a[3] - a[0] * a[5]) / det;
  z[8] = (a[0] * a[4] - a[1] * a[3]) / det;
}

// A v, each row summed left to right
__device__ inline void matvec(const double* __restrict__ a, const double* __restrict__ v, double* __restrict__ z) {
#pragma unroll
  for (int i = 0; i < 3; ++i) z[i] = (a[3 * i] * v[0] + a[3 * i + 1] * v[1]) + a[3 * i + 2] * v[2];
}

// A B for 3x3 matrices
__device__ inline void matmul3(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ z) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) z[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
  }
}

// inv(A, t) = (A^-1, -(A^-1 t))
__device__ inline Aff inverse(const Aff& x) {
  Aff z;
  inverse3(x.a, z.a);
  matvec(z.a, x.t, z.t);
#pragma unroll
  for (int i = 0; i < 3; ++i) z.t[i] = -z.t[i];
  return z;
}

// ---- workgroup reduction (fixed order: a wave's shuffle tree, then the waves in order) ----

__device__ inline double block_sum(double v, double* red) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d);
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  double s = red[0];
  for (int k = 1; k < kWaves; ++k) s += red[k];
  return s;
}

// ---- the kernels ----

template <class T>
__global__ __launch_bounds__(kThreads) void invert_kernel(long long total, int quat, const T* __restrict__ vec,
                                                          double* __restrict__ tinv) {
  const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (k >= total) return;
  const T* p = vec + 6 * k;
  T R[9];
  if (quat) quat_to_R(p[3], p[4], p[5], R); else euler_to_R(p[3], p[4], p[5], R);
  Aff m;
#pragma unroll
  for (int i = 0; i < 9; ++i) m.a[i] = (double)R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) m.t[i] = (double)p[i];
  store(tinv + 12 * k, inverse(m));
}

// the translation of frame f of the compensated ground truth: R0^-1 (t_f - t_0)
__device__ inline void comp_translation(const double* __restrict__ row, const double* __restrict__ r0inv,
                                        const double* __restrict__ t0, double* __restrict__ z) {
  const double d[3] = {row[3] - t0[0], row[7] - t0[1], row[11] - t0[2]};
  matvec(r0inv, d, z);
}

// (four waves per SIMD: without the bound the compiler takes 148 vector registers; with it 126 and still no scratch)
__global__ __launch_bounds__(kThreads, 4) void snippet_kernel(int S, int L, long long total, long long n_snip,
                                                           const double* __restrict__ tinv,
                                                           const double* __restrict__ gt,
                                                           const int* __restrict__ frame_off,
                                                           const int* __restrict__ len,
                                                           const int* __restrict__ snip_off, double* pred,
                                                           double* __restrict__ gt_comp, double* __restrict__ errors) {
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= n_snip) return;
  // the last sequence whose first snippet number is <= g (a sequence without a snippet shares its number with the next)
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (snip_off[mid] <= g) lo = mid; else hi = mid - 1;
  }
  const long long j = g - snip_off[lo], n = len[lo], base = frame_off[lo];
  if (j < 0 || j + L > n || base < 0 || base + n > total) {  // (tables that disagree with n_snip: see the header)
    errors[2 * g] = errors[2 * g + 1] = NAN;
    return;
  }
  const double* grow = gt + 12 * (base + j);
  const double* trow = tinv + 12 * (base + j);
  double* prow = pred + 12 * L * g;
  double* crow = gt_comp ? gt_comp + 12 * L * g : nullptr;

  double r0inv[9], t0[3];
  {
    const Aff g0 = load(grow);
    inverse3(g0.a, r0inv);
    t0[0] = g0.t[0], t0[1] = g0.t[1], t0[2] = g0.t[2];
  }
  // 1. the fold
  {
    Aff P = identity();
    store(prow, P);
#pragma unroll 1
    for (int i = 1; i < L; ++i) {
      P = mul(P, load(trow + 12 * (i - 1)));
      store(prow + 12 * i, P);
    }
  }
  // 2. rotations: the compensated ground truth's, and the residual angle against the fold's
  double re = 0.0;
#pragma unroll 1
  for (int i = 0; i < L; ++i) {
    double ga[9], pinv[9], R[9];
    {
      const double* x = grow + 12 * i;
      const double xa[9] = {x[0], x[1], x[2], x[4], x[5], x[6], x[8], x[9], x[10]};
      matmul3(r0inv, xa, ga);
    }
    if (crow) {
      double* o = crow + 12 * i;
#pragma unroll
      for (int r = 0; r < 3; ++r) o[4 * r] = ga[3 * r], o[4 * r + 1] = ga[3 * r + 1], o[4 * r + 2] = ga[3 * r + 2];
    }
    {
      const double* x = prow + 12 * i;
      const double xa[9] = {x[0], x[1], x[2], x[4], x[5], x[6], x[8], x[9], x[10]};
      inverse3(xa, pinv);
    }
    matmul3(ga, pinv, R);
    const double d0 = R[1] - R[3], d1 = R[5] - R[7], d2 = R[2] - R[6];
    const double s = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    const double c = ((R[0] + R[4]) + R[8]) - 1.0;
    re += atan2(s, c);
  }
  // 3. translations: the scale factor's two sums
  double sgp = 0.0, spp = 0.0;
#pragma unroll 1
  for (int i = 0; i < L; ++i) {
    double gtr[3];
    comp_translation(grow + 12 * i, r0inv, t0, gtr);
    if (crow) crow[12 * i + 3] = gtr[0], crow[12 * i + 7] = gtr[1], crow[12 * i + 11] = gtr[2];
    const double* pt = prow + 12 * i;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      sgp += gtr[k] * pt[4 * k + 3];
      spp += pt[4 * k + 3] * pt[4 * k + 3];
    }
  }
  const double scale = sgp / spp;
  // 4. the residual (the ground truth's translations formed again, by the same operations on the same operands)
  double sq = 0.0;
#pragma unroll 1
  for (int i = 0; i < L; ++i) {
    double gtr[3];
    comp_translation(grow + 12 * i, r0inv, t0, gtr);
    const double* pt = prow + 12 * i;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double e = gtr[k] - scale * pt[4 * k + 3];
      sq += e * e;
    }
  }
  errors[2 * g] = sqrt(sq) / (double)L;
  errors[2 * g + 1] = re / (double)L;
}

__global__ __launch_bounds__(kThreads) void stats_kernel(long long n_snip, const double* __restrict__ errors,
                                                         double* __restrict__ stats) {
  __shared__ double red[kWaves];
  const double n = (double)n_snip;
  for (int c = 0; c < 2; ++c) {  // 0: ATE, 1: RE
    double v = 0.0;
    for (long long i = threadIdx.x; i < n_snip; i += kThreads) v += (double)(float)errors[2 * i + c];
    const double mean = block_sum(v, red) / n;
    v = 0.0;
    for (long long i = threadIdx.x; i < n_snip; i += kThreads) {
      const double d = (double)(float)errors[2 * i + c] - mean;
      v += d * d;
    }
    const double var = block_sum(v, red) / n;
    if (threadIdx.x == 0) {
      stats[c] = mean;
      stats[2 + c] = sqrt(var);
    }
  }
}

inline int ceil_div(long long a, int b) { return (int)((a + b - 1) / b); }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int launch_status() { return (int)hipGetLastError(); }
constexpr size_t kMaxFrames = (size_t)1 << 30;
constexpr int kMaxSeq = 1 << 16;

// bytes of the workspace (the inverted pair matrices), 0 for a rejected argument
inline size_t layout(int S, int seq_len, size_t total_frames) {
  if (S <= 0 || S > kMaxSeq || seq_len < SCSFM_SNIP_MIN_LEN || seq_len > SCSFM_SNIP_MAX_LEN || total_frames == 0 ||
      total_frames >= kMaxFrames)
    return 0;
  return align256(total_frames * 12 * sizeof(double));
}

}  // namespace

extern "C" {

int scsfm_snip_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_snip_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

size_t scsfm_snip_workspace_bytes(int S, int seq_len, size_t total_frames) { return layout(S, seq_len, total_frames); }

int scsfm_snip_eval(int S, int seq_len, int vec_f64, int rot_mode, const void* vec, const double* gt,
                    const int* frame_off, const int* len, const int* snip_off, size_t total_frames, size_t n_snip,
                    double* pred, double* gt_comp, double* errors, double* stats, void* workspace,
                    size_t workspace_bytes, void* stream) {
  const size_t need = layout(S, seq_len, total_frames);
  if (need == 0 || (rot_mode != SCSFM_SNIP_ROT_EULER && rot_mode != SCSFM_SNIP_ROT_QUAT) || !vec || !gt ||
      !frame_off || !len || !snip_off || n_snip < 1 || n_snip > total_frames || !pred || !errors || !stats ||
      !workspace || workspace_bytes < need)
    return SCSFM_SNIP_ERR_ARG;
  double* tinv = static_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  const long long total = (long long)total_frames, ns = (long long)n_snip;
  (void)hipGetLastError();
  if (vec_f64)
    hipLaunchKernelGGL(invert_kernel<double>, dim3(ceil_div(total, kThreads)), dim3(kThreads), 0, s, total, rot_mode,
                       static_cast<const double*>(vec), tinv);
  else
    hipLaunchKernelGGL(invert_kernel<float>, dim3(ceil_div(total, kThreads)), dim3(kThreads), 0, s, total, rot_mode,
                       static_cast<const float*>(vec), tinv);
  hipLaunchKernelGGL(snippet_kernel, dim3(ceil_div(ns, kThreads)), dim3(kThreads), 0, s, S, seq_len, total, ns, tinv,
                     gt, frame_off, len, snip_off, pred, gt_comp, errors);
  hipLaunchKernelGGL(stats_kernel, dim3(1), dim3(kThreads), 0, s, ns, errors, stats);
  return launch_status();
}

}  // extern "C"
