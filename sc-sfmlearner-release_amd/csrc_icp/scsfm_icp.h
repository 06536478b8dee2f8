// The point-to-plane ICP core of the two frame-to-model trackers: csrc_track/ (six degrees of freedom,
// include/scsfm_track.h) and csrc_sim3/ (seven, the scale of the frame's own depth last, include/scsfm_sim3.h).  Both
// include this file by its relative path and both source ids cover it (scsfm_hip/build.py); it belongs to neither library
// and includes nothing of the project's.  kDof is 6 or 7 throughout, kSums = kDof (kDof + 1) / 2 + kDof + 2 (29 or 37):
// the upper triangle of J J^T, J r, r r and the number of pairs.
//
//  the state      Shepperd's quaternion of a pose, the matrix of a quaternion, the fp32 record of a state and the state
//                 back into twelve doubles: one lane per frame in the libraries' init and poses kernels.
//  accumulate     one workgroup (256 threads) per 1024 consecutive pixels of one frame, a thread four of them at a stride
//                 of 256, so that a wave reads 64 consecutive depths and its gathers of the model maps land on neighbouring
//                 pixels.  The kSums double accumulators (58 or 74 VGPRs) are paid once for four pixels.  The estimate's
//                 record, the reference record and the frame's scale are the same addresses in every lane (uniform loads).
//                 The sums meet through six butterfly steps inside a wave, then through LDS across the four waves; every
//                 workgroup stores its kSums values to the slab: no atomics, no clearing.
//  the solve      one wave per frame: lanes 0 .. kSums - 1 add the frame's slab rows in index order (the launch-boundary
//                 reduce: the kernel boundary is the grid-wide barrier); lane 0 then factorises H = L D L^T column by
//                 column, solves and retracts the pose.  Which pivots are judged against what, and what a failed one
//                 means, is each library's own solve_kernel.
//
// A pixel that is no pair adds +0.0 to every sum, which changes no bit: a sum that starts at +0.0 never becomes -0.0
// (x + y is -0.0 only when both are), and s + (+0.0) == s for every other s.  So the four pixels of a thread need no
// divergent accumulation.
//
// Arithmetic: the headers' order, one rounding per operation, in fp32 and in double.  The pragma keeps the compiler from
// contracting a multiply and an add (hipcc's default is -ffp-contract=fast); `/` and sqrt are the correctly rounded
// expansions and fp32 denormals are kept on gfx950.
#pragma once
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

namespace {  // (internal linkage: a library exports exactly its header's symbols)

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerThread = 4;
constexpr int kTile = kThreads * kPerThread;  // a thread takes kPerThread pixels of the tile
constexpr int kRecord = 16;

template <int kDof>
constexpr int kProductsOf = kDof * (kDof + 1) / 2;  // the upper triangle of J J^T
template <int kDof>
constexpr int kSumsOf = kProductsOf<kDof> + kDof + 2;  // J_i J_j, J_i r, r r, 1

// ---- the state: a unit quaternion (w, x, y, z), the centre, and whatever a library keeps behind them ----

__device__ inline void normalise(double q[4]) {
  double len = q[0] * q[0];
  double p = q[1] * q[1];
  len = len + p;
  p = q[2] * q[2];
  len = len + p;
  p = q[3] * q[3];
  len = len + p;
  len = sqrt(len);
  q[0] = q[0] / len, q[1] = q[1] / len, q[2] = q[2] / len, q[3] = q[3] / len;
}

// the headers' matrix of a quaternion, row-major
__device__ inline void matrix(const double q[4], double R[9]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  R[0] = 1.0 - 2.0 * (yy + zz), R[1] = 2.0 * (xy - wz), R[2] = 2.0 * (xz + wy);
  R[3] = 2.0 * (xy + wz), R[4] = 1.0 - 2.0 * (xx + zz), R[5] = 2.0 * (yz - wx);
  R[6] = 2.0 * (xz - wy), R[7] = 2.0 * (yz + wx), R[8] = 1.0 - 2.0 * (xx + yy);
}

// the first twelve floats of the record of a state
__device__ inline void write_record(const double* s, float* rec) {
  double R[9];
  matrix(s, R);
#pragma unroll
  for (int i = 0; i < 9; ++i) rec[i] = (float)R[i];
  rec[9] = (float)s[4], rec[10] = (float)s[5], rec[11] = (float)s[6];
}

// Shepperd's unit quaternion of the rotation of a pose m (3 x 4, camera to world)
__device__ __forceinline__ void quaternion_of_pose(const double* m, double q[4]) {
  const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[4], m11 = m[5], m12 = m[6], m20 = m[8], m21 = m[9], m22 = m[10];
  const double tr = (m00 + m11) + m22;
  double r, f;
  if (tr >= m00 && tr >= m11 && tr >= m22) {
    r = sqrt(1.0 + tr), f = 0.5 / r;
    q[0] = r / 2.0, q[1] = (m21 - m12) * f, q[2] = (m02 - m20) * f, q[3] = (m10 - m01) * f;
  } else if (m00 >= m11 && m00 >= m22) {
    r = sqrt(((1.0 + m00) - m11) - m22), f = 0.5 / r;
    q[1] = r / 2.0, q[0] = (m21 - m12) * f, q[2] = (m01 + m10) * f, q[3] = (m02 + m20) * f;
  } else if (m11 >= m22) {
    r = sqrt(((1.0 + m11) - m00) - m22), f = 0.5 / r;
    q[2] = r / 2.0, q[0] = (m02 - m20) * f, q[1] = (m01 + m10) * f, q[3] = (m12 + m21) * f;
  } else {
    r = sqrt(((1.0 + m22) - m00) - m11), f = 0.5 / r;
    q[3] = r / 2.0, q[0] = (m10 - m01) * f, q[1] = (m02 + m20) * f, q[2] = (m12 + m21) * f;
  }
  normalise(q);
}

// the pose of a state as twelve doubles (3 x 4, camera to world)
__device__ __forceinline__ void pose_of_state(const double* s, double* o) {
  double R[9];
  matrix(s, R);
#pragma unroll
  for (int i = 0; i < 3; ++i) o[4 * i] = R[3 * i], o[4 * i + 1] = R[3 * i + 1], o[4 * i + 2] = R[3 * i + 2], o[4 * i + 3] = s[4 + i];
}

// ---- the sums ----

struct Frame {
  int V, H, W, n_groups, is_disp;
  float near_d, max_depth, max_dist;
};

__device__ inline float dot3(float a0, float b0, float a1, float b1, float a2, float b2) {
  float s = a0 * b0;
  float p = a1 * b1;
  s = s + p;
  p = a2 * b2;
  return s + p;
}

// the pair of pixel (px, py): true and (J, r) for a pair.  With kScaled the depth enters as sigma times the frame's own
// and J has the scale's seventh entry; without, neither is formed and sigma is not read.
template <bool kScaled>
__device__ inline bool pair_of(const Frame& fr, int v, int px, int py, float d, float sigma, const float* __restrict__ a,
                               const float* __restrict__ b, const float* __restrict__ M, const float* __restrict__ N,
                               float* J, float& r) {
  if (fr.is_disp) d = 1.0f / d;
  if constexpr (kScaled) d = sigma * d;
  if (!(d > fr.near_d && d <= fr.max_depth)) return false;
  float dx = (float)px - a[14], dy = (float)py - a[15];
  dx = dx / a[12];
  dy = dy / a[13];
  const float q0 = dx * d, q1 = dy * d;
  float u[3], p[3], e[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    u[i] = dot3(a[3 * i], q0, a[3 * i + 1], q1, a[3 * i + 2], d);
    p[i] = a[9 + i] + u[i];
    e[i] = p[i] - b[9 + i];
  }
  const float xc = dot3(b[0], e[0], b[3], e[1], b[6], e[2]);
  const float yc = dot3(b[1], e[0], b[4], e[1], b[7], e[2]);
  const float zc = dot3(b[2], e[0], b[5], e[1], b[8], e[2]);
  if (!(zc > fr.near_d && zc > 0.0f)) return false;
  float ia = b[12] * xc, ib = b[13] * yc;
  ia = ia / zc, ib = ib / zc;
  ia = ia + b[14], ib = ib + b[15];
  ia = ia + 0.5f, ib = ib + 0.5f;
  // on the floats, before any conversion: a NaN or a huge value fails and converts nothing
  if (!(ia >= 0.0f && ia < (float)fr.W && ib >= 0.0f && ib < (float)fr.H)) return false;
  const int mx = (int)ia, my = (int)ib;
  const size_t hw = (size_t)fr.H * fr.W;
  const size_t at = (size_t)my * fr.W + mx;
  const float s = M[(size_t)v * hw + at];
  if (!(s > 0.0f)) return false;
  const float* __restrict__ np = N + (size_t)v * 3 * hw + at;
  const float n0 = np[0], n1 = np[hw], n2 = np[2 * hw];
  if (!(dot3(n0, n0, n1, n1, n2, n2) > 0.0f)) return false;
  float rx = (float)mx - b[14], ry = (float)my - b[15];
  rx = rx / b[12];
  ry = ry / b[13];
  float delta[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float w = b[3 * i] * rx;
    const float t = b[3 * i + 1] * ry;
    w = w + t;
    w = w + b[3 * i + 2];
    w = s * w;
    const float m = b[9 + i] + w;
    delta[i] = p[i] - m;
  }
  const float md2 = fr.max_dist * fr.max_dist;
  if (!(dot3(delta[0], delta[0], delta[1], delta[1], delta[2], delta[2]) <= md2)) return false;
  const float nu = dot3(n0, u[0], n1, u[1], n2, u[2]);
  if (!(nu < 0.0f)) return false;
  r = dot3(n0, delta[0], n1, delta[1], n2, delta[2]);
  J[0] = n0, J[1] = n1, J[2] = n2;
  float s0 = u[1] * n2, s1 = u[2] * n1;
  J[3] = s0 - s1;
  s0 = u[2] * n0, s1 = u[0] * n2;
  J[4] = s0 - s1;
  s0 = u[0] * n1, s1 = u[1] * n0;
  J[5] = s0 - s1;
  if constexpr (kScaled) J[6] = nu;
  return true;
}

// Both libraries' accumulate_kernel (grid n_groups V): the kSums sums of workgroup g of frame v into row v n_groups + g of
// the slab.  The kernel itself is shared, not a function that two kernels call: a body that reaches a kernel through a
// call is optimised on its own first and comes out with another schedule than the one that was measured.  Scale is empty
// with six degrees of freedom and one `const float* __restrict__`, the frames' fp32 scales, with seven, so that each
// library's kernel has exactly its own arguments.
template <int kDof, class... Scale>
__global__ __launch_bounds__(kThreads) void accumulate_kernel(Frame fr, const float* __restrict__ depth, Scale... sigma_f,
                                                              const float* __restrict__ est,
                                                              const float* __restrict__ ref,
                                                              const float* __restrict__ M, const float* __restrict__ N,
                                                              double* __restrict__ ws) {
  static_assert(sizeof...(Scale) == (kDof == 7), "a scale per frame with seven degrees of freedom, none with six");
  constexpr bool kScaled = kDof == 7;
  constexpr int kProducts = kProductsOf<kDof>, kSums = kSumsOf<kDof>;
  __shared__ double s_part[kWaves][kSums];
  const int tid = (int)threadIdx.x;
  const int g = (int)blockIdx.x % fr.n_groups, v = (int)blockIdx.x / fr.n_groups;
  const float* __restrict__ a = est + (size_t)v * kRecord;  // (the same addresses in every lane)
  const float* __restrict__ b = ref + (size_t)v * kRecord;
  float sigma = 1.0f;
  if constexpr (kScaled) sigma = (sigma_f, ...)[v];
  const int n_pix = fr.H * fr.W;
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
#pragma unroll 1
  for (int j = 0; j < kPerThread; ++j) {
    const int i = g * kTile + j * kThreads + tid;  // (< n_groups 1024 <= H W + 1023)
    double J[kDof] = {}, r = 0.0, one = 0.0;
    if (i < n_pix) {
      float Jf[kDof], rf;
      if (pair_of<kScaled>(fr, v, i % fr.W, i / fr.W, depth[(size_t)v * n_pix + i], sigma, a, b, M, N, Jf, rf)) {
#pragma unroll
        for (int k = 0; k < kDof; ++k) J[k] = (double)Jf[k];
        r = (double)rf, one = 1.0;
      }
    }
    int k = 0;
#pragma unroll
    for (int p = 0; p < kDof; ++p) {
#pragma unroll
      for (int q = p; q < kDof; ++q) {
        const double t = J[p] * J[q];
        acc[k] = acc[k] + t;
        ++k;
      }
    }
#pragma unroll
    for (int p = 0; p < kDof; ++p) {
      const double t = J[p] * r;
      acc[kProducts + p] = acc[kProducts + p] + t;
    }
    const double rr = r * r;
    acc[kSums - 2] = acc[kSums - 2] + rr;
    acc[kSums - 1] = acc[kSums - 1] + one;
  }
  // inside the wave: six butterfly steps; all 256 threads are here (none has returned)
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
    double x = acc[k];
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) {
      const double other = __shfl_xor(x, mask, 64);
      x = x + other;
    }
    acc[k] = x;
  }
  // across the four waves, through LDS, in the waves' order
  const int wave = tid >> 6, lane = tid & 63;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) s_part[wave][k] = acc[k];
  }
  __syncthreads();
  if (tid < kSums) {
    double x = s_part[0][tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) x = x + s_part[w][tid];
    ws[((size_t)v * fr.n_groups + g) * kSums + tid] = x;
  }
}

// ---- the solve: the steps of a library's solve_kernel (one wave per frame) ----

// Lanes tid = 0 .. kSums - 1 add frame v's slab rows in index order into s_sum; every lane of the workgroup comes here,
// and the sums are complete for all of them on return.
template <int kSums>
__device__ __forceinline__ void reduce_slab(int tid, const double* ws, int v, int n_groups, double* s_sum) {
  if (tid < kSums) {
    const double* __restrict__ p = ws + (size_t)v * n_groups * kSums + tid;
    double x = 0.0;
    for (int g = 0; g < n_groups; ++g) x = x + p[(size_t)g * kSums];
    s_sum[tid] = x;
  }
  __syncthreads();
}

// (The pieces of a kernel's body are __forceinline__; called from unrolled loops, every loop below has constant bounds, so
// the matrices live in registers: no scratch.)

// H, symmetric, from the first kDof (kDof + 1) / 2 sums
template <int kDof>
__device__ __forceinline__ void unpack(const double* s_sum, double (&Hm)[kDof][kDof]) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < kDof; ++i) {
#pragma unroll
    for (int j = i; j < kDof; ++j) Hm[i][j] = Hm[j][i] = s_sum[k++];
  }
}

// column j of H = L D L^T from the columns before it: the pivot D[j], which the caller judges and stores ...
template <int kDof>
__device__ __forceinline__ double ldl_pivot(int j, const double (&Hm)[kDof][kDof], const double (&L)[kDof][kDof],
                                            const double (&D)[kDof]) {
  double d = Hm[j][j];
#pragma unroll
  for (int k = 0; k < j; ++k) {
    double t = L[j][k] * L[j][k];
    t = t * D[k];
    d = d - t;
  }
  return d;
}

// ... and L's entries below the pivot d
template <int kDof>
__device__ __forceinline__ void ldl_column(int j, double d, const double (&Hm)[kDof][kDof], double (&L)[kDof][kDof],
                                           const double (&D)[kDof]) {
#pragma unroll
  for (int i = j + 1; i < kDof; ++i) {
    double s = Hm[i][j];
#pragma unroll
    for (int k = 0; k < j; ++k) {
      double t = L[i][k] * L[j][k];
      t = t * D[k];
      s = s - t;
    }
    L[i][j] = s / d;
  }
}

// x = D^-1 L^-1 (-g): the forward and the diagonal solve; g are the sums J_i r
template <int kDof>
__device__ __forceinline__ void solve_lower(const double* g, const double (&L)[kDof][kDof], const double (&D)[kDof],
                                            double (&x)[kDof]) {
#pragma unroll
  for (int i = 0; i < kDof; ++i) {
    double y = -g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) {
      const double t = L[i][k] * x[k];
      y = y - t;
    }
    x[i] = y;
  }
#pragma unroll
  for (int i = 0; i < kDof; ++i) x[i] = x[i] / D[i];
}

// row i < 6 of the back-substitution over the pose's six unknowns: x[i] less the terms of k = i + 1 .. 5, in that order
template <int kDof>
__device__ __forceinline__ double back_row(int i, const double (&L)[kDof][kDof], const double (&x)[kDof]) {
  double y = x[i];
#pragma unroll
  for (int k = i + 1; k < 6; ++k) {
    const double t = L[k][i] * x[k];
    y = y - t;
  }
  return y;
}

// the step x[0 .. 5] (translation, then rotation) applied to the state s: the rational retraction of the quaternion, and
// the centre
__device__ __forceinline__ void retract(const double* x, double* s) {
  const double h0 = 0.5 * x[3], h1 = 0.5 * x[4], h2 = 0.5 * x[5];
  double len = h0 * h0;
  len = 1.0 + len;
  double t = h1 * h1;
  len = len + t;
  t = h2 * h2;
  len = len + t;
  len = sqrt(len);
  const double dw = 1.0 / len, dx = h0 / len, dy = h1 / len, dz = h2 / len;
  const double qw = s[0], qx = s[1], qy = s[2], qz = s[3];
  double q[4];
  q[0] = ((dw * qw - dx * qx) - dy * qy) - dz * qz;
  q[1] = ((dw * qx + dx * qw) + dy * qz) - dz * qy;
  q[2] = ((dw * qy - dx * qz) + dy * qw) + dz * qx;
  q[3] = ((dw * qz + dx * qy) - dy * qx) + dz * qw;
  normalise(q);
  s[0] = q[0], s[1] = q[1], s[2] = q[2], s[3] = q[3];
  s[4] = s[4] + x[0], s[5] = s[5] + x[1], s[6] = s[6] + x[2];
}

// ---- host side ----

// n_groups, or 0 for sizes the libraries reject
inline long long groups_of(int V, int H, int W, int n_sums) {
  if (V <= 0 || H <= 0 || W <= 0) return 0;
  const long long hw = (long long)H * W;
  if (hw > INT_MAX - kTile) return 0;
  if ((long long)V * 3 * hw > INT_MAX) return 0;
  const long long n = (hw + kTile - 1) / kTile;
  if ((long long)V * n * n_sums > INT_MAX) return 0;
  return n;
}

inline bool positive(float x) { return x > 0.0f && std::isfinite(x); }  // (false for a NaN)

inline bool misaligned(const void* p, unsigned to) { return ((uintptr_t)p & (to - 1)) != 0; }

inline bool bad(const void* p, unsigned to) { return !p || misaligned(p, to); }

}  // namespace
