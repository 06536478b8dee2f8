// KITTI visual odometry testing and evaluation (include/scsfm_odom.h): test_vo.py's pose fold as a scan, and
// kitti_eval/kitti_odometry.py's KittiEvalOdom.eval for a whole ragged set of sequences in five launches.
//
//  chain_local   one workgroup per 256 pose vectors of one sequence: pose_vec2mat in the input precision, lifted to
//                double, inverted, then the inclusive prefix product of the workgroup's 256 affine maps -- a
//                Hillis-Steele scan over the lanes of a wave with __shfl_up (12 doubles per map), the four waves'
//                products combined through LDS.  The workgroup's own product goes to the workspace.
//  chain_carry   one wave per sequence: the prefix product of the workgroups' products (64 at a time, with a carry).
//  chain_apply   every pose of workgroup b >= 1 is multiplied from the left by the product of the workgroups before it.
//                (A set whose longest sequence fits one workgroup is done after chain_local.)
//
//  rebase        one lane per frame: X_i <- inv(X_0) X_i for the ground truth and the prediction; GT step lengths.
//  align         one workgroup per sequence: the cumulative GT distance (a scan with a carry) and the alignment -- the
//                sums reduced thread-strided, then by a wave's shuffle tree, then over the waves in order; lane 0
//                solves the 3x3 SVD (one-sided Jacobi in double, the matrices in LDS) and stores c, r, t.
//  apply         one lane per frame: the aligned prediction; the frame's ATE term and (with frame i + 1) RPE terms.
//  segments      one lane per (first frame, length): binary search for the end frame, the pose error.
//  finish        one workgroup per sequence: the segments that exist compacted in slot order (a scan, not an atomic
//                ticket), the per-length and overall means, ATE and RPE.
//
// Determinism: no float atomics.  Every sum of a sequence depends only on that sequence's data and the workgroup size.
// Exactness: contraction is off below the rotations, so products, inverses and error terms round as the numpy
// statements of the header do; the rotations above the pragma are compiled as csrc/scsfm_geom.h's, whose closed forms
// they repeat.
#include <hip/hip_runtime.h>

#include <math.h>

#include "scsfm_odom.h"

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
constexpr int kLengths = SCSFM_ODOM_LENGTHS;
constexpr int kStep = SCSFM_ODOM_STEP;
constexpr int kXf = 16;  // doubles per sequence: c, r[9], t[3], apply

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

// the general inverse: adjugate / determinant, -(A^-1 t)
__device__ inline Aff inverse(const Aff& x) {
  const double* a = x.a;
  const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
  const double det = (a[0] * c0 + a[1] * c1) + a[2] * c2;
  Aff z;
  z.a[0] = c0 / det;
  z.a[3] = c1 / det;
  z.a[6] = c2 / det;
  z.a[1] = (a[2] * a[7] - a[1] * a[8]) / det;
  z.a[4] = (a[0] * a[8] - a[2] * a[6]) / det;
  z.a[7] = (a[1] * a[6] - a[0] * a[7]) / det;
  z.a[2] = (a[1] * a[5] - a[2] * a[4]) / det;
  z.a[5] = (a[2] * a[3] - a[0] * a[5]) / det;
  z.a[8] = (a[0] * a[4] - a[1] * a[3]) / det;
#pragma unroll
  for (int i = 0; i < 3; ++i) z.t[i] = -((z.a[3 * i] * x.t[0] + z.a[3 * i + 1] * x.t[1]) + z.a[3 * i + 2] * x.t[2]);
  return z;
}

__device__ inline Aff shfl_up_aff(const Aff& x, int d) {
  Aff y;
#pragma unroll
  for (int i = 0; i < 9; ++i) y.a[i] = __shfl_up(x.a[i], d);
#pragma unroll
  for (int i = 0; i < 3; ++i) y.t[i] = __shfl_up(x.t[i], d);
  return y;
}

__device__ inline Aff shfl_aff(const Aff& x, int lane) {
  Aff y;
#pragma unroll
  for (int i = 0; i < 9; ++i) y.a[i] = __shfl(x.a[i], lane);
#pragma unroll
  for (int i = 0; i < 3; ++i) y.t[i] = __shfl(x.t[i], lane);
  return y;
}

// inclusive prefix product over the lanes of a wave: lane l ends with x_0 x_1 ... x_l
__device__ inline Aff wave_scan(Aff x) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int d = 1; d < kWave; d <<= 1) {
    const Aff y = shfl_up_aff(x, d);
    if (lane >= d) x = mul(y, x);
  }
  return x;
}

// rotation_error / translation_error of kitti_odometry.py (Python's min / max: a NaN stays a NaN)
__device__ inline double rot_err(const Aff& e) {
  double d = 0.5 * (((e.a[0] + e.a[4]) + e.a[8]) - 1.0);
  d = 1.0 < d ? 1.0 : d;
  d = -1.0 > d ? -1.0 : d;
  return acos(d);
}
__device__ inline double trans_err(const Aff& e) {
  return sqrt((e.t[0] * e.t[0] + e.t[1] * e.t[1]) + e.t[2] * e.t[2]);
}

// ---- workgroup reductions (fixed order: a wave's shuffle tree, then the waves in order) ----

template <class T>
__device__ inline T block_sum(T v, T* red) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d);
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  T s = red[0];
  for (int k = 1; k < kWaves; ++k) s += red[k];
  return s;
}

// inclusive prefix sum over the workgroup in thread order; *total gets the sum
template <class T>
__device__ inline T block_incl_scan(T v, T* red, T* total) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  for (int d = 1; d < kWave; d <<= 1) {
    const T t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  __syncthreads();
  if (lane == kWave - 1) red[wv] = v;
  __syncthreads();
  T before = 0, all = 0;
  for (int k = 0; k < kWaves; ++k) {
    if (k < wv) before += red[k];
    all += red[k];
  }
  *total = all;
  return before + v;
}

// ---- the pose chain ----

template <class T>
__global__ __launch_bounds__(kThreads) void chain_local_kernel(int nblk, int quat, const T* __restrict__ vec,
                                                               const int* __restrict__ off,
                                                               const int* __restrict__ len,
                                                               const int* __restrict__ out_off, T* __restrict__ local,
                                                               double* __restrict__ poses, double* __restrict__ agg) {
  __shared__ double wagg[kWaves][12];
  const int s = blockIdx.x / nblk, b = blockIdx.x - s * nblk;
  const int n = len[s];
  if (b > 0 && b * kThreads >= n) return;  // (workgroup-uniform)
  const int k = b * kThreads + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  Aff x = identity();
  if (k < n) {
    const T* p = vec + 6ll * (off[s] + k);
    T R[9];
    if (quat) quat_to_R(p[3], p[4], p[5], R); else euler_to_R(p[3], p[4], p[5], R);
    Aff m;
#pragma unroll
    for (int i = 0; i < 9; ++i) m.a[i] = (double)R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) m.t[i] = (double)p[i];
    if (local) {
      T* o = local + 12ll * (off[s] + k);
#pragma unroll
      for (int i = 0; i < 3; ++i) o[4 * i] = R[3 * i], o[4 * i + 1] = R[3 * i + 1], o[4 * i + 2] = R[3 * i + 2], o[4 * i + 3] = p[i];
    }
    x = inverse(m);
  }
  x = wave_scan(x);
  if (lane == kWave - 1) store(wagg[wv], x);
  __syncthreads();
  if (wv > 0) {
    Aff before = load(wagg[0]);
    for (int w = 1; w < wv; ++w) before = mul(before, load(wagg[w]));
    x = mul(before, x);
  }
  double* out = poses + 12ll * out_off[s];
  if (k < n) store(out + 12ll * (k + 1), x);
  if (b == 0 && threadIdx.x == 0) store(out, identity());
  if (threadIdx.x == kThreads - 1) store(agg + 12ll * blockIdx.x, x);
}

// carry[s, b] = agg[s, 0] agg[s, 1] ... agg[s, b - 1]   (identity for b = 0)
__global__ __launch_bounds__(kWave) void chain_carry_kernel(int nblk, const int* __restrict__ len,
                                                            const double* __restrict__ agg,
                                                            double* __restrict__ carry) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int used = (len[s] + kThreads - 1) / kThreads;  // workgroups of chain_local that stored a product
  Aff c = identity();
  if (lane == 0) store(carry + 12ll * s * nblk, c);
  for (int b0 = 0; b0 < used; b0 += kWave) {  // (wave-uniform)
    const int b = b0 + lane;
    Aff x = b < used ? load(agg + 12ll * (s * nblk + b)) : identity();
    x = mul(c, wave_scan(x));
    if (b + 1 < used) store(carry + 12ll * (s * nblk + b + 1), x);
    c = shfl_aff(x, kWave - 1);
  }
}

__global__ __launch_bounds__(kThreads) void chain_apply_kernel(int nblk, const int* __restrict__ len,
                                                               const int* __restrict__ out_off,
                                                               const double* __restrict__ carry,
                                                               double* __restrict__ poses) {
  const int s = blockIdx.x / nblk, b = blockIdx.x - s * nblk;
  const int k = b * kThreads + threadIdx.x;
  if (b == 0 || k >= len[s]) return;
  double* row = poses + 12ll * (out_off[s] + k + 1);
  store(row, mul(load(carry + 12ll * blockIdx.x), load(row)));
}

// ---- evaluation ----

__global__ __launch_bounds__(kThreads) void rebase_kernel(int nblk, const double* __restrict__ gt,
                                                          const double* __restrict__ pred,
                                                          const int* __restrict__ off, const int* __restrict__ len,
                                                          double* __restrict__ gt_rel, double* __restrict__ prel,
                                                          double* __restrict__ step) {
  const int s = blockIdx.x / nblk, b = blockIdx.x - s * nblk;
  const int i = b * kThreads + threadIdx.x;
  if (i >= len[s]) return;
  const long long base = off[s];
  const Aff g0 = inverse(load(gt + 12 * base)), p0 = inverse(load(pred + 12 * base));
  const Aff g = mul(g0, load(gt + 12 * (base + i)));
  store(gt_rel + 12 * (base + i), g);
  store(prel + 12 * (base + i), mul(p0, load(pred + 12 * (base + i))));
  double d = 0.0;
  if (i > 0) {  // trajectory_distances: P1 = frame i - 1, P2 = frame i
    const Aff h = mul(g0, load(gt + 12 * (base + i - 1)));
    const double dx = h.t[0] - g.t[0], dy = h.t[1] - g.t[1], dz = h.t[2] - g.t[2];
    d = sqrt((dx * dx + dy * dy) + dz * dz);
  }
  step[base + i] = d;
}

// C (LDS, row-major 3x3) = U D V^T by one-sided Jacobi; called by one lane.  On return A holds U, V holds V (not
// transposed) and d the singular values in descending order.
__device__ inline void svd3(double (*A)[3], double (*V)[3], double* d) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    int rotated = 0;
    for (int p = 0; p < 2; ++p) {
      for (int q = p + 1; q < 3; ++q) {
        const double alpha = (A[0][p] * A[0][p] + A[1][p] * A[1][p]) + A[2][p] * A[2][p];
        const double beta = (A[0][q] * A[0][q] + A[1][q] * A[1][q]) + A[2][q] * A[2][q];
        const double gamma = (A[0][p] * A[0][q] + A[1][p] * A[1][q]) + A[2][p] * A[2][q];
        if (!(fabs(gamma) > 4.440892098500626e-16 * sqrt(alpha * beta))) continue;
        rotated = 1;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double az = fabs(zeta);
        double t = 1.0 / (az + sqrt(1.0 + zeta * zeta));
        if (zeta < 0.0) t = -t;
        const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
        for (int k = 0; k < 3; ++k) {
          const double ap = A[k][p], aq = A[k][q], vp = V[k][p], vq = V[k][q];
          A[k][p] = c * ap - sn * aq;
          A[k][q] = sn * ap + c * aq;
          V[k][p] = c * vp - sn * vq;
          V[k][q] = sn * vp + c * vq;
        }
      }
    }
    if (!rotated) break;
  }
  for (int j = 0; j < 3; ++j) d[j] = sqrt((A[0][j] * A[0][j] + A[1][j] * A[1][j]) + A[2][j] * A[2][j]);
  // descending order (three compare-exchanges of columns)
  for (int pass = 0; pass < 3; ++pass) {
    const int p = pass == 1 ? 1 : 0, q = p + 1;
    if (d[p] < d[q]) {
      const double td = d[p];
      d[p] = d[q];
      d[q] = td;
      for (int k = 0; k < 3; ++k) {
        const double ta = A[k][p], tv = V[k][p];
        A[k][p] = A[k][q], A[k][q] = ta;
        V[k][p] = V[k][q], V[k][q] = tv;
      }
    }
  }
  // U: the columns over their norms; a column without a direction (d_j <= 1e-13 d_0) is completed orthonormally
  if (!(d[0] > 0.0)) {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) A[i][j] = i == j ? 1.0 : 0.0;
    return;
  }
  const double tiny = 1e-13 * d[0];
  for (int k = 0; k < 3; ++k) A[k][0] = A[k][0] / d[0];
  if (d[1] > tiny) {
    for (int k = 0; k < 3; ++k) A[k][1] = A[k][1] / d[1];
  } else {
    int m = 0;
    if (fabs(A[1][0]) < fabs(A[m][0])) m = 1;
    if (fabs(A[2][0]) < fabs(A[m][0])) m = 2;
    double w[3];
    for (int k = 0; k < 3; ++k) w[k] = (k == m ? 1.0 : 0.0) - A[m][0] * A[k][0];
    const double nw = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    for (int k = 0; k < 3; ++k) A[k][1] = w[k] / nw;
  }
  if (d[2] > tiny) {
    for (int k = 0; k < 3; ++k) A[k][2] = A[k][2] / d[2];
  } else {
    A[0][2] = A[1][0] * A[2][1] - A[2][0] * A[1][1];
    A[1][2] = A[2][0] * A[0][1] - A[0][0] * A[2][1];
    A[2][2] = A[0][0] * A[1][1] - A[1][0] * A[0][1];
  }
}

__device__ inline double det3(double (*m)[3]) {
  return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) + m[0][1] * (m[1][2] * m[2][0] - m[1][0] * m[2][2])) +
         m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

__global__ __launch_bounds__(kThreads) void align_kernel(int align, const int* __restrict__ off,
                                                         const int* __restrict__ len,
                                                         const double* __restrict__ gt_rel,
                                                         const double* __restrict__ prel, double* __restrict__ dist,
                                                         double* __restrict__ xf) {
  __shared__ double red[kWaves];
  __shared__ double A[3][3], V[3][3];
  const int s = blockIdx.x, n = len[s];
  const long long base = off[s];

  // cumulative GT distance, in place over the step lengths
  double carry = 0.0;
  for (int i0 = 0; i0 < n; i0 += kThreads) {
    const int i = i0 + threadIdx.x;
    double total;
    const double incl = block_incl_scan(i < n ? dist[base + i] : 0.0, red, &total);
    if (i < n) dist[base + i] = carry + incl;
    carry = carry + total;
  }

  double* o = xf + (long long)s * kXf;
  const double dn = (double)n;
  if (align == SCSFM_ODOM_ALIGN_NONE) {
    if (threadIdx.x == 0) {
      o[0] = 1.0;
      for (int k = 1; k < kXf; ++k) o[k] = 0.0;
    }
    return;
  }
  if (align == SCSFM_ODOM_ALIGN_SCALE) {  // scale_lse_solver: sum(X * Y) / sum(X ** 2)
    double sxy = 0.0, sxx = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads) {
      const double* x = prel + 12 * (base + i);
      const double* y = gt_rel + 12 * (base + i);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        sxy += x[4 * k + 3] * y[4 * k + 3];
        sxx += x[4 * k + 3] * x[4 * k + 3];
      }
    }
    sxy = block_sum(sxy, red);
    sxx = block_sum(sxx, red);
    if (threadIdx.x == 0) {
      o[0] = sxy / sxx;
      for (int k = 1; k < kXf; ++k) o[k] = 0.0;
    }
    return;
  }
  // umeyama_alignment(x = prediction, y = ground truth)
  double mx[3] = {0.0, 0.0, 0.0}, my[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n; i += kThreads) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      mx[k] += prel[12 * (base + i) + 4 * k + 3];
      my[k] += gt_rel[12 * (base + i) + 4 * k + 3];
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    mx[k] = block_sum(mx[k], red) / dn;
    my[k] = block_sum(my[k], red) / dn;
  }
  double sig = 0.0, cov[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n; i += kThreads) {
    double dx[3], dy[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      dx[k] = prel[12 * (base + i) + 4 * k + 3] - mx[k];
      dy[k] = gt_rel[12 * (base + i) + 4 * k + 3] - my[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      sig += dx[k] * dx[k];
#pragma unroll
      for (int j = 0; j < 3; ++j) cov[3 * k + j] += dy[k] * dx[j];
    }
  }
  sig = block_sum(sig, red);
#pragma unroll
  for (int k = 0; k < 9; ++k) cov[k] = block_sum(cov[k], red);
  if (threadIdx.x != 0) return;
  const double inv_n = 1.0 / dn;
  const double nrm = sqrt(sig);
  const double sigma_x = inv_n * (nrm * nrm);
  for (int k = 0; k < 9; ++k) A[k / 3][k % 3] = inv_n * cov[k];
  double d[3];
  svd3(A, V, d);
  // det(u) * det(v) with v = V^T (the determinant of a transpose is computed on the transpose)
  double Vt[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Vt[i][j] = V[j][i];
  const double s3 = det3(A) * det3(Vt) < 0.0 ? -1.0 : 1.0;
  double r[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r[3 * i + j] = (A[i][0] * Vt[0][j] + A[i][1] * Vt[1][j]) + (A[i][2] * s3) * Vt[2][j];
  const double c = align == SCSFM_ODOM_ALIGN_6DOF ? 1.0 : (1.0 / sigma_x) * ((d[0] + d[1]) + d[2] * s3);
  o[0] = c;
  for (int k = 0; k < 9; ++k) o[1 + k] = r[k];
  for (int i = 0; i < 3; ++i)
    o[10 + i] = my[i] - c * ((r[3 * i] * mx[0] + r[3 * i + 1] * mx[1]) + r[3 * i + 2] * mx[2]);
  o[13] = align == SCSFM_ODOM_ALIGN_SCALE_7DOF ? 0.0 : 1.0;
  o[14] = o[15] = 0.0;
}

__device__ inline Aff aligned_pose(const double* __restrict__ row, const double* __restrict__ x) {
  Aff p = load(row);
  const double c = x[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) p.t[i] = p.t[i] * c;
  if (x[13] != 0.0) {
    Aff a;
#pragma unroll
    for (int i = 0; i < 9; ++i) a.a[i] = x[1 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) a.t[i] = x[10 + i];
    p = mul(a, p);
  }
  return p;
}

__global__ __launch_bounds__(kThreads) void apply_kernel(int nblk, const int* __restrict__ off,
                                                         const int* __restrict__ len,
                                                         const double* __restrict__ gt_rel,
                                                         const double* __restrict__ prel,
                                                         const double* __restrict__ xf, double* __restrict__ aligned,
                                                         double* __restrict__ ate2, double* __restrict__ rpe_t,
                                                         double* __restrict__ rpe_r) {
  const int s = blockIdx.x / nblk, b = blockIdx.x - s * nblk;
  const int i = b * kThreads + threadIdx.x, n = len[s];
  if (i >= n) return;
  const long long row = (long long)off[s] + i;
  const double* x = xf + (long long)s * kXf;
  const Aff p = aligned_pose(prel + 12 * row, x);
  const Aff g = load(gt_rel + 12 * row);
  store(aligned + 12 * row, p);
  // compute_ATE: sqrt(sum((gt_xyz - pred_xyz) ** 2)), squared again for the RMSE
  const double ex = g.t[0] - p.t[0], ey = g.t[1] - p.t[1], ez = g.t[2] - p.t[2];
  const double e = sqrt((ex * ex + ey * ey) + ez * ez);
  ate2[row] = e * e;
  double rt = 0.0, rr = 0.0;
  if (i + 1 < n) {  // compute_RPE
    const Aff p2 = aligned_pose(prel + 12 * (row + 1), x);
    const Aff g2 = load(gt_rel + 12 * (row + 1));
    const Aff err = mul(inverse(mul(inverse(g), g2)), mul(inverse(p), p2));
    rt = trans_err(err);
    rr = rot_err(err);
  }
  rpe_t[row] = rt;
  rpe_r[row] = rr;
}

// slot = (f / 10) * 8 + k of sequence s: tmp[slot * 5 + 0..4] = f, r_err / L, t_err / L, L, speed; L = 0: no segment
__global__ __launch_bounds__(kThreads) void segment_kernel(int nblk, int max_slots, const int* __restrict__ off,
                                                           const int* __restrict__ len,
                                                           const double* __restrict__ gt_rel,
                                                           const double* __restrict__ aligned,
                                                           const double* __restrict__ dist, double* __restrict__ tmp) {
  const int s = blockIdx.x / nblk, b = blockIdx.x - s * nblk;
  const int slot = b * kThreads + threadIdx.x, n = len[s];
  if (slot >= max_slots) return;
  const int f = slot / kLengths * kStep, k = slot - slot / kLengths * kLengths;
  double* o = tmp + ((long long)s * max_slots + slot) * 5;
  if (f >= n) {
    o[3] = 0.0;
    return;
  }
  const long long base = off[s];
  const double* ds = dist + base;
  const double L = 100.0 * (k + 1);
  const double thr = ds[f] + L;
  int lo = f, hi = n;  // the first frame whose distance exceeds thr (the distances do not decrease)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ds[mid] > thr) hi = mid; else lo = mid + 1;
  }
  if (lo >= n) {
    o[3] = 0.0;
    return;
  }
  const Aff dg = mul(inverse(load(gt_rel + 12 * (base + f))), load(gt_rel + 12 * (base + lo)));
  const Aff dp = mul(inverse(load(aligned + 12 * (base + f))), load(aligned + 12 * (base + lo)));
  const Aff err = mul(inverse(dp), dg);
  const double nf = (double)(lo - f) + 1.0;
  o[0] = (double)f;
  o[1] = rot_err(err) / L;
  o[2] = trans_err(err) / L;
  o[3] = L;
  o[4] = L / (0.1 * nf);
}

__global__ __launch_bounds__(kThreads) void finish_kernel(int max_slots, int max_seg, const int* __restrict__ off,
                                                          const int* __restrict__ len,
                                                          const double* __restrict__ tmp,
                                                          const double* __restrict__ xf,
                                                          const double* __restrict__ ate2,
                                                          const double* __restrict__ rpe_t,
                                                          const double* __restrict__ rpe_r,
                                                          double* __restrict__ summary,
                                                          double* __restrict__ per_length, double* __restrict__ seg,
                                                          int* __restrict__ n_seg) {
  __shared__ int ired[kWaves];
  __shared__ double dred[kWaves];
  __shared__ double st[kThreads], sr[kThreads];
  __shared__ int sc[kThreads];
  __shared__ double lt[kLengths], lr[kLengths];
  __shared__ int lc[kLengths];
  const int s = blockIdx.x, n = len[s];
  const long long base = off[s];
  const double* slots = tmp + (long long)s * max_slots * 5;
  double* rows = seg + (long long)s * max_seg * 5;

  // compaction in slot order; a thread always meets the same length (kThreads is a multiple of kLengths)
  double at = 0.0, ar = 0.0;
  int ac = 0, carry = 0;
  for (int j0 = 0; j0 < max_slots; j0 += kThreads) {
    const int j = j0 + threadIdx.x;
    const bool has = j < max_slots && slots[j * 5 + 3] != 0.0;
    int total;
    const int at_row = carry + block_incl_scan(has ? 1 : 0, ired, &total) - 1;
    if (has) {
#pragma unroll
      for (int q = 0; q < 5; ++q) rows[at_row * 5 + q] = slots[j * 5 + q];
      ar += slots[j * 5 + 1];
      at += slots[j * 5 + 2];
      ++ac;
    }
    carry += total;
  }
  for (int j = carry + threadIdx.x; j < max_seg; j += kThreads) {
#pragma unroll
    for (int q = 0; q < 5; ++q) rows[j * 5 + q] = 0.0;
  }
  st[threadIdx.x] = at, sr[threadIdx.x] = ar, sc[threadIdx.x] = ac;
  __syncthreads();
  if (threadIdx.x < kLengths) {
    double t = 0.0, r = 0.0;
    int c = 0;
    for (int j = threadIdx.x; j < kThreads; j += kLengths) t += st[j], r += sr[j], c += sc[j];
    lt[threadIdx.x] = t, lr[threadIdx.x] = r, lc[threadIdx.x] = c;
    double* pl = per_length + ((long long)s * kLengths + threadIdx.x) * 3;
    pl[0] = c > 0 ? t / (double)c : 0.0;
    pl[1] = c > 0 ? r / (double)c : 0.0;
    pl[2] = (double)c;
  }

  double a2 = 0.0, rt = 0.0, rr = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    a2 += ate2[base + i];
    if (i + 1 < n) rt += rpe_t[base + i], rr += rpe_r[base + i];
  }
  a2 = block_sum(a2, dred);  // (its barriers also publish lt / lr / lc)
  rt = block_sum(rt, dred);
  rr = block_sum(rr, dred);
  if (threadIdx.x == 0) {
    double t = 0.0, r = 0.0;
    for (int k = 0; k < kLengths; ++k) t += lt[k], r += lr[k];
    double* o = summary + (long long)s * SCSFM_ODOM_SUMMARY;
    o[0] = carry > 0 ? t / (double)carry : 0.0;
    o[1] = carry > 0 ? r / (double)carry : 0.0;
    o[2] = sqrt(a2 / (double)n);
    o[3] = rt / (double)(n - 1);  // (0 / 0 = NaN for a one-frame sequence: numpy's mean of nothing)
    o[4] = rr / (double)(n - 1);
    o[5] = xf[(long long)s * kXf];
    o[6] = (double)carry;
    n_seg[s] = carry;
  }
}

inline int ceil_div(long long a, int b) { return (int)((a + b - 1) / b); }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int launch_status() { return (int)hipGetLastError(); }
constexpr int kMaxLen = 1 << 24;  // frames per sequence
constexpr int kMaxSeq = 1 << 16;

struct ChainLayout {
  size_t agg, carry, bytes;
};

inline bool chain_layout(int S, int max_len, ChainLayout* L) {
  if (S <= 0 || S > kMaxSeq || max_len < 0 || max_len > kMaxLen) return false;
  const long long nb = (long long)S * (max_len > 0 ? ceil_div(max_len, kThreads) : 1);
  if (nb >= (1ll << 24)) return false;
  L->agg = 0;
  L->carry = align256(nb * 12 * sizeof(double));
  L->bytes = 2 * L->carry;
  return true;
}

struct EvalLayout {
  size_t prel, dist, ate2, rpe_t, rpe_r, xf, tmp, bytes;
  int max_slots;
};

inline bool eval_layout(int S, int max_len, size_t total, EvalLayout* L) {
  if (S <= 0 || S > kMaxSeq || max_len <= 0 || max_len > kMaxLen || total == 0 || total >= ((size_t)1 << 30))
    return false;
  L->max_slots = kLengths * ceil_div(max_len, kStep);
  if ((long long)S * ceil_div(L->max_slots, kThreads) >= (1ll << 24)) return false;
  const size_t rows = align256(total * sizeof(double));
  L->prel = 0;
  L->dist = align256(total * 12 * sizeof(double));
  L->ate2 = L->dist + rows;
  L->rpe_t = L->ate2 + rows;
  L->rpe_r = L->rpe_t + rows;
  L->xf = L->rpe_r + rows;
  L->tmp = L->xf + align256((size_t)S * kXf * sizeof(double));
  L->bytes = L->tmp + align256((size_t)S * L->max_slots * 5 * sizeof(double));
  return true;
}

template <class T>
int run_chain(int S, int max_len, int quat, const T* vec, const int* off, const int* len, const int* out_off, T* local,
              double* poses, char* ws, const ChainLayout& L, hipStream_t stream) {
  const int nblk = max_len > 0 ? ceil_div(max_len, kThreads) : 1;
  double* agg = reinterpret_cast<double*>(ws + L.agg);
  double* carry = reinterpret_cast<double*>(ws + L.carry);
  (void)hipGetLastError();
  hipLaunchKernelGGL(chain_local_kernel<T>, dim3(S * nblk), dim3(kThreads), 0, stream, nblk, quat, vec, off, len,
                     out_off, local, poses, agg);
  if (nblk > 1) {
    hipLaunchKernelGGL(chain_carry_kernel, dim3(S), dim3(kWave), 0, stream, nblk, len, agg, carry);
    hipLaunchKernelGGL(chain_apply_kernel, dim3(S * nblk), dim3(kThreads), 0, stream, nblk, len, out_off, carry, poses);
  }
  return launch_status();
}

}  // namespace

extern "C" {

int scsfm_odom_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_odom_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

size_t scsfm_odom_chain_workspace_bytes(int S, int max_len) {
  ChainLayout L;
  return chain_layout(S, max_len, &L) ? L.bytes : 0;
}

int scsfm_odom_chain(int S, int max_len, int vec_f64, int rot_mode, const void* vec, const int* off, const int* len,
                     const int* out_off, void* local, double* poses, void* workspace, size_t workspace_bytes,
                     void* stream) {
  ChainLayout L;
  if (!chain_layout(S, max_len, &L) || (rot_mode != SCSFM_ODOM_ROT_EULER && rot_mode != SCSFM_ODOM_ROT_QUAT) ||
      (!vec && max_len > 0) || !off || !len || !out_off || !poses || !workspace || workspace_bytes < L.bytes)
    return SCSFM_ODOM_ERR_ARG;
  char* ws = static_cast<char*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  if (vec_f64)
    return run_chain<double>(S, max_len, rot_mode, static_cast<const double*>(vec), off, len, out_off,
                             static_cast<double*>(local), poses, ws, L, s);
  return run_chain<float>(S, max_len, rot_mode, static_cast<const float*>(vec), off, len, out_off,
                          static_cast<float*>(local), poses, ws, L, s);
}

size_t scsfm_odom_eval_max_segments(int max_len) {
  if (max_len <= 0 || max_len > kMaxLen) return 0;
  return (size_t)kLengths * ceil_div(max_len, kStep);
}

size_t scsfm_odom_eval_workspace_bytes(int S, int max_len, size_t total) {
  EvalLayout L;
  return eval_layout(S, max_len, total, &L) ? L.bytes : 0;
}

int scsfm_odom_eval(int S, int max_len, size_t total, int align, const double* gt, const double* pred, const int* off,
                    const int* len, int max_seg, void* workspace, size_t workspace_bytes, double* summary,
                    double* per_length, double* seg, int* n_seg, double* gt_rel, double* aligned, void* stream) {
  EvalLayout L;
  if (!eval_layout(S, max_len, total, &L) || align < SCSFM_ODOM_ALIGN_NONE || align > SCSFM_ODOM_ALIGN_6DOF || !gt ||
      !pred || !off || !len || max_seg < L.max_slots || !workspace || workspace_bytes < L.bytes || !summary ||
      !per_length || !seg || !n_seg || !gt_rel || !aligned)
    return SCSFM_ODOM_ERR_ARG;
  char* ws = static_cast<char*>(workspace);
  double* prel = reinterpret_cast<double*>(ws + L.prel);
  double* dist = reinterpret_cast<double*>(ws + L.dist);
  double* ate2 = reinterpret_cast<double*>(ws + L.ate2);
  double* rpe_t = reinterpret_cast<double*>(ws + L.rpe_t);
  double* rpe_r = reinterpret_cast<double*>(ws + L.rpe_r);
  double* xf = reinterpret_cast<double*>(ws + L.xf);
  double* tmp = reinterpret_cast<double*>(ws + L.tmp);
  hipStream_t s = (hipStream_t)stream;
  const int nblk = ceil_div(max_len, kThreads), sblk = ceil_div(L.max_slots, kThreads);
  (void)hipGetLastError();
  hipLaunchKernelGGL(rebase_kernel, dim3(S * nblk), dim3(kThreads), 0, s, nblk, gt, pred, off, len, gt_rel, prel, dist);
  hipLaunchKernelGGL(align_kernel, dim3(S), dim3(kThreads), 0, s, align, off, len, gt_rel, prel, dist, xf);
  hipLaunchKernelGGL(apply_kernel, dim3(S * nblk), dim3(kThreads), 0, s, nblk, off, len, gt_rel, prel, xf, aligned,
                     ate2, rpe_t, rpe_r);
  hipLaunchKernelGGL(segment_kernel, dim3(S * sblk), dim3(kThreads), 0, s, sblk, L.max_slots, off, len, gt_rel,
                     aligned, dist, tmp);
  hipLaunchKernelGGL(finish_kernel, dim3(S), dim3(kThreads), 0, s, L.max_slots, max_seg, off, len, tmp, xf, ate2,
                     rpe_t, rpe_r, summary, per_length, seg, n_seg);
  return launch_status();
}

}  // extern "C"
