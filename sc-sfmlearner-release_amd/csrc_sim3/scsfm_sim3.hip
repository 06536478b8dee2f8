// Frame-to-model tracking with a scale: point-to-plane ICP over seven degrees of freedom on the maps of the ray cast
// (include/scsfm_sim3.h).  The rigid tracker of csrc_track/ restated with the scale's column, as csrc_conf/ restates the
// integration: libscsfm_track.so stays what it is, and the two share no code.
//
//  init_kernel        one lane per frame: Shepperd's quaternion of the pose, the state, the fp32 record and the fp32 scale.
//  poses_kernel       one lane per frame: the state back into twelve doubles and the scale.
//  accumulate_kernel  one workgroup (256 threads) per 1024 consecutive pixels of one frame, a thread four of them at a
//                     stride of 256, so that a wave reads 64 consecutive depths and its gathers of the model maps land on
//                     neighbouring pixels.  The 37 double accumulators (74 VGPRs) are paid once for four pixels.  The
//                     estimate's record, the reference record and the frame's scale are the same addresses in every lane
//                     (uniform loads).  The sums meet through six butterfly steps inside a wave, then through LDS across
//                     the four waves; every workgroup stores its 37 values to the slab: no atomics, no clearing.
//  solve_kernel       one wave per frame: lanes 0 .. 36 add the frame's slab rows in index order (the launch-boundary
//                     reduce: the kernel boundary is the grid-wide barrier), lane 0 factorises the 7 x 7 system with the
//                     scale last, decides from the last pivot whether the scale is solved or held, solves, updates the
//                     state and rewrites the record and the fp32 scale.
//  scale_kernel       streaming: a thread four consecutive floats of the frames, as one 16-byte load and store where the
//                     pointers allow it; the frame of an element is its index over H W.
//
// A pixel that is no pair adds +0.0 to every sum, which changes no bit: a sum that starts at +0.0 never becomes -0.0
// (x + y is -0.0 only when both are), and s + (+0.0) == s for every other s.  So the four pixels of a thread need no
// divergent accumulation.
//
// Arithmetic: the header's order, one rounding per operation, in fp32 and in double.  The pragma keeps the compiler from
// contracting a multiply and an add (hipcc's default is -ffp-contract=fast); `/` and sqrt are the correctly rounded
// expansions and fp32 denormals are kept on gfx950.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "scsfm_sim3.h"

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerThread = 4;
constexpr int kTile = SCSFM_SIM3_TILE;
constexpr int kState = SCSFM_SIM3_STATE;
constexpr int kRecord = SCSFM_SIM3_RECORD;
constexpr int kSums = SCSFM_SIM3_SUMS;
constexpr int kReport = SCSFM_SIM3_REPORT;
constexpr int kDof = 7;
constexpr int kProducts = kDof * (kDof + 1) / 2;  // 28: the upper triangle of J J^T
static_assert(kThreads * kPerThread == kTile, "a thread takes kPerThread pixels of the tile");
static_assert(kProducts + kDof + 2 == kSums, "J_i J_j, J_i r, r r, 1");

// ---- the state ----

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

// the header's matrix of a quaternion, row-major
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

__global__ __launch_bounds__(kThreads) void init_kernel(int V, const double* __restrict__ c2w,
                                                        const double* __restrict__ scale0, const float* __restrict__ K,
                                                        double* __restrict__ state, float* __restrict__ est,
                                                        float* __restrict__ sigma_f) {
  const int v = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (v >= V) return;
  const double* m = c2w + 12 * (size_t)v;
  const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[4], m11 = m[5], m12 = m[6], m20 = m[8], m21 = m[9], m22 = m[10];
  const double tr = (m00 + m11) + m22;
  double q[4], r, f;
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
  double R[9];
  matrix(s, R);
  double* o = c2w + 12 * (size_t)v;
#pragma unroll
  for (int i = 0; i < 3; ++i) o[4 * i] = R[3 * i], o[4 * i + 1] = R[3 * i + 1], o[4 * i + 2] = R[3 * i + 2], o[4 * i + 3] = s[4 + i];
  scale[v] = s[7];
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

// the pair of pixel (px, py): true and (J, r) for a pair
__device__ inline bool pair_of(const Frame& fr, int v, int px, int py, float d, float sigma, const float* __restrict__ a,
                               const float* __restrict__ b, const float* __restrict__ M, const float* __restrict__ N,
                               float J[kDof], float& r) {
  if (fr.is_disp) d = 1.0f / d;
  d = sigma * d;
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
  J[6] = nu;
  return true;
}

__global__ __launch_bounds__(kThreads) void accumulate_kernel(Frame fr, const float* __restrict__ depth,
                                                              const float* __restrict__ sigma_f,
                                                              const float* __restrict__ est,
                                                              const float* __restrict__ ref,
                                                              const float* __restrict__ M, const float* __restrict__ N,
                                                              double* __restrict__ ws) {
  __shared__ double s_part[kWaves][kSums];
  const int tid = (int)threadIdx.x;
  const int g = (int)blockIdx.x % fr.n_groups, v = (int)blockIdx.x / fr.n_groups;
  const float* __restrict__ a = est + (size_t)v * kRecord;  // (the same addresses in every lane)
  const float* __restrict__ b = ref + (size_t)v * kRecord;
  const float sigma = sigma_f[v];
  const int n_pix = fr.H * fr.W;
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
#pragma unroll 1
  for (int j = 0; j < kPerThread; ++j) {
    const int i = g * kTile + j * kThreads + tid;  // (< n_groups 1024 <= H W + 1023)
    double J[kDof] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r = 0.0, one = 0.0;
    if (i < n_pix) {
      float Jf[kDof], rf;
      if (pair_of(fr, v, i % fr.W, i / fr.W, depth[(size_t)v * n_pix + i], sigma, a, b, M, N, Jf, rf)) {
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

// ---- the solve ----

__global__ __launch_bounds__(64) void solve_kernel(int n_groups, int min_pairs, double min_scale_pivot, int n_iters,
                                                   int iter, const double* __restrict__ ws, double* __restrict__ state,
                                                   float* __restrict__ est, float* __restrict__ sigma_f,
                                                   double* __restrict__ report) {
  __shared__ double s_sum[kSums];
  const int tid = (int)threadIdx.x, v = (int)blockIdx.x;
  if (tid < kSums) {
    const double* __restrict__ p = ws + (size_t)v * n_groups * kSums + tid;
    double x = 0.0;
    for (int g = 0; g < n_groups; ++g) x = x + p[(size_t)g * kSums];
    s_sum[tid] = x;
  }
  __syncthreads();
  if (tid != 0) return;
  // (every loop below has constant bounds and is unrolled, so the matrices live in registers: no scratch)
  double Hm[kDof][kDof], L[kDof][kDof], D[kDof], x[kDof];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < kDof; ++i) {
#pragma unroll
      for (int j = i; j < kDof; ++j) Hm[i][j] = Hm[j][i] = s_sum[k++];
    }
  }
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
      // (after a pivot has failed the loops run on, on values nobody reads: the header's factorisation has stopped)
#pragma unroll
      for (int j = 0; j < kDof; ++j) {
        double d = Hm[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) {
          double t = L[j][k] * L[j][k];
          t = t * D[k];
          d = d - t;
        }
        D[j] = d;
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
#pragma unroll
        for (int i = j + 1; i < kDof; ++i) {
          double t0 = Hm[i][j];
#pragma unroll
          for (int k = 0; k < j; ++k) {
            double t = L[i][k] * L[j][k];
            t = t * D[k];
            t0 = t0 - t;
          }
          L[i][j] = t0 / d;
        }
      }
#pragma unroll
      for (int i = 0; i < kDof; ++i) {
        double y = -s_sum[kProducts + i];
#pragma unroll
        for (int k = 0; k < i; ++k) {
          const double t = L[i][k] * x[k];
          y = y - t;
        }
        x[i] = y;
      }
#pragma unroll
      for (int i = 0; i < kDof; ++i) x[i] = x[i] / D[i];
      if (!(x[6] > -1.0 && x[6] < 1.0)) held = true;
      if (held) x[6] = 0.0;
#pragma unroll
      for (int i = 5; i >= 0; --i) {
        double y = x[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) {
          const double t = L[k][i] * x[k];
          y = y - t;
        }
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

// ---- host side ----

// n_groups, or 0 for sizes the library rejects
inline long long groups_of(int V, int H, int W) {
  if (V <= 0 || H <= 0 || W <= 0) return 0;
  const long long hw = (long long)H * W;
  if (hw > INT_MAX - kTile) return 0;
  if ((long long)V * 3 * hw > INT_MAX) return 0;
  const long long n = (hw + kTile - 1) / kTile;
  if ((long long)V * n * kSums > INT_MAX) return 0;
  return n;
}

inline bool positive(float x) { return x > 0.0f && std::isfinite(x); }  // (false for a NaN)

inline bool misaligned(const void* p, unsigned to) { return ((uintptr_t)p & (to - 1)) != 0; }

inline bool bad(const void* p, unsigned to) { return !p || misaligned(p, to); }

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
  const long long n = groups_of(V, H, W);
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
  const long long n_groups = groups_of(V, H, W);
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
    hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)(n_groups * V)), dim3(kThreads), 0, (hipStream_t)stream, fr,
                       depth, (const float*)sigma_f, (const float*)est, ref, model_depth, model_normal, ws);
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
