// The per-frame work of data/prepare_train_data.py (include/scsfm_prep.h).
//
//  resize   Pillow's ImagingResample for 8 bits per channel with host-built tap tables: one lane per output byte, a
//           horizontal pass over the source rows that the kept output rows reach, then a vertical pass over its uint8
//           result.  A pass whose size does not change is not run.
//  depth    generate_depth_map for a batch of scans: clear, collect (one lane per point), resolve (one lane per pixel).
//
// Determinism of the depth maps: collect only forms, per pixel, the maximum of (point index + 1) and, per key, the
// maximum of ~index (the lowest index), the number of points and the maximum of ~ordered(depth) (the minimum depth,
// float bits mapped to an order-preserving uint32).  Maxima and integer sums do not depend on the order of arrival.
// resolve recomputes the projection of the one or two points a pixel depends on with the same statements, so it sees
// the same bits as collect did, and stores every pixel once.
// Exactness: contraction is off, so the projection rounds as the header's statement does.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "scsfm_prep.h"

#pragma clang fp contract(off)

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kThreads = 256;
constexpr int kBits = SCSFM_PREP_PRECISION_BITS;

// ---- resize ----

__device__ inline unsigned char clip8(int acc) {
  const int v = acc >> kBits;
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// src uint8 [N, H, W, C], rows [row0, row0 + rows) -> dst uint8 [N, rows, w, C]
__global__ void __launch_bounds__(kThreads)
hpass_kernel(long long total, int H, int W, int C, int w, int row0, int rows, const unsigned char* __restrict__ src,
             const int* __restrict__ tab, const int* __restrict__ taps, int n_taps, unsigned char* __restrict__ dst) {
  const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (gid >= total) return;
  const int c = (int)(gid % C);
  long long q = gid / C;
  const int x = (int)(q % w);
  q /= w;
  const int r = (int)(q % rows);
  const long long n = q / rows;
  const int first = tab[3 * x], cnt = tab[3 * x + 1], off = tab[3 * x + 2];
  const unsigned char* __restrict__ line = src + ((n * H + row0 + r) * W) * C + c;
  int acc = 1 << (kBits - 1);
  for (int i = 0; i < cnt; ++i) {
    const int xi = first + i, ti = off + i;
    if ((unsigned)xi < (unsigned)W && (unsigned)ti < (unsigned)n_taps) acc += taps[ti] * (int)line[(long long)xi * C];
  }
  dst[gid] = clip8(acc);
}

// src uint8 [N, rows, w, C] holding source rows [row0, row0 + rows) -> dst uint8 [N, keep, w, C]
__global__ void __launch_bounds__(kThreads)
vpass_kernel(long long total, int C, int w, int keep, int row0, int rows, const unsigned char* __restrict__ src,
             const int* __restrict__ tab, const int* __restrict__ taps, int n_taps, unsigned char* __restrict__ dst) {
  const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (gid >= total) return;
  const long long line = (long long)w * C;
  const long long col = gid % line;
  const long long q = gid / line;
  const int y = (int)(q % keep);
  const long long n = q / keep;
  const int first = tab[3 * y], cnt = tab[3 * y + 1], off = tab[3 * y + 2];
  const unsigned char* __restrict__ base = src + n * rows * line + col;
  int acc = 1 << (kBits - 1);
  for (int i = 0; i < cnt; ++i) {
    const int yi = first + i - row0, ti = off + i;
    if ((unsigned)yi < (unsigned)rows && (unsigned)ti < (unsigned)n_taps) acc += taps[ti] * (int)base[yi * line];
  }
  dst[gid] = clip8(acc);
}

// the first `keep` rows of every frame
__global__ void __launch_bounds__(kThreads)
copy_rows_kernel(long long total, long long frame_in, long long frame_out, const unsigned char* __restrict__ src,
                 unsigned char* __restrict__ dst) {
  const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (gid >= total) return;
  dst[gid] = src[(gid / frame_out) * frame_in + gid % frame_out];
}

// ---- depth ----

// float bits -> uint32 with the order of the floats (negative below positive)
__device__ inline uint32_t ordered(float z) {
  const uint32_t b = __builtin_bit_cast(uint32_t, z);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ inline float unordered(uint32_t o) {
  return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

struct Proj {
  int u, v;
  float z;
  bool kept;
};

// the header's statement for one point
__device__ inline Proj project(const float* __restrict__ pt, const double* __restrict__ P, int h, int w, double bu,
                               double bv) {
  const float xf = pt[0];
  const double x = (double)xf, y = (double)pt[1], z = (double)pt[2];
  const double q0 = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
  const double q1 = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
  const double q2 = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
  const double u = rint(q0 / q2) - 1.0, v = rint(q1 / q2) - 1.0;
  Proj p;
  p.kept = xf >= 0.0f && u >= 0.0 && v >= 0.0 && u < bu && v < bv;
  p.u = p.kept ? (int)u : 0;
  p.v = p.kept ? (int)v : 0;
  // (bu <= w and bv <= h are checked by the host; this keeps a lane inside the map whatever it is given)
  p.kept = p.kept && p.u < w && p.v < h;
  p.z = (float)q2;
  return p;
}

// the scan that owns row g of `points`: the last f with scan_off[f] <= g
__device__ inline int scan_of(const int* __restrict__ scan_off, int F, long long g) {
  int lo = 0, hi = F - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long long)scan_off[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(kThreads) clear_kernel(long long words, uint32_t* __restrict__ ws) {
  const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (gid < words) ws[gid] = 0u;
}

// workspace of a scan: pix[h w] | lowest[keys] | count[keys] | minz[keys], keys = h (w - 1) + 1 (key + 1 indexes them)
__global__ void __launch_bounds__(kThreads)
collect_kernel(long long total, int F, int h, int w, double bu, double bv, const float* __restrict__ points,
               const int* __restrict__ scan_off, const double* __restrict__ P, uint32_t* __restrict__ ws) {
  const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (gid >= total) return;
  const int f = scan_of(scan_off, F, gid);
  const long long i = gid - (long long)scan_off[f];
  if (i < 0 || gid >= (long long)scan_off[f + 1]) return;
  const Proj p = project(points + 4 * gid, P + 12 * f, h, w, bu, bv);
  if (!p.kept) return;
  const long long pixels = (long long)h * w, keys = (long long)h * (w - 1) + 1;
  uint32_t* __restrict__ pix = ws + (pixels + 3 * keys) * f;
  uint32_t* __restrict__ lowest = pix + pixels;
  uint32_t* __restrict__ count = lowest + keys;
  uint32_t* __restrict__ minz = count + keys;
  const long long k = (long long)p.v * (w - 1) + p.u;  // key + 1
  atomicMax(pix + (long long)p.v * w + p.u, (uint32_t)i + 1u);
  atomicMax(lowest + k, ~(uint32_t)i);
  atomicAdd(count + k, 1u);
  atomicMax(minz + k, ~ordered(p.z));
}

__global__ void __launch_bounds__(kThreads)
resolve_kernel(long long total, int F, int h, int w, double bu, double bv, const float* __restrict__ points,
               size_t n_points, const int* __restrict__ scan_off, const double* __restrict__ P,
               const uint32_t* __restrict__ ws, float* __restrict__ depth) {
  const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (gid >= total) return;
  const long long pixels = (long long)h * w, keys = (long long)h * (w - 1) + 1;
  const int f = (int)(gid / pixels);
  const long long p = gid % pixels;
  const int y = (int)(p / w), x = (int)(p % w);
  const uint32_t* __restrict__ pix = ws + (pixels + 3 * keys) * f;
  const uint32_t* __restrict__ lowest = pix + pixels;
  const uint32_t* __restrict__ count = lowest + keys;
  const uint32_t* __restrict__ minz = count + keys;
  const long long base = (long long)scan_off[f];
  float d = 0.0f;
  const uint32_t top = pix[p];
  if (top != 0u) {
    const long long g = base + (long long)(top - 1u);
    if (g >= 0 && g < (long long)n_points) d = project(points + 4 * g, P + 12 * f, h, w, bu, bv).z;
    const long long k = (long long)y * (w - 1) + x;
    if (count[k] > 1u) {
      // every point of this pixel holds key k; the group's first point decides which pixel takes the minimum
      const long long g0 = base + (long long)(~lowest[k]);
      if (g0 >= 0 && g0 < (long long)n_points) {
        const Proj q = project(points + 4 * g0, P + 12 * f, h, w, bu, bv);
        if (q.kept && q.u == x && q.v == y) d = unordered(~minz[k]);
      }
    }
  }
  depth[gid] = d < 0.0f ? 0.0f : d;
}

inline int ceil_div(long long a, int b) { return (int)((a + b - 1) / b); }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int launch_status() { return (int)hipGetLastError(); }
constexpr long long kMaxBytes = (long long)1 << 31;   // of one image buffer
constexpr long long kMaxWords = (long long)1 << 30;   // of the depth workspace
constexpr long long kMaxPoints = (long long)1 << 31;  // rows of `points` (an index + 1 fits 32 bits)

inline bool channels_ok(int C) { return C == 1 || C == 3 || C == 4; }

inline size_t resize_layout(int N, int C, int w, int src_rows, int both) {
  if (N < 1 || !channels_ok(C) || w < 1 || src_rows < 1) return 0;
  const long long bytes = (long long)N * src_rows * w * C;
  if (bytes >= kMaxBytes || !both) return 0;
  return align256((size_t)bytes);
}

inline long long velo_words(int F, int h, int w) {
  if (F < 1 || h < 1 || w < 1) return 0;
  const long long per = (long long)h * w + 3 * ((long long)h * (w - 1) + 1);
  if (per >= kMaxWords || per * F >= kMaxWords) return 0;
  return per * F;
}

}  // namespace

extern "C" {

int scsfm_prep_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_prep_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

size_t scsfm_prep_resize_workspace_bytes(int N, int C, int w, int src_rows, int both_passes) {
  return resize_layout(N, C, w, src_rows, both_passes);
}

int scsfm_prep_resize_u8(int N, int H, int W, int C, int keep_rows, int w, const unsigned char* in, const int* hrows,
                         const int* htaps, int n_htaps, const int* vrows, const int* vtaps, int n_vtaps, int src_row0,
                         int src_rows, unsigned char* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (N < 1 || H < 1 || W < 1 || !channels_ok(C) || keep_rows < 1 || w < 1 || !in || !out) return SCSFM_PREP_ERR_ARG;
  if ((long long)N * H * W * C >= kMaxBytes || (long long)N * keep_rows * w * C >= kMaxBytes) return SCSFM_PREP_ERR_ARG;
  if (hrows ? (!htaps || n_htaps < 1) : w != W) return SCSFM_PREP_ERR_ARG;
  if (vrows ? (!vtaps || n_vtaps < 1) : keep_rows > H) return SCSFM_PREP_ERR_ARG;
  const bool both = hrows && vrows;
  if (both) {
    if (src_row0 < 0 || src_rows < 1 || src_rows > H || src_row0 > H - src_rows) return SCSFM_PREP_ERR_ARG;
    const size_t need = resize_layout(N, C, w, src_rows, 1);
    if (need == 0 || !workspace || workspace_bytes < need) return SCSFM_PREP_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const long long n_out = (long long)N * keep_rows * w * C;
  (void)hipGetLastError();
  if (both) {
    unsigned char* mid = static_cast<unsigned char*>(workspace);
    const long long n_mid = (long long)N * src_rows * w * C;
    hipLaunchKernelGGL(hpass_kernel, dim3(ceil_div(n_mid, kThreads)), dim3(kThreads), 0, s, n_mid, H, W, C, w, src_row0,
                       src_rows, in, hrows, htaps, n_htaps, mid);
    hipLaunchKernelGGL(vpass_kernel, dim3(ceil_div(n_out, kThreads)), dim3(kThreads), 0, s, n_out, C, w, keep_rows,
                       src_row0, src_rows, mid, vrows, vtaps, n_vtaps, out);
  } else if (hrows) {
    // the kept rows of a frame are its first keep_rows rows: every frame is H rows apart in `in`
    hipLaunchKernelGGL(hpass_kernel, dim3(ceil_div(n_out, kThreads)), dim3(kThreads), 0, s, n_out, H, W, C, w, 0,
                       keep_rows, in, hrows, htaps, n_htaps, out);
  } else if (vrows) {
    hipLaunchKernelGGL(vpass_kernel, dim3(ceil_div(n_out, kThreads)), dim3(kThreads), 0, s, n_out, C, w, keep_rows, 0, H,
                       in, vrows, vtaps, n_vtaps, out);
  } else {
    hipLaunchKernelGGL(copy_rows_kernel, dim3(ceil_div(n_out, kThreads)), dim3(kThreads), 0, s, n_out,
                       (long long)H * W * C, (long long)keep_rows * w * C, in, out);
  }
  return launch_status();
}

size_t scsfm_prep_velo_workspace_bytes(int F, int h, int w) { return align256((size_t)velo_words(F, h, w) * 4); }

int scsfm_prep_velo_depth(int F, int h, int w, double bound_u, double bound_v, const float* points, size_t total,
                          const int* scan_off, const double* P, float* depth, void* workspace, size_t workspace_bytes,
                          void* stream) {
  const long long words = velo_words(F, h, w);
  if (words == 0 || !(bound_u > 0.0 && bound_u <= (double)w) || !(bound_v > 0.0 && bound_v <= (double)h) ||
      (total > 0 && !points) || total >= (size_t)kMaxPoints || !scan_off || !P ||
      !depth || !workspace || workspace_bytes < align256((size_t)words * 4))
    return SCSFM_PREP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* ws = static_cast<uint32_t*>(workspace);
  const long long n_points = (long long)total, n_pix = (long long)F * h * w;
  (void)hipGetLastError();
  hipLaunchKernelGGL(clear_kernel, dim3(ceil_div(words, kThreads)), dim3(kThreads), 0, s, words, ws);
  if (n_points > 0)
    hipLaunchKernelGGL(collect_kernel, dim3(ceil_div(n_points, kThreads)), dim3(kThreads), 0, s, n_points, F, h, w,
                       bound_u, bound_v, points, scan_off, P, ws);
  hipLaunchKernelGGL(resolve_kernel, dim3(ceil_div(n_pix, kThreads)), dim3(kThreads), 0, s, n_pix, F, h, w, bound_u,
                     bound_v, points, total, scan_off, P, ws, depth);
  return launch_status();
}

}  // extern "C"
