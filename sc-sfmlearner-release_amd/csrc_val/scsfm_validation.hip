// Ground-truth validation metrics of training (include/scsfm_val.h): validate_with_gt's 1 / disp and nearest resize and
// compute_errors' per-image loop -- mask and crop, clamp, torch.median scaling, the six error terms -- for a whole batch
// in four launches and without a device-to-host copy.
//
//  count    one workgroup per 2048-pixel tile of one GT map: masks 8 consecutive pixels per lane (vector loads where the
//           address allows) and stores the tile's valid count.
//  scan     one workgroup per image: exclusive scan of its tiles' counts -> each tile's first slot; the image's count.
//  compact  the count kernel's tiling again: every valid pixel's GT value and its clamped prediction are stored at the
//           tile's first slot plus the pixel's rank in the tile, i.e. in pixel order.  The prediction is fetched by the
//           nearest-neighbour rule (and inverted, for a disparity) only where the mask holds: no resized map exists.
//  select   one workgroup per image: the lower-middle order statistic of the compacted GT and of the compacted
//           prediction by radix select on order-preserving integer keys (digits of 11, 11 and 10 bits, an LDS histogram
//           of 2048 bins), then the scaled prediction's three sums in double and three integer counts, thread-strided
//           and tree-reduced.
//
// Determinism: no float atomics anywhere.  The compacted order is pixel order (a scan, not an atomic ticket), image i's
// pairs live at i * H * W whatever the batch, and its sums depend only on its own data and the workgroup size: results
// are bit-identical from run to run and however a batch is split into calls.  Exactness: a median is an element selected
// on keys, hence the very value torch.median returns; floating-point contraction is off, so every fp32 term rounds as
// the separate tensor operations of the reference do.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "scsfm_val.h"

#pragma clang fp contract(off)

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kWave = 64;
constexpr int kPrepThreads = 256;
constexpr int kPer = 8;  // consecutive pixels per lane in count / compact
constexpr int kTile = kPrepThreads * kPer;
constexpr int kSel = 512;  // workgroup of the select kernel
constexpr int kDigit = 11;
constexpr int kBins = 1 << kDigit;
constexpr int kBinsPerThread = kBins / kSel;

// order-preserving map of a float's bits to an unsigned integer (negatives reversed below the positives)
__device__ inline unsigned to_key(float v) {
  unsigned u;
  __builtin_memcpy(&u, &v, sizeof(u));
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float from_key(unsigned k) {
  const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float v;
  __builtin_memcpy(&v, &u, sizeof(v));
  return v;
}

// ---- workgroup reductions and scans (fixed order: a wave's shuffle tree, then the waves in order) ----

template <int NT, class T>
__device__ inline T block_sum(T v, T* red) {
  constexpr int nw = NT / kWave;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d);
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  T s = red[0];
  for (int k = 1; k < nw; ++k) s += red[k];
  return s;
}

// exclusive prefix sum of v over the workgroup in thread order; *total gets the sum
template <int NT>
__device__ inline int block_excl_scan(int v, int* red, int* total) {
  constexpr int nw = NT / kWave;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  int x = v;
  for (int d = 1; d < kWave; d <<= 1) {
    const int t = __shfl_up(x, d);
    if (lane >= d) x += t;
  }
  __syncthreads();
  if (lane == kWave - 1) red[wv] = x;
  __syncthreads();
  int before = 0, all = 0;
  for (int k = 0; k < nw; ++k) {
    if (k < wv) before += red[k];
    all += red[k];
  }
  *total = all;
  return before + x - v;
}

// ---- count / compact ----

struct Box {
  int H, W, hw, y1, y2, x1, x2;
  float lo, hi;  // gt > lo && gt < hi
};

// the lane's 8 pixels p0 .. p0+7 of one GT map: values into v, the mask as bits
__device__ inline unsigned mask8(const float* __restrict__ g, const Box& m, int p0, float v[kPer]) {
  if (p0 + kPer <= m.hw && (reinterpret_cast<uintptr_t>(g + p0) & 15) == 0) {
    const float4 a = reinterpret_cast<const float4*>(g + p0)[0], b = reinterpret_cast<const float4*>(g + p0)[1];
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < kPer; ++j) v[j] = p0 + j < m.hw ? g[p0 + j] : 0.f;
  }
  int r = p0 / m.W, c = p0 - r * m.W;
  unsigned bits = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const bool ok = p0 + j < m.hw && v[j] > m.lo && v[j] < m.hi && r >= m.y1 && r < m.y2 && c >= m.x1 && c < m.x2;
    bits |= (unsigned)ok << j;
    if (++c == m.W) c = 0, ++r;
  }
  return bits;
}

__global__ __launch_bounds__(kPrepThreads) void count_kernel(int nblk, const float* __restrict__ gt, Box m,
                                                             int* __restrict__ blkcnt) {
  __shared__ int red[kPrepThreads / kWave];
  const int i = blockIdx.x / nblk, b = blockIdx.x - i * nblk;
  const int p0 = b * kTile + threadIdx.x * kPer;
  int c = 0;
  if (p0 < m.hw) {
    float v[kPer];
    c = __builtin_popcount(mask8(gt + (long long)i * m.hw, m, p0, v));
  }
  c = block_sum<kPrepThreads>(c, red);
  if (threadIdx.x == 0) blkcnt[blockIdx.x] = c;
}

__global__ __launch_bounds__(kPrepThreads) void scan_kernel(int nblk, const int* __restrict__ blkcnt,
                                                            int* __restrict__ blkoff, int* __restrict__ count) {
  __shared__ int red[kPrepThreads / kWave];
  const int i = blockIdx.x;
  int carry = 0;
  for (int b0 = 0; b0 < nblk; b0 += kPrepThreads) {
    const int b = b0 + threadIdx.x;
    const int v = b < nblk ? blkcnt[i * nblk + b] : 0;
    int total;
    const int ex = block_excl_scan<kPrepThreads>(v, red, &total);
    if (b < nblk) blkoff[i * nblk + b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) count[i] = carry;
}

// F.interpolate(mode='nearest'): the source index of destination index d, scale = (float)in / (float)out
__device__ inline int nearest(int d, float scale, int in) {
  const int s = (int)floorf((float)d * scale);
  return s < in - 1 ? s : in - 1;
}

// torch.clamp(x, lo, hi): a NaN stays NaN
__device__ inline float clampf(float x, float lo, float hi) {
  if (x != x) return x;
  return x < lo ? lo : (x > hi ? hi : x);
}

__global__ __launch_bounds__(kPrepThreads) void compact_kernel(int nblk, const float* __restrict__ gt, Box m,
                                                               const int* __restrict__ blkoff,
                                                               const float* __restrict__ src, int h, int w, int is_disp,
                                                               float clamp_lo, float* __restrict__ gtc,
                                                               float* __restrict__ prc) {
  __shared__ int red[kPrepThreads / kWave];
  const int i = blockIdx.x / nblk, b = blockIdx.x - i * nblk;
  const int p0 = b * kTile + threadIdx.x * kPer;
  float v[kPer];
  const unsigned bits = p0 < m.hw ? mask8(gt + (long long)i * m.hw, m, p0, v) : 0u;
  int total;
  int slot = block_excl_scan<kPrepThreads>(__builtin_popcount(bits), red, &total);
  if (!bits) return;
  const long long base = (long long)i * m.hw + blkoff[blockIdx.x];
  const float* img = src + (long long)i * h * w;
  const float sy = (float)h / (float)m.H, sx = (float)w / (float)m.W;
  int r = p0 / m.W, c = p0 - r * m.W;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (bits >> j & 1u) {
      float p = img[(long long)nearest(r, sy, h) * w + nearest(c, sx, w)];
      if (is_disp) p = 1.0f / p;
      gtc[base + slot] = v[j];
      prc[base + slot] = clampf(p, clamp_lo, m.hi);
      ++slot;
    }
    if (++c == m.W) c = 0, ++r;
  }
}

// ---- select + metrics ----

// The k-th smallest (0-based) of a[0..n), none of them NaN: most significant digit first, an LDS histogram per digit
// over the elements whose higher digits match the prefix found so far.
__device__ float kth(const float* __restrict__ a, int n, int k, unsigned* hist, int* ired, int* pick) {
  unsigned prefix = 0, pmask = 0;
  int shift = 32;
  while (shift > 0) {
    const int d = shift >= kDigit ? kDigit : shift;
    shift -= d;
    const unsigned dmask = (1u << d) - 1;
    __syncthreads();
    for (int j = threadIdx.x; j < kBins; j += kSel) hist[j] = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += kSel) {
      const unsigned key = to_key(a[j]);
      if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & dmask], 1u);
    }
    __syncthreads();
    int loc[kBinsPerThread], s = 0;
#pragma unroll
    for (int q = 0; q < kBinsPerThread; ++q) s += loc[q] = (int)hist[threadIdx.x * kBinsPerThread + q];
    int total;
    int below = block_excl_scan<kSel>(s, ired, &total);
#pragma unroll
    for (int q = 0; q < kBinsPerThread; ++q) {
      if (below <= k && k < below + loc[q]) {
        pick[0] = threadIdx.x * kBinsPerThread + q;
        pick[1] = below;
      }
      below += loc[q];
    }
    __syncthreads();
    prefix |= (unsigned)pick[0] << shift;
    pmask |= dmask << shift;
    k -= pick[1];
  }
  return from_key(prefix);
}

__global__ __launch_bounds__(kSel) void select_kernel(long long hw, const int* __restrict__ count,
                                                      const float* __restrict__ gtc, const float* __restrict__ prc,
                                                      double* __restrict__ metrics, float* __restrict__ medians) {
  __shared__ unsigned hist[kBins];
  __shared__ double dred[kSel / kWave];
  __shared__ int ired[kSel / kWave];
  __shared__ int pick[2];
  const int i = blockIdx.x;
  const int n = count[i];
  const float* g = gtc + i * hw;
  const float* p = prc + i * hw;

  // the valid GT lies inside (min_gt, max_depth) and holds no NaN; the clamped prediction may
  int nans = 0;
  for (int j = threadIdx.x; j < n; j += kSel) nans += p[j] != p[j];
  nans = block_sum<kSel>(nans, ired);
  const float fnan = __builtin_nanf("");
  float mg = fnan, mp = fnan;
  if (n > 0) {  // (workgroup-uniform, as is nans)
    mg = kth(g, n, (n - 1) / 2, hist, ired, pick);
    if (nans == 0) mp = kth(p, n, (n - 1) / 2, hist, ired, pick);
  }
  if (threadIdx.x == 0) medians[i * 2] = mg, medians[i * 2 + 1] = mp;
  if (n == 0 || nans > 0) {  // torch.median of nothing, or of anything with a NaN in it, is NaN: so is every metric
    if (threadIdx.x < 6) metrics[i * 6 + threadIdx.x] = __builtin_nan("");
    return;
  }

  double acc[3] = {0.0, 0.0, 0.0};
  int a1 = 0, a2 = 0, a3 = 0;
  for (int j = threadIdx.x; j < n; j += kSel) {
    const float gv = g[j];
    const float pv = (p[j] * mg) / mp;
    const float d = gv - pv;
    const float e = fabsf(d);
    acc[0] += (double)e;
    acc[1] += (double)(e / gv);
    acc[2] += (double)((d * d) / gv);
    const float t1 = gv / pv, t2 = pv / gv;
    const float t = (t1 != t1 || t1 > t2) ? t1 : t2;  // torch.max: a NaN wins
    a1 += t < 1.25f;
    a2 += t < 1.5625f;
    a3 += t < 1.953125f;
  }
  double sums[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) sums[q] = block_sum<kSel>(acc[q], dred);
  a1 = block_sum<kSel>(a1, ired);
  a2 = block_sum<kSel>(a2, ired);
  a3 = block_sum<kSel>(a3, ired);
  if (threadIdx.x == 0) {
    const double dn = (double)n;
    double* o = metrics + i * 6;
    o[0] = sums[0] / dn;
    o[1] = sums[1] / dn;
    o[2] = sums[2] / dn;
    o[3] = (double)a1 / dn;
    o[4] = (double)a2 / dn;
    o[5] = (double)a3 / dn;
  }
}

inline int ceil_div(long long a, int b) { return (int)((a + b - 1) / b); }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Layout {
  size_t blkcnt, blkoff, gtc, prc, bytes;
};

inline bool layout(int B, int H, int W, Layout* L) {
  if (B <= 0 || H <= 0 || W <= 0) return false;
  const long long hw = (long long)H * W;
  if (hw >= (1ll << 31) || hw * B >= (1ll << 31)) return false;
  const size_t nb = (size_t)B * ceil_div(hw, kTile), total = (size_t)(hw * B);
  L->blkcnt = 0;
  L->blkoff = align256(nb * sizeof(int));
  L->gtc = L->blkoff + align256(nb * sizeof(int));
  L->prc = L->gtc + align256(total * sizeof(float));
  L->bytes = L->prc + align256(total * sizeof(float));
  return true;
}

}  // namespace

extern "C" {

int scsfm_val_abi_version(void) { return 2; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_val_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

size_t scsfm_val_workspace_bytes(int B, int H, int W) {
  Layout L;
  return layout(B, H, W, &L) ? L.bytes : 0;
}

int scsfm_val_depth_errors(int B, int h, int w, const float* src, int src_is_disp, int H, int W, const float* gt,
                           int y1, int y2, int x1, int x2, float min_gt, float max_depth, float clamp_lo,
                           void* workspace, size_t workspace_bytes, double* metrics, float* medians, int* count,
                           void* stream) {
  Layout L;
  if (!layout(B, H, W, &L) || h <= 0 || w <= 0 || (long long)h * w * B >= (1ll << 31) || y1 < 0 || y1 > y2 ||
      y2 > H || x1 < 0 || x1 > x2 || x2 > W || !(min_gt < max_depth) || !src || !gt || !workspace ||
      workspace_bytes < L.bytes || !metrics || !medians || !count)
    return SCSFM_VAL_ERR_ARG;
  char* ws = static_cast<char*>(workspace);
  int* blkcnt = reinterpret_cast<int*>(ws + L.blkcnt);
  int* blkoff = reinterpret_cast<int*>(ws + L.blkoff);
  float* gtc = reinterpret_cast<float*>(ws + L.gtc);
  float* prc = reinterpret_cast<float*>(ws + L.prc);
  hipStream_t s = (hipStream_t)stream;
  Box m;
  m.H = H, m.W = W, m.hw = H * W, m.y1 = y1, m.y2 = y2, m.x1 = x1, m.x2 = x2, m.lo = min_gt, m.hi = max_depth;
  const int nblk = ceil_div(m.hw, kTile);
  (void)hipGetLastError();
  hipLaunchKernelGGL(count_kernel, dim3(B * nblk), dim3(kPrepThreads), 0, s, nblk, gt, m, blkcnt);
  hipLaunchKernelGGL(scan_kernel, dim3(B), dim3(kPrepThreads), 0, s, nblk, blkcnt, blkoff, count);
  hipLaunchKernelGGL(compact_kernel, dim3(B * nblk), dim3(kPrepThreads), 0, s, nblk, gt, m, blkoff, src, h, w,
                     src_is_disp, clamp_lo, gtc, prc);
  hipLaunchKernelGGL(select_kernel, dim3(B), dim3(kSel), 0, s, (long long)m.hw, count, gtc, prc, metrics, medians);
  return (int)hipGetLastError();
}

}  // extern "C"
