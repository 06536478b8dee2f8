// Monocular depth evaluation (include/scsfm_eval.h): eval_depth.py's per-image loop -- inverse-depth resize to the
// ground truth's size, mask and crop, median scaling, the eight error terms -- for a whole ragged set in four launches.
//
//  count    one workgroup per 2048-pixel tile of one GT map: masks 8 consecutive pixels per lane (vector loads) and
//           stores the tile's valid count.
//  scan     one workgroup per image: exclusive scan of its tiles' counts -> each tile's first slot; the image's count.
//  compact  the count kernel's tiling again: every valid pixel's GT value and its resized prediction are stored at the
//           tile's first slot plus the pixel's rank in the tile, i.e. in pixel order.  The prediction is resized only
//           where the mask holds: nothing else is needed without visualisation.
//  select   one workgroup per image: the prediction-mean skip test, exact medians of the compacted GT and prediction
//           by radix select on order-preserving integer keys (11-bit digits, an LDS histogram of 2048 bins), the
//           ratio, then the scaled and clamped prediction's eight sums in double, thread-strided and tree-reduced.
//
// Determinism: no float atomics anywhere.  The compacted order is pixel order (a scan, not an atomic ticket), and the
// sums of an image depend only on that image's data and the workgroup size, so results are bit-identical from run to
// run and however the images are chunked into calls.  Exactness: the medians are order statistics selected on keys,
// so they are the very values np.median picks (the even case averages the two middle ones in the array's precision,
// as numpy does); floating-point contraction is off, so the resize and the error terms round as numpy's separate
// multiplies and adds do.
#include <hip/hip_runtime.h>

#include <math.h>

#include "scsfm_eval.h"

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

template <class T> struct Key;
template <> struct Key<float> { using K = unsigned; static constexpr int kBits = 32; };
template <> struct Key<double> { using K = unsigned long long; static constexpr int kBits = 64; };

// order-preserving map of a float's bits to an unsigned integer (negatives reversed below the positives)
template <class T>
__device__ inline typename Key<T>::K to_key(T v) {
  using K = typename Key<T>::K;
  K u;
  __builtin_memcpy(&u, &v, sizeof(u));
  const K top = (K)1 << (Key<T>::kBits - 1);
  return (u & top) ? (K)~u : (K)(u | top);
}
template <class T>
__device__ inline T from_key(typename Key<T>::K k) {
  using K = typename Key<T>::K;
  const K top = (K)1 << (Key<T>::kBits - 1);
  const K u = (k & top) ? (K)(k & ~top) : (K)~k;
  T v;
  __builtin_memcpy(&v, &u, sizeof(v));
  return v;
}

template <class A, class B> struct Promote { using T = double; };
template <> struct Promote<float, float> { using T = float; };

__device__ inline float lg(float x) { return logf(x); }
__device__ inline double lg(double x) { return log(x); }
__device__ inline float lg10(float x) { return log10f(x); }
__device__ inline double lg10(double x) { return log10(x); }

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

template <int NT, class T>
__device__ inline T block_min(T v, T* red) {
  constexpr int nw = NT / kWave;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  for (int d = kWave / 2; d > 0; d >>= 1) {
    const T o = __shfl_down(v, d);
    if (lane + d < kWave && o < v) v = o;
  }
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  T s = red[0];
  for (int k = 1; k < nw; ++k) s = red[k] < s ? red[k] : s;
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

struct Image {
  long long off;
  int H, W, hw, y1, y2, x1, x2;
};

__device__ inline Image image(int i, const long long* off, const int* gh, const int* gw, int crop) {
  Image m;
  m.off = off[i];
  m.H = gh[i];
  m.W = gw[i];
  m.hw = m.H * m.W;
  if (crop) {  // np.array([0.40810811 * H, 0.99189189 * H, 0.03594771 * W, 0.96405229 * W]).astype(np.int32)
    m.y1 = (int)(0.40810811 * m.H);
    m.y2 = (int)(0.99189189 * m.H);
    m.x1 = (int)(0.03594771 * m.W);
    m.x2 = (int)(0.96405229 * m.W);
  } else {
    m.y1 = 0, m.y2 = m.H, m.x1 = 0, m.x2 = m.W;
  }
  return m;
}

__device__ inline void vload8(const float* p, float v[kPer]) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}
__device__ inline void vload8(const double* p, double v[kPer]) {
#pragma unroll
  for (int k = 0; k < kPer / 2; ++k) {
    const double2 a = reinterpret_cast<const double2*>(p)[k];
    v[2 * k] = a.x, v[2 * k + 1] = a.y;
  }
}

// the lane's 8 pixels p0 .. p0+7 of image m: values into v, the mask as bits
template <class G>
__device__ inline unsigned mask8(const G* __restrict__ gt, const Image& m, int p0, G lo, G hi, G v[kPer]) {
  const G* src = gt + m.off;
  if ((m.off & 3) == 0 && p0 + kPer <= m.hw) {
    vload8(src + p0, v);
  } else {
#pragma unroll
    for (int j = 0; j < kPer; ++j) v[j] = p0 + j < m.hw ? src[p0 + j] : (G)0;
  }
  int r = p0 / m.W, c = p0 - r * m.W;
  unsigned bits = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const bool ok = p0 + j < m.hw && v[j] > lo && v[j] < hi && r >= m.y1 && r < m.y2 && c >= m.x1 && c < m.x2;
    bits |= (unsigned)ok << j;
    if (++c == m.W) c = 0, ++r;
  }
  return bits;
}

template <class G>
__global__ __launch_bounds__(kPrepThreads) void count_kernel(int nblk, const G* __restrict__ gt,
                                                             const long long* __restrict__ off,
                                                             const int* __restrict__ gh, const int* __restrict__ gw,
                                                             int crop, G lo, G hi, int* __restrict__ blkcnt) {
  __shared__ int red[kPrepThreads / kWave];
  const int i = blockIdx.x / nblk, b = blockIdx.x - i * nblk;
  const Image m = image(i, off, gh, gw, crop);
  const int p0 = b * kTile + threadIdx.x * kPer;
  int c = 0;
  if (p0 < m.hw) {
    G v[kPer];
    c = __builtin_popcount(mask8(gt, m, p0, lo, hi, v));
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

template <class P>
__device__ inline P inv(P x) { return (P)1 / (x + (P)1e-6); }

// cv2.resize(1 / (pred + 1e-6), (W, H)) (INTER_LINEAR) at the GT pixel (r, c), then 1 / (. + 1e-6).  The source
// coordinate is (d + 0.5) * scale - 0.5 with scale = 1 / (dst / src) in double, rounded to float and floored; a
// coordinate below 0 takes index 0 and weight 0, one at or past src - 1 the last index and weight 0.  The weights are
// floats; the rows are interpolated first, then the two rows, in the prediction's precision.
template <class P>
__device__ inline P resized(const P* __restrict__ img, int h, int w, int r, int c, double sy, double sx) {
  float fy = (float)((r + 0.5) * sy - 0.5), fx = (float)((c + 0.5) * sx - 0.5);
  int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
  fy -= (float)y0;
  fx -= (float)x0;
  if (y0 < 0) y0 = 0, fy = 0.f;
  if (y0 >= h - 1) y0 = h - 1, fy = 0.f;
  if (x0 < 0) x0 = 0, fx = 0.f;
  if (x0 >= w - 1) x0 = w - 1, fx = 0.f;
  const int y1 = y0 + 1 < h ? y0 + 1 : h - 1, x1 = x0 + 1 < w ? x0 + 1 : w - 1;
  const P ax0 = (P)(1.f - fx), ax1 = (P)fx, by0 = (P)(1.f - fy), by1 = (P)fy;
  const P* r0 = img + (long long)y0 * w;
  const P* r1 = img + (long long)y1 * w;
  const P h0 = inv(r0[x0]) * ax0 + inv(r0[x1]) * ax1;
  const P h1 = inv(r1[x0]) * ax0 + inv(r1[x1]) * ax1;
  return inv(h0 * by0 + h1 * by1);
}

template <class G, class P>
__global__ __launch_bounds__(kPrepThreads) void compact_kernel(
    int nblk, const G* __restrict__ gt, const long long* __restrict__ off, const int* __restrict__ gh,
    const int* __restrict__ gw, int crop, G lo, G hi, const int* __restrict__ blkoff, const P* __restrict__ pred, int h,
    int w, G* __restrict__ gtc, P* __restrict__ prc) {
  __shared__ int red[kPrepThreads / kWave];
  const int i = blockIdx.x / nblk, b = blockIdx.x - i * nblk;
  const Image m = image(i, off, gh, gw, crop);
  if (b * kTile >= m.hw) return;  // (workgroup-uniform)
  const int p0 = b * kTile + threadIdx.x * kPer;
  G v[kPer];
  const unsigned bits = p0 < m.hw ? mask8(gt, m, p0, lo, hi, v) : 0u;
  int total;
  int slot = block_excl_scan<kPrepThreads>(__builtin_popcount(bits), red, &total);
  if (!bits) return;
  const long long base = m.off + blkoff[blockIdx.x];
  const P* img = pred + (long long)i * h * w;
  const double sy = 1.0 / ((double)m.H / (double)h), sx = 1.0 / ((double)m.W / (double)w);
  int r = p0 / m.W, c = p0 - r * m.W;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (bits >> j & 1u) {
      gtc[base + slot] = v[j];
      prc[base + slot] = resized(img, h, w, r, c, sy, sx);
      ++slot;
    }
    if (++c == m.W) c = 0, ++r;
  }
}

// ---- select + metrics ----

// The key of the k-th smallest (0-based) of a[0..n): most significant digit first, an LDS histogram per digit over the
// elements whose higher digits match the prefix found so far.  *eq: how many elements carry that key; *rank: k's rank
// among them.
template <class T>
__device__ typename Key<T>::K kth_key(const T* __restrict__ a, int n, int k, unsigned* hist, int* ired, int* pick,
                                      int* eq, int* rank) {
  using K = typename Key<T>::K;
  K prefix = 0, pmask = 0;
  int shift = Key<T>::kBits, found = 0;
  while (shift > 0) {
    const int d = shift >= kDigit ? kDigit : shift;
    shift -= d;
    const K dmask = (K)((1u << d) - 1);
    __syncthreads();
    for (int j = threadIdx.x; j < kBins; j += kSel) hist[j] = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += kSel) {
      const K key = to_key(a[j]);
      if ((key & pmask) == prefix) atomicAdd(&hist[(unsigned)((key >> shift) & dmask)], 1u);
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
        pick[2] = loc[q];
      }
      below += loc[q];
    }
    __syncthreads();
    prefix |= (K)pick[0] << shift;
    pmask |= dmask << shift;
    k -= pick[1];
    found = pick[2];
  }
  *eq = found;
  *rank = k;
  return prefix;
}

// np.median(a[0..n)), n >= 1
template <class T>
__device__ T median(const T* __restrict__ a, int n, unsigned* hist, int* ired, int* pick,
                    typename Key<T>::K* kred) {
  using K = typename Key<T>::K;
  int eq, rank;
  const K k1 = kth_key(a, n, (n - 1) / 2, hist, ired, pick, &eq, &rank);
  const T v1 = from_key<T>(k1);
  if (n & 1) return v1;
  K k2 = k1;
  if (rank + 1 >= eq) {  // the upper middle element is the smallest one above v1
    K m = ~(K)0;
    for (int j = threadIdx.x; j < n; j += kSel) {
      const K key = to_key(a[j]);
      if (key > k1 && key < m) m = key;
    }
    k2 = block_min<kSel>(m, kred);
  }
  return (T)((v1 + from_key<T>(k2)) / (T)2);
}

template <class G, class P>
__global__ __launch_bounds__(kSel) void select_kernel(const P* __restrict__ pred, long long hw_pred,
                                                      const long long* __restrict__ off,
                                                      const int* __restrict__ count, const G* __restrict__ gtc,
                                                      const P* __restrict__ prc, P pmin, P pmax,
                                                      double* __restrict__ metrics, double* __restrict__ stats,
                                                      int* __restrict__ flag) {
  using R = typename Promote<G, P>::T;
  __shared__ unsigned hist[kBins];
  __shared__ double dred[kSel / kWave];
  __shared__ int ired[kSel / kWave];
  __shared__ int pick[3];
  __shared__ typename Key<G>::K gkred[kSel / kWave];
  __shared__ typename Key<P>::K pkred[kSel / kWave];
  const int i = blockIdx.x;

  // the reference skips an image whose prediction has mean exactly -1
  const P* img = pred + i * hw_pred;
  double s = 0.0;
  for (long long j = threadIdx.x; j < hw_pred; j += kSel) s += (double)img[j];
  s = block_sum<kSel>(s, dred);
  const bool skip = s / (double)hw_pred == -1.0;
  const int n = count[i];
  const double nan = __builtin_nan("");
  if (skip || n == 0) {  // (workgroup-uniform) an empty mask: np.median of nothing is NaN, so is every metric
    if (threadIdx.x < 8) metrics[i * 8 + threadIdx.x] = nan;
    if (threadIdx.x < 3) stats[i * 3 + threadIdx.x] = nan;
    if (threadIdx.x == 0) flag[i] = skip ? 0 : 1;
    return;
  }
  const G* g = gtc + off[i];
  const P* p = prc + off[i];
  const G mg = median(g, n, hist, ired, pick, gkred);
  const P mp = median(p, n, hist, ired, pick, pkred);
  const R ratio = (R)mg / (R)mp;

  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  int a1 = 0, a2 = 0, a3 = 0;
  for (int j = threadIdx.x; j < n; j += kSel) {
    const G gv = g[j];
    P pv = (P)((R)p[j] * ratio);
    if (pv < pmin) pv = pmin;
    if (pv > pmax) pv = pmax;
    const R gr = (R)gv, pr = (R)pv;
    const R t1 = gr / pr, t2 = pr / gr;
    a1 += t1 < (R)1.25 && t2 < (R)1.25;
    a2 += t1 < (R)1.5625 && t2 < (R)1.5625;
    a3 += t1 < (R)1.953125 && t2 < (R)1.953125;
    const R d = gr - pr, d2 = d * d;
    acc[0] += (double)((d < (R)0 ? -d : d) / gr);
    acc[1] += (double)(d2 / gr);
    acc[2] += (double)d2;
    const R dl = (R)lg(gv) - (R)lg(pv);
    acc[3] += (double)(dl * dl);
    const R d10 = (R)lg10(gv) - (R)lg10(pv);
    acc[4] += (double)(d10 < (R)0 ? -d10 : d10);
  }
  double sums[5];
#pragma unroll
  for (int q = 0; q < 5; ++q) sums[q] = block_sum<kSel>(acc[q], dred);
  a1 = block_sum<kSel>(a1, ired);
  a2 = block_sum<kSel>(a2, ired);
  a3 = block_sum<kSel>(a3, ired);
  if (threadIdx.x == 0) {
    const double dn = (double)n;
    double* o = metrics + i * 8;
    o[0] = sums[0] / dn;
    o[1] = sums[1] / dn;
    o[2] = sqrt(sums[2] / dn);
    o[3] = sqrt(sums[3] / dn);
    o[4] = sums[4] / dn;
    o[5] = (double)a1 / dn;
    o[6] = (double)a2 / dn;
    o[7] = (double)a3 / dn;
    stats[i * 3 + 0] = (double)ratio;
    stats[i * 3 + 1] = (double)mg;
    stats[i * 3 + 2] = (double)mp;
    flag[i] = 1;
  }
}

inline int ceil_div(long long a, int b) { return (int)((a + b - 1) / b); }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int launch_status() { return (int)hipGetLastError(); }

struct Layout {
  size_t blkcnt, blkoff, gtc, prc, bytes;
};

inline bool layout(int N, int max_hw, size_t total, int pred_f64, int gt_f64, Layout* L) {
  if (N <= 0 || max_hw <= 0 || total == 0 || total >= ((size_t)1 << 40)) return false;
  const long long nb = (long long)N * ceil_div(max_hw, kTile);
  if (nb >= (1ll << 31)) return false;
  L->blkcnt = 0;
  L->blkoff = align256(nb * sizeof(int));
  L->gtc = L->blkoff + align256(nb * sizeof(int));
  L->prc = L->gtc + align256(total * (gt_f64 ? 8 : 4));
  L->bytes = L->prc + align256(total * (pred_f64 ? 8 : 4));
  return true;
}

template <class G, class P>
int run(int N, int h, int w, const P* pred, const G* gt, const long long* off, const int* gh, const int* gw,
        int max_hw, int crop, double min_depth, double max_depth, char* ws, const Layout& L, double* metrics,
        double* stats, int* count, int* flag, hipStream_t stream) {
  const int nblk = ceil_div(max_hw, kTile);
  int* blkcnt = reinterpret_cast<int*>(ws + L.blkcnt);
  int* blkoff = reinterpret_cast<int*>(ws + L.blkoff);
  G* gtc = reinterpret_cast<G*>(ws + L.gtc);
  P* prc = reinterpret_cast<P*>(ws + L.prc);
  const G lo = (G)min_depth, hi = (G)max_depth;
  (void)hipGetLastError();
  hipLaunchKernelGGL(count_kernel<G>, dim3(N * nblk), dim3(kPrepThreads), 0, stream, nblk, gt, off, gh, gw, crop, lo,
                     hi, blkcnt);
  hipLaunchKernelGGL(scan_kernel, dim3(N), dim3(kPrepThreads), 0, stream, nblk, blkcnt, blkoff, count);
  hipLaunchKernelGGL((compact_kernel<G, P>), dim3(N * nblk), dim3(kPrepThreads), 0, stream, nblk, gt, off, gh, gw,
                     crop, lo, hi, blkoff, pred, h, w, gtc, prc);
  hipLaunchKernelGGL((select_kernel<G, P>), dim3(N), dim3(kSel), 0, stream, pred, (long long)h * w, off, count, gtc,
                     prc, (P)min_depth, (P)max_depth, metrics, stats, flag);
  return launch_status();
}

}  // namespace

extern "C" {

int scsfm_eval_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_eval_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

size_t scsfm_eval_workspace_bytes(int N, int max_hw, size_t total, int pred_f64, int gt_f64) {
  Layout L;
  return layout(N, max_hw, total, pred_f64, gt_f64, &L) ? L.bytes : 0;
}

int scsfm_eval_depth(int N, int h, int w, int pred_f64, const void* pred, int gt_f64, const void* gt,
                     const long long* gt_off, const int* gt_h, const int* gt_w, int max_hw, size_t total, int crop,
                     double min_depth, double max_depth, void* workspace, size_t workspace_bytes, double* metrics,
                     double* stats, int* count, int* flag, void* stream) {
  Layout L;
  if (!layout(N, max_hw, total, pred_f64, gt_f64, &L) || h <= 0 || w <= 0 || (long long)h * w >= (1ll << 31) ||
      !pred || !gt || !gt_off || !gt_h || !gt_w || !workspace || workspace_bytes < L.bytes || !metrics || !stats ||
      !count || !flag || !(min_depth < max_depth))
    return SCSFM_EVAL_ERR_ARG;
  char* ws = static_cast<char*>(workspace);
  hipStream_t s = (hipStream_t)stream;
#define SCSFM_EVAL_RUN(G, P)                                                                                        \
  run<G, P>(N, h, w, static_cast<const P*>(pred), static_cast<const G*>(gt), gt_off, gt_h, gt_w, max_hw, crop,       \
            min_depth, max_depth, ws, L, metrics, stats, count, flag, s)
  if (gt_f64)
    return pred_f64 ? SCSFM_EVAL_RUN(double, double) : SCSFM_EVAL_RUN(double, float);
  return pred_f64 ? SCSFM_EVAL_RUN(float, double) : SCSFM_EVAL_RUN(float, float);
#undef SCSFM_EVAL_RUN
}

}  // extern "C"
