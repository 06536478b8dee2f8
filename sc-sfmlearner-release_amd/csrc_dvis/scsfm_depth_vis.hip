// Depth visualisation of eval_depth.py --vis_dir (include/scsfm_dvis.h).
//
//  scaled    one lane per ground-truth pixel: the inverse-depth resize of the prediction (the arithmetic of
//            csrc_eval/scsfm_eval.hip's `resized`), back to depth, widened and multiplied by the image's ratio.
//  range     one workgroup of 1024 lanes per image.  Pass 0 forms inv = 1 / (x + 1e-6), stores it in the workspace and
//            folds the minimum on order-preserving integer keys (a NaN is flagged).  The lo-th smallest key is found by
//            a radix select: 11-bit digits, most significant first, an LDS histogram of 2048 bins per digit over the
//            elements that match the prefix found so far.  hi = lo + 1 is the same key while duplicates last, otherwise
//            the smallest key above it (one more pass).  Lane 0 interpolates as numpy's _lerp does.
//  colourise pure streaming: one lane per pixel, the 768-byte table staged in LDS, three byte stores per pixel at the
//            caller's pitch.
//
// Determinism and exactness: no float atomics; the histograms count integers, so the order of arrival cannot matter;
// an image's result depends on that image alone.  Contraction is off and every `/` is the full IEEE division.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "scsfm_dvis.h"

#pragma clang fp contract(off)

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kWave = 64;
constexpr int kThreads = 256;            // scaled, colourise
constexpr int kPer = 4;                  // pixels per lane there, kThreads apart (coalesced)
constexpr int kTile = kThreads * kPer;
constexpr int kSel = 1024;               // workgroup of the range kernel
constexpr int kDigit = 11;
constexpr int kBins = 1 << kDigit;
constexpr int kBinsPerThread = kBins / kSel;
constexpr int kTable = 256;

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

template <class P>
__device__ inline P inv(P x) { return (P)1 / (x + (P)1e-6); }

// ---- (a) scaled prediction ----

// cv2.resize(1 / (pred + 1e-6), (W, H)) (INTER_LINEAR) at the GT pixel (r, c), then 1 / (. + 1e-6): see
// csrc_eval/scsfm_eval.hip.  Every index is clamped into the image.
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

template <class P, class R>
__global__ __launch_bounds__(kThreads) void scaled_kernel(int nblk, const P* __restrict__ pred, int h, int w,
                                                          const R* __restrict__ ratio,
                                                          const long long* __restrict__ off,
                                                          const int* __restrict__ gh, const int* __restrict__ gw,
                                                          R* __restrict__ out) {
  const int i = blockIdx.x / nblk, b = blockIdx.x - i * nblk;
  const int H = gh[i], W = gw[i];
  if (H < 1 || W < 1) return;
  const long long hw = (long long)H * W;
  const P* img = pred + (long long)i * h * w;
  R* o = out + off[i];
  const R k = ratio[i];
  const double sy = 1.0 / ((double)H / (double)h), sx = 1.0 / ((double)W / (double)w);
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const long long p = (long long)b * kTile + j * kThreads + threadIdx.x;
    if (p >= hw) return;
    const int r = (int)(p / W), c = (int)(p - (long long)r * W);
    o[p] = (R)resized(img, h, w, r, c, sy, sx) * k;
  }
}

// ---- (b) range ----

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

// The key of the k-th smallest (0-based) of a[0..n), none of them a NaN.  *eq: how many elements carry that key; *rank:
// k's rank among them.
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

template <class T>
__global__ __launch_bounds__(kSel) void range_kernel(const T* __restrict__ maps, const long long* __restrict__ off,
                                                     const int* __restrict__ gh, const int* __restrict__ gw,
                                                     const int* __restrict__ lo, const int* __restrict__ hi,
                                                     const T* __restrict__ tw, T* __restrict__ ws,
                                                     double* __restrict__ range) {
  using K = typename Key<T>::K;
  __shared__ unsigned hist[kBins];
  __shared__ int ired[kSel / kWave];
  __shared__ int pick[3];
  __shared__ K kred[kSel / kWave];
  const int i = blockIdx.x;
  const int H = gh[i], W = gw[i];
  const long long hw = (long long)H * W;
  if (H < 1 || W < 1 || hw >= (1ll << 31)) {  // (workgroup-uniform; the callers never pass such a size)
    if (threadIdx.x < 2) range[2 * i + threadIdx.x] = __builtin_nan("");
    return;
  }
  const int n = (int)hw;
  const T* x = maps + off[i];
  T* a = ws + off[i];

  // pass 0: the inverse depths, their minimum and whether any is a NaN
  K kmin = ~(K)0;
  int bad = 0;
  for (int j = threadIdx.x; j < n; j += kSel) {
    const T v = inv(x[j]);
    a[j] = v;
    if (v != v) {
      bad = 1;
    } else {
      const K key = to_key(v);
      kmin = key < kmin ? key : kmin;
    }
  }
  int nbad;
  (void)block_excl_scan<kSel>(bad, ired, &nbad);
  if (nbad) {  // (workgroup-uniform)
    if (threadIdx.x < 2) range[2 * i + threadIdx.x] = __builtin_nan("");
    return;
  }
  kmin = block_min<kSel>(kmin, kred);
  // (the stores of pass 0 are read by other lanes below: kth_key begins with a barrier)

  int k_lo = lo[i], k_hi = hi[i];
  k_lo = k_lo < 0 ? 0 : (k_lo > n - 1 ? n - 1 : k_lo);
  k_hi = k_hi < k_lo ? k_lo : (k_hi > n - 1 ? n - 1 : k_hi);
  int eq, rank;
  const K ka = kth_key(a, n, k_lo, hist, ired, pick, &eq, &rank);
  K kb = ka;
  if (k_hi > k_lo && rank + (k_hi - k_lo) >= eq) {  // (workgroup-uniform)
    if (k_hi == k_lo + 1) {  // the smallest key above ka
      K m = ~(K)0;
      for (int j = threadIdx.x; j < n; j += kSel) {
        const K key = to_key(a[j]);
        if (key > ka && key < m) m = key;
      }
      kb = block_min<kSel>(m, kred);
    } else {
      kb = kth_key(a, n, k_hi, hist, ired, pick, &eq, &rank);
    }
  }
  if (threadIdx.x == 0) {
    const T va = from_key<T>(ka), vb = from_key<T>(kb), t = tw[i];
    const T d = vb - va;
    const T vmax = t < (T)0.5 ? (T)(va + d * t) : (T)(vb - d * ((T)1 - t));
    range[2 * i] = (double)from_key<T>(kmin);
    range[2 * i + 1] = (double)vmax;
  }
}

// ---- (c) colourise ----

template <class T>
__global__ __launch_bounds__(kThreads) void colourise_kernel(int nblk, const T* __restrict__ maps,
                                                             const long long* __restrict__ off,
                                                             const int* __restrict__ gh, const int* __restrict__ gw,
                                                             const double* __restrict__ range,
                                                             const unsigned char* __restrict__ table,
                                                             unsigned char* __restrict__ out,
                                                             const long long* __restrict__ out_off,
                                                             const int* __restrict__ out_pitch) {
  __shared__ unsigned char tab[3 * kTable];
  for (int j = threadIdx.x; j < 3 * kTable; j += kThreads) tab[j] = table[j];
  __syncthreads();
  const int i = blockIdx.x / nblk, b = blockIdx.x - i * nblk;
  const int H = gh[i], W = gw[i];
  if (H < 1 || W < 1) return;
  const long long hw = (long long)H * W;
  const T* x = maps + off[i];
  unsigned char* o = out + out_off[i];
  const long long pitch = out_pitch[i];
  const double vmin = range[2 * i], vmax = range[2 * i + 1];
  const bool flat = vmin == vmax;
  const double span = vmax - vmin;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const long long p = (long long)b * kTile + j * kThreads + threadIdx.x;
    if (p >= hw) return;
    const int r = (int)(p / W), c = (int)(p - (long long)r * W);
    T v = (T)0;
    if (!flat) {
      v = (T)((double)inv(x[p]) - vmin);
      v = (T)((double)v / span);
    }
    const T xa = v * (T)kTable;
    const bool nan = xa != xa;
    int idx = xa >= (T)kTable ? kTable - 1 : (int)(xa > (T)0 ? xa : (T)0);  // (a NaN fails both: entry 0, not used)
    idx = idx < 0 ? 0 : (idx > kTable - 1 ? kTable - 1 : idx);
    unsigned char* px = o + r * pitch + 3ll * c;
    px[0] = nan ? (unsigned char)0 : tab[3 * idx];
    px[1] = nan ? (unsigned char)0 : tab[3 * idx + 1];
    px[2] = nan ? (unsigned char)0 : tab[3 * idx + 2];
  }
}

inline int ceil_div(long long a, int b) { return (int)((a + b - 1) / b); }
inline int launch_status() { return (int)hipGetLastError(); }
inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool flag(int f) { return f == 0 || f == 1; }
// blocks per image and in all; false when the grid would not fit
inline bool grid(int N, int max_hw, int* nblk, unsigned* blocks) {
  *nblk = ceil_div(max_hw, kTile);
  const long long nb = (long long)N * *nblk;
  *blocks = (unsigned)nb;
  return nb < (1ll << 31);
}

}  // namespace

extern "C" {

int scsfm_dvis_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_dvis_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

int scsfm_dvis_scaled_depth(int N, int h, int w, int pred_f64, const void* pred, int out_f64, const void* ratio,
                            const long long* off, const int* gh, const int* gw, int max_hw, void* out, void* stream) {
  int nblk;
  unsigned blocks;
  if (N < 1 || h < 1 || w < 1 || (long long)h * w >= (1ll << 31) || max_hw < 1 || !flag(pred_f64) || !flag(out_f64) ||
      (pred_f64 && !out_f64) || !pred || !ratio || !off || !gh || !gw || !out || !grid(N, max_hw, &nblk, &blocks))
    return SCSFM_DVIS_ERR_ARG;
  if (!aligned(pred, pred_f64 ? 8 : 4) || !aligned(ratio, out_f64 ? 8 : 4) || !aligned(out, out_f64 ? 8 : 4) ||
      !aligned(off, 8) || !aligned(gh, 4) || !aligned(gw, 4))
    return SCSFM_DVIS_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError();
#define SCSFM_DVIS_SCALED(P, R)                                                                                      \
  hipLaunchKernelGGL((scaled_kernel<P, R>), dim3(blocks), dim3(kThreads), 0, s, nblk, static_cast<const P*>(pred), h, \
                     w, static_cast<const R*>(ratio), off, gh, gw, static_cast<R*>(out))
  if (pred_f64) {
    SCSFM_DVIS_SCALED(double, double);
  } else if (out_f64) {
    SCSFM_DVIS_SCALED(float, double);
  } else {
    SCSFM_DVIS_SCALED(float, float);
  }
#undef SCSFM_DVIS_SCALED
  return launch_status();
}

size_t scsfm_dvis_range_workspace_bytes(size_t total, int f64) {
  if (total == 0 || total >= ((size_t)1 << 40) || !flag(f64)) return 0;
  return (total * (f64 ? 8 : 4) + 255) & ~(size_t)255;
}

int scsfm_dvis_range(int N, int f64, const void* maps, const long long* off, const int* gh, const int* gw,
                     size_t total, const int* lo, const int* hi, const void* t, void* workspace,
                     size_t workspace_bytes, double* range, void* stream) {
  const size_t need = scsfm_dvis_range_workspace_bytes(total, f64);
  if (N < 1 || !flag(f64) || need == 0 || !maps || !off || !gh || !gw || !lo || !hi || !t || !workspace ||
      workspace_bytes < need || !range)
    return SCSFM_DVIS_ERR_ARG;
  const uintptr_t el = f64 ? 8 : 4;
  if (!aligned(maps, el) || !aligned(t, el) || !aligned(workspace, el) || !aligned(range, 8) || !aligned(off, 8) ||
      !aligned(gh, 4) || !aligned(gw, 4) || !aligned(lo, 4) || !aligned(hi, 4))
    return SCSFM_DVIS_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError();
  if (f64) {
    hipLaunchKernelGGL(range_kernel<double>, dim3(N), dim3(kSel), 0, s, static_cast<const double*>(maps), off, gh, gw,
                       lo, hi, static_cast<const double*>(t), static_cast<double*>(workspace), range);
  } else {
    hipLaunchKernelGGL(range_kernel<float>, dim3(N), dim3(kSel), 0, s, static_cast<const float*>(maps), off, gh, gw, lo,
                       hi, static_cast<const float*>(t), static_cast<float*>(workspace), range);
  }
  return launch_status();
}

int scsfm_dvis_colourise(int N, int f64, const void* maps, const long long* off, const int* gh, const int* gw,
                         int max_hw, const double* range, const unsigned char* table, unsigned char* out,
                         const long long* out_off, const int* out_pitch, void* stream) {
  int nblk;
  unsigned blocks;
  if (N < 1 || !flag(f64) || max_hw < 1 || !maps || !off || !gh || !gw || !range || !table || !out || !out_off ||
      !out_pitch || !grid(N, max_hw, &nblk, &blocks))
    return SCSFM_DVIS_ERR_ARG;
  if (!aligned(maps, f64 ? 8 : 4) || !aligned(range, 8) || !aligned(off, 8) || !aligned(out_off, 8) ||
      !aligned(gh, 4) || !aligned(gw, 4) || !aligned(out_pitch, 4))
    return SCSFM_DVIS_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  (void)hipGetLastError();
  if (f64) {
    hipLaunchKernelGGL(colourise_kernel<double>, dim3(blocks), dim3(kThreads), 0, s, nblk,
                       static_cast<const double*>(maps), off, gh, gw, range, table, out, out_off, out_pitch);
  } else {
    hipLaunchKernelGGL(colourise_kernel<float>, dim3(blocks), dim3(kThreads), 0, s, nblk,
                       static_cast<const float*>(maps), off, gh, gw, range, table, out, out_off, out_pitch);
  }
  return launch_status();
}

}  // extern "C"
