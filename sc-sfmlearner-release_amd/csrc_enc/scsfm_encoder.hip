// Memory-bound glue of the ResNet encoder (include/scsfm_enc.h): train-mode BatchNorm fused with the residual add and
// the ReLU behind it, forward and backward, and the stem's 3x3 / stride 2 / pad 1 max-pool with a one-byte argmax.
//
// BatchNorm, work split: a channel of an NCHW tensor is B runs of H*W contiguous floats.  It is cut into `units` of V
// floats (V = 4, one 16-byte access, when H*W is a multiple of 4 and the pointers are 16-byte aligned; V = 1 otherwise)
// and a grid of C x S workgroups gives every channel S contiguous ranges of units (S <= 64, chosen on the host so that
// the grid has about kTargetBlocks workgroups whatever C is).  A thread walks its range kThreads units apart, so that a
// wave's access covers 1 KiB (V = 4) of consecutive bytes, with kUnroll independent loads in flight.
//
// Each operation is two launches and no more: a reduction that leaves one fp64 pair per workgroup in the workspace
// (forward: sum x, sum x^2; backward: sum g', sum g' * xhat), and an elementwise pass whose every workgroup first adds
// the S pairs of its channel -- by the same shuffle tree, hence to the same bits in every workgroup -- and then
// streams.  Workgroup (c, 0) of the elementwise pass also stores the per-channel results (mean / invstd, the running
// statistics, dgamma / dbeta) and workgroup (0, 0) counts the batch, which is what a separate finalising launch or a
// last-workgroup ticket would do.  Every element is accumulated in fp64 (a cvt, an add and an fma per element are far
// below what the memory traffic leaves room for), so var = E[x^2] - mean^2 is formed in fp64 from fp64 sums: with a
// mean of 100 standard deviations it loses 4 of 16 digits.  The fp32 rounding of the mean would cost 100 ulp of xhat
// there, so the part it loses travels with it (stat[2*C + c]) and xhat = ((x - mean) - mean_lo) * invstd.
//
// The ReLU mask of the backward is the forward's, entry for entry: mode 1 recomputes fmaf(xhat, gamma, beta) with the
// very expression of the forward (bn_value below: explicit fmaf, nothing the compiler may contract differently) and
// tests it as ATen's threshold_backward tests the stored result (v <= 0 drops the gradient, a NaN lets it pass); mode 2
// reads the stored output, which the next convolution keeps alive anyway.
#include <hip/hip_runtime.h>

#include "scsfm_enc.h"

namespace scsfm_enc {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxSplit = 64;        // partial pairs per channel: one per lane of the wave that adds them up
constexpr int kTargetBlocks = 2048;  // 8 workgroups of 4 waves per CU on 256 CUs
constexpr int kUnroll = 4;           // loads in flight per thread in the reductions
constexpr int kUnrollEw = 2;         // ... in the elementwise passes (two or three streams each)

template <int V>
struct Pack {
  float v[V];
};
template <int V>
__device__ inline Pack<V> load(const float* __restrict__ p);
template <>
__device__ inline Pack<1> load<1>(const float* __restrict__ p) {
  return {{p[0]}};
}
template <>
__device__ inline Pack<4> load<4>(const float* __restrict__ p) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  return {{t.x, t.y, t.z, t.w}};
}
__device__ inline void store(float* __restrict__ p, const Pack<1>& a) { p[0] = a.v[0]; }
__device__ inline void store(float* __restrict__ p, const Pack<4>& a) {
  float4 t;
  t.x = a.v[0]; t.y = a.v[1]; t.z = a.v[2]; t.w = a.v[3];
  *reinterpret_cast<float4*>(p) = t;
}

__device__ inline int imin(int a, int b) { return a < b ? a : b; }
__device__ inline int imax(int a, int b) { return a > b ? a : b; }

// one channel's units: `per` units in each of its B runs, HW floats from one run to the same channel's next
struct Geo {
  int C, HW, per, units;
};
template <int V>
__device__ inline int offset_of(const Geo& g, int c, int u) {
  const int b = u / g.per;
  return (b * g.C + c) * g.HW + (u - b * g.per) * V;
}
// this workgroup's range of units [u0, u1) of channel blockIdx.x
__device__ inline void range(const Geo& g, int& u0, int& u1) {
  const long long S = gridDim.y, s = blockIdx.y;
  u0 = (int)(g.units * s / S);
  u1 = (int)(g.units * (s + 1) / S);
}

// sum over the wave by a fixed tree; the total is in lane 0
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d);
  return v;
}

// the workgroup's sums of (a, b) -> part[2 * (c * S + s)], waves added in ascending order
__device__ inline void block_sum_to(double a, double b, double* __restrict__ part) {
  __shared__ double red[2 * kWaves];
  a = wave_sum(a);
  b = wave_sum(b);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[2 * wave] = a;
    red[2 * wave + 1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ta = red[0], tb = red[1];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      ta += red[2 * w];
      tb += red[2 * w + 1];
    }
    double* dst = part + 2 * ((size_t)blockIdx.x * gridDim.y + blockIdx.y);
    dst[0] = ta;
    dst[1] = tb;
  }
}

// the channel's two totals from the S pairs the reduction left, valid in lane 0 of wave 0 (call from wave 0 only)
__device__ inline void channel_totals(const double* __restrict__ part, double& a, double& b) {
  const int lane = threadIdx.x & (kWave - 1), S = gridDim.y;
  const double* src = part + 2 * ((size_t)blockIdx.x * S + imin(lane, S - 1));
  a = wave_sum(lane < S ? src[0] : 0.0);
  b = wave_sum(lane < S ? src[1] : 0.0);
}

__device__ inline float relu(float v) { return v > 0.f ? v : (v != v ? v : 0.f); }
__device__ inline float xhat_of(float x, float mean, float mean_lo, float invstd) { return ((x - mean) - mean_lo) * invstd; }
__device__ inline float bn_value(float xh, float gamma, float beta) { return fmaf(xh, gamma, beta); }

// part[c][s] = {sum x, sum x^2} over the workgroup's range
template <int V>
__global__ __launch_bounds__(kThreads) void bn_stats_kernel(Geo geo, const float* __restrict__ x,
                                                             double* __restrict__ part) {
  const int c = blockIdx.x;
  int u0, u1;
  range(geo, u0, u1);
  double s = 0.0, q = 0.0;
  for (int u = u0 + (int)threadIdx.x; u < u1; u += kUnroll * kThreads) {
    Pack<V> p[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) p[j] = load<V>(x + offset_of<V>(geo, c, imin(u + j * kThreads, u1 - 1)));
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      if (u + j * kThreads < u1) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const double d = (double)p[j].v[k];
          s += d;
          q = fma(d, d, q);
        }
      }
    }
  }
  block_sum_to(s, q, part);
}

template <int V, int MODE>
__global__ __launch_bounds__(kThreads) void bn_apply_fwd_kernel(
    Geo geo, double inv_n, double unbias, double eps, double momentum, const float* __restrict__ x,
    const float* __restrict__ identity, const float* __restrict__ gamma, const float* __restrict__ beta,
    const double* __restrict__ part, float* __restrict__ y, float* __restrict__ stat, float* __restrict__ running_mean,
    float* __restrict__ running_var, long long* __restrict__ num_batches_tracked) {
  __shared__ float sh[3];
  const int c = blockIdx.x;
  if (threadIdx.x < kWave) {
    double s, q;
    channel_totals(part, s, q);
    if (threadIdx.x == 0) {
      const double m = s * inv_n;
      double var = q * inv_n - m * m;
      if (var < 0.0) var = 0.0;
      const float mf = (float)m, lo = (float)(m - (double)mf), is = (float)(1.0 / sqrt(var + eps));
      sh[0] = mf;
      sh[1] = is;
      sh[2] = lo;
      if (blockIdx.y == 0) {
        stat[c] = mf;
        stat[geo.C + c] = is;
        stat[2 * geo.C + c] = lo;
        running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * m);
        running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * var * unbias);
        if (c == 0) num_batches_tracked[0] += 1;
      }
    }
  }
  __syncthreads();
  const float mean = sh[0], invstd = sh[1], mean_lo = sh[2], ga = gamma[c], be = beta[c];
  int u0, u1;
  range(geo, u0, u1);
  for (int u = u0 + (int)threadIdx.x; u < u1; u += kUnrollEw * kThreads) {
    Pack<V> p[kUnrollEw], r[kUnrollEw];
    int off[kUnrollEw];
#pragma unroll
    for (int j = 0; j < kUnrollEw; ++j) {
      off[j] = offset_of<V>(geo, c, imin(u + j * kThreads, u1 - 1));
      p[j] = load<V>(x + off[j]);
      if (MODE == 2) r[j] = load<V>(identity + off[j]);
    }
#pragma unroll
    for (int j = 0; j < kUnrollEw; ++j) {
      if (u + j * kThreads < u1) {
        Pack<V> o;
#pragma unroll
        for (int k = 0; k < V; ++k) {
          float v = bn_value(xhat_of(p[j].v[k], mean, mean_lo, invstd), ga, be);
          if (MODE == 2) v += r[j].v[k];
          o.v[k] = MODE == 0 ? v : relu(v);
        }
        store(y + off[j], o);
      }
    }
  }
}

// g' of one entry: the upstream gradient where the forward's ReLU let the value through
template <int MODE>
__device__ inline float masked(float g, float xh, float ga, float be, float yv) {
  if (MODE == 1) return bn_value(xh, ga, be) <= 0.f ? 0.f : g;
  if (MODE == 2) return yv <= 0.f ? 0.f : g;
  return g;
}

// part[c][s] = {sum g', sum g' * xhat}
template <int V, int MODE>
__global__ __launch_bounds__(kThreads) void bn_bwd_reduce_kernel(Geo geo, const float* __restrict__ g,
                                                                  const float* __restrict__ x,
                                                                  const float* __restrict__ y,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta,
                                                                  const float* __restrict__ stat,
                                                                  double* __restrict__ part) {
  const int c = blockIdx.x;
  const float mean = stat[c], invstd = stat[geo.C + c], mean_lo = stat[2 * geo.C + c], ga = gamma[c], be = beta[c];
  int u0, u1;
  range(geo, u0, u1);
  double sb = 0.0, sg = 0.0;
  for (int u = u0 + (int)threadIdx.x; u < u1; u += kUnrollEw * kThreads) {
    Pack<V> pg[kUnrollEw], px[kUnrollEw], py[kUnrollEw];
#pragma unroll
    for (int j = 0; j < kUnrollEw; ++j) {
      const int off = offset_of<V>(geo, c, imin(u + j * kThreads, u1 - 1));
      pg[j] = load<V>(g + off);
      px[j] = load<V>(x + off);
      if (MODE == 2) py[j] = load<V>(y + off);
    }
#pragma unroll
    for (int j = 0; j < kUnrollEw; ++j) {
      if (u + j * kThreads < u1) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float xh = xhat_of(px[j].v[k], mean, mean_lo, invstd);
          const double gm = (double)masked<MODE>(pg[j].v[k], xh, ga, be, MODE == 2 ? py[j].v[k] : 0.f);
          sb += gm;
          sg = fma(gm, (double)xh, sg);
        }
      }
    }
  }
  block_sum_to(sb, sg, part);
}

template <int V, int MODE>
__global__ __launch_bounds__(kThreads) void bn_bwd_dx_kernel(Geo geo, double inv_n, const float* __restrict__ g,
                                                              const float* __restrict__ x, const float* __restrict__ y,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta,
                                                              const float* __restrict__ stat,
                                                              const double* __restrict__ part, float* __restrict__ dx,
                                                              float* __restrict__ d_identity, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta) {
  __shared__ float sh[2];
  const int c = blockIdx.x;
  if (threadIdx.x < kWave) {
    double sb, sg;
    channel_totals(part, sb, sg);
    if (threadIdx.x == 0) {
      sh[0] = (float)(sb * inv_n);
      sh[1] = (float)(sg * inv_n);
      if (blockIdx.y == 0) {
        dbeta[c] = (float)sb;
        dgamma[c] = (float)sg;
      }
    }
  }
  __syncthreads();
  const float mean = stat[c], invstd = stat[geo.C + c], mean_lo = stat[2 * geo.C + c], ga = gamma[c], be = beta[c];
  const float mb = sh[0], mg = sh[1], k1 = ga * invstd;
  int u0, u1;
  range(geo, u0, u1);
  for (int u = u0 + (int)threadIdx.x; u < u1; u += kUnrollEw * kThreads) {
    Pack<V> pg[kUnrollEw], px[kUnrollEw], py[kUnrollEw];
    int off[kUnrollEw];
#pragma unroll
    for (int j = 0; j < kUnrollEw; ++j) {
      off[j] = offset_of<V>(geo, c, imin(u + j * kThreads, u1 - 1));
      pg[j] = load<V>(g + off[j]);
      px[j] = load<V>(x + off[j]);
      if (MODE == 2) py[j] = load<V>(y + off[j]);
    }
#pragma unroll
    for (int j = 0; j < kUnrollEw; ++j) {
      if (u + j * kThreads < u1) {
        Pack<V> o, m;
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float xh = xhat_of(px[j].v[k], mean, mean_lo, invstd);
          m.v[k] = masked<MODE>(pg[j].v[k], xh, ga, be, MODE == 2 ? py[j].v[k] : 0.f);
          o.v[k] = ((m.v[k] - mb) - xh * mg) * k1;
        }
        store(dx + off[j], o);
        if (MODE == 2) store(d_identity + off[j], m);
      }
    }
  }
}

// one thread per pooled entry; rows of the output are walked by consecutive threads
// (static: the templates above are weak symbols, a plain kernel's host stub would be an exported one)
static __global__ __launch_bounds__(kThreads) void maxpool_fwd_kernel(int total, int H, int W, int PH, int PW,
                                                                const float* __restrict__ x, float* __restrict__ out,
                                                                unsigned char* __restrict__ arg) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int t = i / PW, pw = i - t * PW, plane = t / PH, ph = t - plane * PH;
  const int hs = 2 * ph - 1, ws = 2 * pw - 1;
  const int h0 = imax(hs, 0), h1 = imin(hs + 3, H), w0 = imax(ws, 0), w1 = imin(ws + 3, W);
  const float* src = x + (size_t)plane * H * W;
  float best = -INFINITY;
  int at = (h0 - hs) * 3 + (w0 - ws);
  for (int h = h0; h < h1; ++h)
    for (int w = w0; w < w1; ++w) {
      const float v = src[h * W + w];
      if (v > best || v != v) {
        best = v;
        at = (h - hs) * 3 + (w - ws);
      }
    }
  out[i] = best;
  arg[i] = (unsigned char)at;
}

// one thread per input entry: a gather over the windows that cover it
static __global__ __launch_bounds__(kThreads) void maxpool_bwd_kernel(int total, int H, int W, int PH, int PW,
                                                                const float* __restrict__ g,
                                                                const unsigned char* __restrict__ arg,
                                                                float* __restrict__ dx) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int t = i / W, w = i - t * W, plane = t / H, h = t - plane * H;
  const int ph0 = h / 2, ph1 = imin((h + 1) / 2, PH - 1), pw0 = w / 2, pw1 = imin((w + 1) / 2, PW - 1);
  const int base = plane * PH * PW;
  float acc = 0.f;
  for (int ph = ph0; ph <= ph1; ++ph)
    for (int pw = pw0; pw <= pw1; ++pw) {
      const int o = base + ph * PW + pw;
      if ((int)arg[o] == (h - 2 * ph + 1) * 3 + (w - 2 * pw + 1)) acc += g[o];
    }
  dx[i] = acc;
}

inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// the BatchNorm entry points' shape: >= 2 entries per channel, every element index a non-negative int
inline bool bn_shape_ok(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return false;
  const long long n = (long long)B * H * W;
  return n >= 2 && n * C < (1ll << 31);
}

inline bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

inline Geo geometry(int B, int C, int H, int W, bool vec) {
  const int HW = H * W, per = vec ? HW / 4 : HW;
  return {C, HW, per, B * per};
}

inline int splits(int C, int units) {
  int S = ceil_div(kTargetBlocks, C);
  const int most = ceil_div(units, kThreads);  // (a workgroup with less than one unit per thread helps nobody)
  if (S > most) S = most;
  if (S > kMaxSplit) S = kMaxSplit;
  return S < 1 ? 1 : S;
}

inline int launch_status() { return (int)hipGetLastError(); }

}  // namespace scsfm_enc

using namespace scsfm_enc;

#define SCSFM_ENC_BY_MODE(KERNEL, V, ...)                                                            \
  do {                                                                                               \
    if (mode == 0) hipLaunchKernelGGL((KERNEL<V, 0>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__);      \
    else if (mode == 1) hipLaunchKernelGGL((KERNEL<V, 1>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<V, 2>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__);                \
  } while (0)

extern "C" {

int scsfm_enc_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_enc_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

size_t scsfm_enc_bn_workspace_bytes(int B, int C, int H, int W) {
  if (!bn_shape_ok(B, C, H, W)) return 0;
  return (size_t)C * kMaxSplit * 2 * sizeof(double);
}

int scsfm_enc_bn_fwd_f32(int B, int C, int H, int W, int mode, double eps, double momentum, const float* x,
                         const float* identity, const float* gamma, const float* beta, float* y, float* stat,
                         float* running_mean, float* running_var, long long* num_batches_tracked, void* ws,
                         size_t ws_bytes, void* stream) {
  if (!bn_shape_ok(B, C, H, W) || mode < 0 || mode > 2 || !(eps >= 0.0) || !(momentum >= 0.0 && momentum <= 1.0) ||
      !x || (mode == 2 && !identity) || !gamma || !beta || !y || !stat || !running_mean || !running_var ||
      !num_batches_tracked || !ws || ((size_t)ws & 7) || ws_bytes < scsfm_enc_bn_workspace_bytes(B, C, H, W))
    return -1;
  (void)hipGetLastError();
  const bool vec = (H * W) % 4 == 0 && aligned16(x) && aligned16(y) && (mode != 2 || aligned16(identity));
  const Geo geo = geometry(B, C, H, W, vec);
  const dim3 grid(C, splits(C, geo.units)), block(kThreads);
  const double n = (double)B * H * W, inv_n = 1.0 / n, unbias = n / (n - 1.0);
  double* part = (double*)ws;
  if (vec) {
    hipLaunchKernelGGL(bn_stats_kernel<4>, grid, block, 0, (hipStream_t)stream, geo, x, part);
    SCSFM_ENC_BY_MODE(bn_apply_fwd_kernel, 4, geo, inv_n, unbias, eps, momentum, x, identity, gamma, beta, part, y,
                      stat, running_mean, running_var, num_batches_tracked);
  } else {
    hipLaunchKernelGGL(bn_stats_kernel<1>, grid, block, 0, (hipStream_t)stream, geo, x, part);
    SCSFM_ENC_BY_MODE(bn_apply_fwd_kernel, 1, geo, inv_n, unbias, eps, momentum, x, identity, gamma, beta, part, y,
                      stat, running_mean, running_var, num_batches_tracked);
  }
  return launch_status();
}

int scsfm_enc_bn_bwd_f32(int B, int C, int H, int W, int mode, const float* g, const float* x, const float* y,
                         const float* gamma, const float* beta, const float* stat, float* dx, float* d_identity,
                         float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
  if (!bn_shape_ok(B, C, H, W) || mode < 0 || mode > 2 || !g || !x || (mode == 2 && (!y || !d_identity)) || !gamma ||
      !beta || !stat || !dx || !dgamma || !dbeta || !ws || ((size_t)ws & 7) ||
      ws_bytes < scsfm_enc_bn_workspace_bytes(B, C, H, W))
    return -1;
  (void)hipGetLastError();
  const bool vec = (H * W) % 4 == 0 && aligned16(g) && aligned16(x) && aligned16(dx) &&
                   (mode != 2 || (aligned16(y) && aligned16(d_identity)));
  const Geo geo = geometry(B, C, H, W, vec);
  const dim3 grid(C, splits(C, geo.units)), block(kThreads);
  const double inv_n = 1.0 / ((double)B * H * W);
  double* part = (double*)ws;
  if (vec) {
    SCSFM_ENC_BY_MODE(bn_bwd_reduce_kernel, 4, geo, g, x, y, gamma, beta, stat, part);
    SCSFM_ENC_BY_MODE(bn_bwd_dx_kernel, 4, geo, inv_n, g, x, y, gamma, beta, stat, part, dx, d_identity, dgamma, dbeta);
  } else {
    SCSFM_ENC_BY_MODE(bn_bwd_reduce_kernel, 1, geo, g, x, y, gamma, beta, stat, part);
    SCSFM_ENC_BY_MODE(bn_bwd_dx_kernel, 1, geo, inv_n, g, x, y, gamma, beta, stat, part, dx, d_identity, dgamma, dbeta);
  }
  return launch_status();
}

int scsfm_enc_maxpool_fwd_f32(int B, int C, int H, int W, const float* x, float* out, unsigned char* arg, void* stream) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || !x || !out || !arg || (long long)B * C * H * W >= (1ll << 31)) return -1;
  (void)hipGetLastError();
  const int PH = (H - 1) / 2 + 1, PW = (W - 1) / 2 + 1, total = B * C * PH * PW;
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(ceil_div(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, total,
                     H, W, PH, PW, x, out, arg);
  return launch_status();
}

int scsfm_enc_maxpool_bwd_f32(int B, int C, int H, int W, const float* g, const unsigned char* arg, float* dx,
                              void* stream) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || !g || !arg || !dx || (long long)B * C * H * W >= (1ll << 31)) return -1;
  (void)hipGetLastError();
  const int PH = (H - 1) / 2 + 1, PW = (W - 1) / 2 + 1, total = B * C * H * W;
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(ceil_div(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, total,
                     H, W, PH, PW, g, arg, dx);
  return launch_status();
}

}  // extern "C"
