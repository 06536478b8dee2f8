// The ResNet stem's train-mode BatchNorm + ReLU fused with the 3x3 / stride 2 / pad 1 max-pool behind it
// (include/scsfm_stem.h).  The stem's tensor is the largest activation of the net and every pass over it costs as much as
// any other; here the forward reads x twice (statistics, apply) and writes f0 once, and the backward reads x and the
// gradient of f0 twice and writes dx once -- the pooled map, its argmax and its gradient are a quarter of a pass each.
//
// Forward, launch 1: bn_stats_kernel is csrc_enc/scsfm_encoder.hip's, with its partition (C x S workgroups, S <= 64
// contiguous ranges per channel) and its summation tree, so mean / invstd / mean_lo and the running statistics come out
// with the same bits.
//
// Forward, launch 2 (stem_fwd_kernel): a plane is cut into bands of PB pooled rows (2 PB input rows) and into strips of
// V columns; a thread owns one strip of one band and walks down its rows, two input rows (one pooled row) per step.
// V = 4 (one 16-byte load and store per row, two pooled columns per strip) where W % 4 == 0 and the pointers allow, V = 2
// with scalar accesses (one pooled column per strip) otherwise.  A strip's windows need one value from outside it, the
// last ReLU output of the strip to its left: the threads of a workgroup lie side by side along the row and pass it
// through LDS (double-buffered, one barrier per step).  The horizontal fold of the odd row 2ph+1 is carried in registers
// to the next step, where it is the top row of window ph+1, so inside a band every x is loaded once; a band's first step
// re-reads the one row above it (1 / (2 PB) of the plane).  Only where a row is wider than one workgroup (V * 256
// columns) does the first thread of a later segment recompute its left neighbour from x.  The fold keeps the scan rule of
// include/scsfm_enc.h: within a row and then across rows "take the candidate if it is greater or a NaN", which is the
// row-major scan regrouped (the first maximum wins, the last NaN wins); ReLU zeros tie all the time.
//
// Backward, two launches (stem_bwd_reduce_kernel, stem_bwd_dx_kernel) over the same bands and strips, flattened so that
// consecutive threads own consecutive strips: each re-derives g' of its rows from the pooled gradient and argmax bytes
// (the pooled rows ph and ph+1, the latter carried), the gradient of f0 where there is one, and x (the ReLU mask is the
// forward's expression, entry for entry).  A strip needs the pooled column to its right as well; it is read directly
// (one more 4-byte and 1-byte load per pooled row from a cache line its neighbour fetches anyway), so the backward has no
// barriers.  The reduction leaves one fp64 pair per workgroup (at most kMaxPart per channel); every workgroup of the
// second launch adds its channel's pairs in the same order, lane by lane and then by the shuffle tree.
#include <hip/hip_runtime.h>

#include "scsfm_stem.h"

namespace scsfm_stem {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxSplit = 64;        // statistics: partial pairs per channel (csrc_enc's)
constexpr int kMaxPart = 256;        // backward: partial pairs per channel
constexpr int kTargetBlocks = 2048;  // 8 workgroups of 4 waves per CU on 256 CUs
constexpr int kUnroll = 4;           // loads in flight per thread in the statistics

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

__device__ inline int imin(int a, int b) { return a < b ? a : b; }
__device__ inline int imax(int a, int b) { return a > b ? a : b; }

// ---- the statistics pass of csrc_enc/scsfm_encoder.hip, unchanged ----------------------------------------------------
struct Geo {
  int C, HW, per, units;
};
template <int V>
__device__ inline int offset_of(const Geo& g, int c, int u) {
  const int b = u / g.per;
  return (b * g.C + c) * g.HW + (u - b * g.per) * V;
}
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

// the workgroup's sums of (a, b) -> dst[0..1], waves added in ascending order
__device__ inline void block_sum_to(double a, double b, double* __restrict__ dst) {
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
    dst[0] = ta;
    dst[1] = tb;
  }
}

// channel c's two totals from the S <= 64 pairs the statistics left, valid in lane 0 of wave 0 (call from wave 0 only)
__device__ inline void stat_totals(const double* __restrict__ part, int c, int S, double& a, double& b) {
  const int lane = threadIdx.x & (kWave - 1);
  const double* src = part + 2 * ((size_t)c * S + imin(lane, S - 1));
  a = wave_sum(lane < S ? src[0] : 0.0);
  b = wave_sum(lane < S ? src[1] : 0.0);
}

// ... from the G <= kMaxPart pairs of the backward's reduction: lane l adds pairs l, l + 64, ... and the tree the lanes
__device__ inline void part_totals(const double* __restrict__ part, int c, int G, double& a, double& b) {
  const int lane = threadIdx.x & (kWave - 1);
  double sa = 0.0, sb = 0.0;
  for (int j = lane; j < G; j += kWave) {
    const double* src = part + 2 * ((size_t)c * G + j);
    sa += src[0];
    sb += src[1];
  }
  a = wave_sum(sa);
  b = wave_sum(sb);
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
  block_sum_to(s, q, part + 2 * ((size_t)blockIdx.x * gridDim.y + blockIdx.y));
}

// ---- bands and strips ------------------------------------------------------------------------------------------------
// a plane: NB bands of PB pooled rows, Wq strips of V columns; items = B * NB bands per channel
struct Plan {
  int C, H, W, PH, PW, Wq, PB, NB, items;
};
struct Bn {
  float mean, mean_lo, invstd, ga, be;
};

// V entries of a row from column col0 on (V = 2: those inside the row, 0 for the others)
template <int V>
__device__ inline void load_row(const float* __restrict__ row, int col0, int W, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(row + col0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = col0 + j < W ? row[col0 + j] : 0.f;
  }
}
template <int V>
__device__ inline void store_row(float* __restrict__ row, int col0, int W, const float (&v)[V]) {
  if constexpr (V == 4) {
    float4 t;
    t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
    *reinterpret_cast<float4*>(row + col0) = t;
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (col0 + j < W) row[col0 + j] = v[j];
  }
}

__device__ inline float act(float x, const Bn& s) { return relu(bn_value(xhat_of(x, s.mean, s.mean_lo, s.invstd), s.ga, s.be)); }

// one candidate of the scan: taken if it is greater than the best so far, or a NaN
__device__ inline void take(float v, int at_v, float& best, int& at) {
  if (v > best || v != v) {
    best = v;
    at = at_v;
  }
}
// the scan of one row of a window: (a, b, c) at dw = 0, 1, 2, the outer two possibly outside the plane
__device__ inline void hfold(float a, bool va, float b, float c, bool vc, float& best, int& at) {
  best = -INFINITY;
  at = va ? 0 : 1;
  if (va) take(a, 0, best, at);
  take(b, 1, best, at);
  if (vc) take(c, 2, best, at);
}
// ... of the V / 2 windows of a strip; `l` is the entry left of the strip
template <int V>
__device__ inline void hfold_strip(const float (&y)[V], float l, int col0, int W, float (&best)[V / 2], int (&at)[V / 2]) {
#pragma unroll
  for (int q = 0; q < V / 2; ++q)
    hfold(q == 0 ? l : y[imax(2 * q - 1, 0)], col0 + 2 * q > 0, y[2 * q], y[2 * q + 1], col0 + 2 * q + 1 < W, best[q],
          at[q]);
}

template <int V>
__global__ __launch_bounds__(kThreads) void stem_fwd_kernel(
    Plan p, int S, int span, int rows, int segs, int groups, double inv_n, double unbias, double eps, double momentum,
    const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    const double* __restrict__ part, float* __restrict__ f0, float* __restrict__ out, unsigned char* __restrict__ arg,
    float* __restrict__ stat, float* __restrict__ running_mean, float* __restrict__ running_var,
    long long* __restrict__ num_batches_tracked) {
  constexpr int NP = V / 2;
  __shared__ float sh[3];
  __shared__ float edge[2][2][kThreads];
  const int tid = threadIdx.x;
  const int c = blockIdx.x / groups, grp = blockIdx.x - c * groups;
  if (tid < kWave) {
    double s, q;
    stat_totals(part, c, S, s, q);
    if (tid == 0) {
      const double m = s * inv_n;
      double var = q * inv_n - m * m;
      if (var < 0.0) var = 0.0;
      const float mf = (float)m, lo = (float)(m - (double)mf), is = (float)(1.0 / sqrt(var + eps));
      sh[0] = mf;
      sh[1] = is;
      sh[2] = lo;
      if (grp == 0) {
        stat[c] = mf;
        stat[p.C + c] = is;
        stat[2 * p.C + c] = lo;
        running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * m);
        running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * var * unbias);
        if (c == 0) num_batches_tracked[0] += 1;
      }
    }
  }
  __syncthreads();
  const Bn bn = {sh[0], sh[2], sh[1], gamma[c], beta[c]};

  // this thread's band and strip: `rows` bands side by side in the workgroup, or one band's segment `seg`
  const int ig = grp / segs, seg = grp - ig * segs;
  const int r = tid / span, tl = tid - r * span;
  const int strip = seg * kThreads + tl, item = ig * rows + r;
  const bool live = r < rows && item < p.items && strip < p.Wq;
  const int it = live ? item : 0, b = it / p.NB, ph0 = (it - b * p.NB) * p.PB;
  const int col0 = live ? strip * V : 0, HW = p.H * p.W;
  const size_t plane = (size_t)b * p.C + c;
  const float* xp = x + plane * HW;
  float* fp = f0 + plane * HW;
  float* op = out + plane * p.PH * p.PW;
  unsigned char* ap = arg + plane * p.PH * p.PW;
  const bool recompute_left = live && tl == 0 && strip > 0;  // a later segment's first strip

  float cb[NP];  // the fold of row 2 ph - 1, carried from step to step
  int ca[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    cb[q] = -INFINITY;
    ca[q] = 0;
  }
  int buf = 0;
  {  // the row above the band
    const int h = 2 * ph0 - 1;
    const bool on = live && h >= 0;
    float y[V] = {};
    if (on) {
      load_row<V>(xp + h * p.W, col0, p.W, y);
#pragma unroll
      for (int j = 0; j < V; ++j) y[j] = act(y[j], bn);
    }
    edge[buf][0][tid] = y[V - 1];
    __syncthreads();
    if (on) {
      float l = 0.f;
      if (tl > 0) l = edge[buf][0][tid - 1];
      else if (recompute_left) l = act(xp[h * p.W + col0 - 1], bn);
      hfold_strip<V>(y, l, col0, p.W, cb, ca);
    }
    buf ^= 1;
  }
  for (int i = 0; i < p.PB; ++i) {  // (the same trip count for every thread: one barrier per step)
    const int ph = ph0 + i, ha = 2 * ph, hb = ha + 1;
    const bool on = live && ph < p.PH, onb = on && hb < p.H;
    float ya[V] = {}, yb[V] = {};
    if (on) load_row<V>(xp + ha * p.W, col0, p.W, ya);
    if (onb) load_row<V>(xp + hb * p.W, col0, p.W, yb);
    if (on) {
#pragma unroll
      for (int j = 0; j < V; ++j) ya[j] = act(ya[j], bn);
      store_row<V>(fp + ha * p.W, col0, p.W, ya);
    }
    if (onb) {
#pragma unroll
      for (int j = 0; j < V; ++j) yb[j] = act(yb[j], bn);
      store_row<V>(fp + hb * p.W, col0, p.W, yb);
    }
    edge[buf][0][tid] = ya[V - 1];
    edge[buf][1][tid] = yb[V - 1];
    __syncthreads();
    if (on) {
      float la = 0.f, lb = 0.f;
      if (tl > 0) {
        la = edge[buf][0][tid - 1];
        lb = edge[buf][1][tid - 1];
      } else if (recompute_left) {
        la = act(xp[ha * p.W + col0 - 1], bn);
        if (onb) lb = act(xp[hb * p.W + col0 - 1], bn);
      }
      float ab[NP], bb[NP];
      int aa[NP], ba[NP];
      hfold_strip<V>(ya, la, col0, p.W, ab, aa);
      hfold_strip<V>(yb, lb, col0, p.W, bb, ba);
      float best[NP];
      int at[NP];
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        // the scan starts at the first entry of the clipped window
        best[q] = -INFINITY;
        at[q] = (ha > 0 ? 0 : 3) + (col0 + 2 * q > 0 ? 0 : 1);
        if (ha > 0) take(cb[q], ca[q], best[q], at[q]);
        take(ab[q], 3 + aa[q], best[q], at[q]);
        if (onb) take(bb[q], 6 + ba[q], best[q], at[q]);
        cb[q] = bb[q];
        ca[q] = ba[q];
      }
      const int o = ph * p.PW + strip * NP;
      if constexpr (V == 4) {
        float2 t;
        t.x = best[0]; t.y = best[1];
        *reinterpret_cast<float2*>(op + o) = t;
        *reinterpret_cast<unsigned short*>(ap + o) = (unsigned short)(at[0] | (at[1] << 8));
      } else {
        op[o] = best[0];
        ap[o] = (unsigned char)at[0];
      }
    }
    buf ^= 1;
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------
// the pooled gradient and argmax of one pooled row at the V / 2 + 1 columns a strip's entries can win; 255 names nobody
template <int V>
struct Pooled {
  float g[V / 2 + 1];
  int a[V / 2 + 1];
};
template <int V>
__device__ inline Pooled<V> load_pooled(const float* __restrict__ gp, const unsigned char* __restrict__ ap, int ph,
                                        int pw0, int PH, int PW) {
  Pooled<V> r;
#pragma unroll
  for (int q = 0; q < V / 2 + 1; ++q) {
    r.g[q] = 0.f;
    r.a[q] = 255;
  }
  if (ph < PH) {
    const int o = ph * PW + pw0;
    if constexpr (V == 4) {
      const float2 t = *reinterpret_cast<const float2*>(gp + o);
      const unsigned s = *reinterpret_cast<const unsigned short*>(ap + o);
      r.g[0] = t.x; r.g[1] = t.y;
      r.a[0] = (int)(s & 255u); r.a[1] = (int)(s >> 8);
      if (pw0 + 2 < PW) {
        r.g[2] = gp[o + 2];
        r.a[2] = ap[o + 2];
      }
    } else {
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (pw0 + q < PW) {
          r.g[q] = gp[o + q];
          r.a[q] = ap[o + q];
        }
    }
  }
  return r;
}
// acc[j] += the gradients of the windows of pooled row `t` whose winner is entry j of the input row at dh = base / 3 in
// them, in ascending pw: an even column lies in one window (dw = 1), an odd one in two (dw = 2, then dw = 0)
template <int V>
__device__ inline void route(const Pooled<V>& t, int base, float (&acc)[V]) {
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (t.a[j / 2] == base + 1 + (j & 1)) acc[j] += t.g[j / 2];
    if ((j & 1) && t.a[(j + 1) / 2] == base) acc[j] += t.g[(j + 1) / 2];
  }
}

// Calls f(offset of the row's strip in the tensor, col0, g'[V], xhat[V]) for every row of every (band, strip) in
// [w0, w1) of channel c that this thread owns.
template <int V, bool SKIP, class F>
__device__ inline void walk(const Plan& p, int c, int w0, int w1, const Bn& bn, const float* __restrict__ g_pool,
                            const float* __restrict__ g_f0, const unsigned char* __restrict__ arg,
                            const float* __restrict__ x, F&& f) {
  const int HW = p.H * p.W;
  for (int w = w0 + (int)threadIdx.x; w < w1; w += kThreads) {
    const int item = w / p.Wq, strip = w - item * p.Wq, b = item / p.NB, ph0 = (item - b * p.NB) * p.PB;
    const int ph1 = imin(p.PH, ph0 + p.PB), col0 = strip * V, pw0 = strip * (V / 2);
    const size_t plane = (size_t)b * p.C + c;
    const int base = (int)(plane * HW);
    const float* gp = g_pool + plane * p.PH * p.PW;
    const unsigned char* ap = arg + plane * p.PH * p.PW;
    Pooled<V> top = load_pooled<V>(gp, ap, ph0, pw0, p.PH, p.PW);
    for (int ph = ph0; ph < ph1; ++ph) {
      const int oa = base + 2 * ph * p.W, ob = oa + p.W;
      const bool onb = 2 * ph + 1 < p.H;
      const Pooled<V> bot = load_pooled<V>(gp, ap, ph + 1, pw0, p.PH, p.PW);
      float xa[V], xb[V] = {}, ta[V] = {}, tb[V] = {};
      load_row<V>(x + oa, col0, p.W, xa);
      if (onb) load_row<V>(x + ob, col0, p.W, xb);
      if (SKIP) {
        load_row<V>(g_f0 + oa, col0, p.W, ta);
        if (onb) load_row<V>(g_f0 + ob, col0, p.W, tb);
      }
      float pa[V] = {}, pb[V] = {}, ma[V], mb[V], ha[V], hb[V];
      route<V>(top, 3, pa);
      route<V>(top, 6, pb);
      route<V>(bot, 0, pb);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        ha[j] = xhat_of(xa[j], bn.mean, bn.mean_lo, bn.invstd);
        hb[j] = xhat_of(xb[j], bn.mean, bn.mean_lo, bn.invstd);
        const float ga = SKIP ? pa[j] + ta[j] : pa[j], gb = SKIP ? pb[j] + tb[j] : pb[j];
        ma[j] = bn_value(ha[j], bn.ga, bn.be) <= 0.f ? 0.f : ga;
        mb[j] = bn_value(hb[j], bn.ga, bn.be) <= 0.f ? 0.f : gb;
      }
      f(oa, col0, ma, ha);
      if (onb) f(ob, col0, mb, hb);
      top = bot;
    }
  }
}

// the units of work of a channel, `work` = items * Wq, split over the G workgroups of the channel
__device__ inline void work_range(int work, int G, int g, int& w0, int& w1) {
  w0 = (int)((long long)work * g / G);
  w1 = (int)((long long)work * (g + 1) / G);
}

// part[c][g] = {sum g', sum g' * xhat}
template <int V, bool SKIP>
__global__ __launch_bounds__(kThreads) void stem_bwd_reduce_kernel(
    Plan p, int G, const float* __restrict__ g_pool, const float* __restrict__ g_f0,
    const unsigned char* __restrict__ arg, const float* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ stat, double* __restrict__ part) {
  const int c = blockIdx.x / G, g = blockIdx.x - c * G;
  const Bn bn = {stat[c], stat[2 * p.C + c], stat[p.C + c], gamma[c], beta[c]};
  int w0, w1;
  work_range(p.items * p.Wq, G, g, w0, w1);
  double sb = 0.0, sg = 0.0;
  const int W = p.W;
  walk<V, SKIP>(p, c, w0, w1, bn, g_pool, g_f0, arg, x, [&](int, int col0, const float (&m)[V], const float (&xh)[V]) {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (V == 4 || col0 + j < W) {
        const double gm = (double)m[j];
        sb += gm;
        sg = fma(gm, (double)xh[j], sg);
      }
  });
  block_sum_to(sb, sg, part + 2 * (size_t)blockIdx.x);
}

template <int V, bool SKIP>
__global__ __launch_bounds__(kThreads) void stem_bwd_dx_kernel(
    Plan p, int G, double inv_n, const float* __restrict__ g_pool, const float* __restrict__ g_f0,
    const unsigned char* __restrict__ arg, const float* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ stat, const double* __restrict__ part,
    float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float sh[2];
  const int c = blockIdx.x / G, g = blockIdx.x - c * G;
  if (threadIdx.x < kWave) {
    double sb, sg;
    part_totals(part, c, G, sb, sg);
    if (threadIdx.x == 0) {
      sh[0] = (float)(sb * inv_n);
      sh[1] = (float)(sg * inv_n);
      if (g == 0) {
        dbeta[c] = (float)sb;
        dgamma[c] = (float)sg;
      }
    }
  }
  __syncthreads();
  const Bn bn = {stat[c], stat[2 * p.C + c], stat[p.C + c], gamma[c], beta[c]};
  const float mb = sh[0], mg = sh[1], k1 = bn.ga * bn.invstd;
  int w0, w1;
  work_range(p.items * p.Wq, G, g, w0, w1);
  const int W = p.W;
  walk<V, SKIP>(p, c, w0, w1, bn, g_pool, g_f0, arg, x, [&](int off, int col0, const float (&m)[V], const float (&xh)[V]) {
    float o[V];
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = ((m[j] - mb) - xh[j] * mg) * k1;
    store_row<V>(dx + off, col0, W, o);
  });
}

// ---- host ------------------------------------------------------------------------------------------------------------
inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// the entry points' shape (scsfm_enc's bn_shape_ok): >= 2 entries per channel, every element index a non-negative int
inline bool shape_ok(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return false;
  const long long n = (long long)B * H * W;
  return n >= 2 && n * C < (1ll << 31);
}
inline bool aligned(const void* p, size_t a) { return ((size_t)p & (a - 1)) == 0; }

inline Geo geometry(int B, int C, int H, int W, bool vec) {
  const int HW = H * W, per = vec ? HW / 4 : HW;
  return {C, HW, per, B * per};
}
inline int splits(int C, int units) {
  int S = ceil_div(kTargetBlocks, C);
  const int most = ceil_div(units, kThreads);
  if (S > most) S = most;
  if (S > kMaxSplit) S = kMaxSplit;
  return S < 1 ? 1 : S;
}

// how the forward lays bands and strips over workgroups
struct FwdGrid {
  int span, rows, segs, groups;
};
inline FwdGrid fwd_grid(const Plan& p) {
  FwdGrid f;
  f.span = p.Wq < kThreads ? p.Wq : kThreads;
  f.rows = kThreads / f.span;
  f.segs = ceil_div(p.Wq, kThreads);
  f.groups = ceil_div(p.items, f.rows) * f.segs;
  return f;
}
inline int bwd_groups(const Plan& p) {
  const int G = ceil_div((long long)p.items * p.Wq, kThreads);
  return G > kMaxPart ? kMaxPart : G;
}
// bands as short as the target number of workgroups allows (PB doubles until the grid fits or a band is the plane)
inline Plan plan(int B, int C, int H, int W, int V, bool forward) {
  Plan p = {C, H, W, (H - 1) / 2 + 1, (W - 1) / 2 + 1, ceil_div(W, V), 1, 0, 0};
  for (;; p.PB *= 2) {
    p.NB = ceil_div(p.PH, p.PB);
    p.items = B * p.NB;
    const long long blocks = (long long)C * (forward ? fwd_grid(p).groups : bwd_groups(p));
    if (blocks <= kTargetBlocks || p.PB >= p.PH) return p;
  }
}

inline int launch_status() { return (int)hipGetLastError(); }

}  // namespace scsfm_stem

using namespace scsfm_stem;

extern "C" {

int scsfm_stem_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_stem_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

size_t scsfm_stem_workspace_bytes(int B, int C, int H, int W) {
  if (!shape_ok(B, C, H, W)) return 0;
  return (size_t)C * kMaxPart * 2 * sizeof(double);
}

int scsfm_stem_fwd_f32(int B, int C, int H, int W, double eps, double momentum, const float* x, const float* gamma,
                       const float* beta, float* f0, float* out, unsigned char* arg, float* stat, float* running_mean,
                       float* running_var, long long* num_batches_tracked, void* ws, size_t ws_bytes, void* stream) {
  if (!shape_ok(B, C, H, W) || !(eps >= 0.0) || !(momentum >= 0.0 && momentum <= 1.0) || !x || !gamma || !beta || !f0 ||
      !out || !arg || !stat || !running_mean || !running_var || !num_batches_tracked || !ws || ((size_t)ws & 7) ||
      ws_bytes < scsfm_stem_workspace_bytes(B, C, H, W))
    return -1;
  (void)hipGetLastError();
  const double n = (double)B * H * W, inv_n = 1.0 / n, unbias = n / (n - 1.0);
  double* part = (double*)ws;
  // the statistics take scsfm_enc_bn_fwd_f32's choice of access width: the partition decides the bits
  const bool vec_stats = (H * W) % 4 == 0 && aligned(x, 16) && aligned(f0, 16);
  const Geo geo = geometry(B, C, H, W, vec_stats);
  const int S = splits(C, geo.units);
  if (vec_stats) hipLaunchKernelGGL(bn_stats_kernel<4>, dim3(C, S), dim3(kThreads), 0, (hipStream_t)stream, geo, x, part);
  else hipLaunchKernelGGL(bn_stats_kernel<1>, dim3(C, S), dim3(kThreads), 0, (hipStream_t)stream, geo, x, part);
  const bool vec = W % 4 == 0 && aligned(x, 16) && aligned(f0, 16) && aligned(out, 8) && aligned(arg, 2);
  const Plan p = plan(B, C, H, W, vec ? 4 : 2, true);
  const FwdGrid f = fwd_grid(p);
  const dim3 grid((unsigned)((long long)C * f.groups)), block(kThreads);
  if (vec)
    hipLaunchKernelGGL(stem_fwd_kernel<4>, grid, block, 0, (hipStream_t)stream, p, S, f.span, f.rows, f.segs, f.groups,
                       inv_n, unbias, eps, momentum, x, gamma, beta, part, f0, out, arg, stat, running_mean, running_var,
                       num_batches_tracked);
  else
    hipLaunchKernelGGL(stem_fwd_kernel<2>, grid, block, 0, (hipStream_t)stream, p, S, f.span, f.rows, f.segs, f.groups,
                       inv_n, unbias, eps, momentum, x, gamma, beta, part, f0, out, arg, stat, running_mean, running_var,
                       num_batches_tracked);
  return launch_status();
}

#define SCSFM_STEM_BWD(V, SKIP)                                                                                          \
  do {                                                                                                                   \
    hipLaunchKernelGGL((stem_bwd_reduce_kernel<V, SKIP>), grid, block, 0, (hipStream_t)stream, p, G, g_pool, g_f0, arg,  \
                       x, gamma, beta, stat, part);                                                                      \
    hipLaunchKernelGGL((stem_bwd_dx_kernel<V, SKIP>), grid, block, 0, (hipStream_t)stream, p, G, inv_n, g_pool, g_f0,    \
                       arg, x, gamma, beta, stat, part, dx, dgamma, dbeta);                                              \
  } while (0)

int scsfm_stem_bwd_f32(int B, int C, int H, int W, const float* g_pool, const float* g_f0, const unsigned char* arg,
                       const float* x, const float* gamma, const float* beta, const float* stat, float* dx,
                       float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
  if (!shape_ok(B, C, H, W) || !g_pool || !arg || !x || !gamma || !beta || !stat || !dx || !dgamma || !dbeta || !ws ||
      ((size_t)ws & 7) || ws_bytes < scsfm_stem_workspace_bytes(B, C, H, W))
    return -1;
  (void)hipGetLastError();
  const bool vec = W % 4 == 0 && aligned(x, 16) && aligned(dx, 16) && (!g_f0 || aligned(g_f0, 16)) &&
                   aligned(g_pool, 8) && aligned(arg, 2);
  const Plan p = plan(B, C, H, W, vec ? 4 : 2, false);
  const int G = bwd_groups(p);
  const dim3 grid((unsigned)((long long)C * G)), block(kThreads);
  const double inv_n = 1.0 / ((double)B * H * W);
  double* part = (double*)ws;
  if (vec) {
    if (g_f0) SCSFM_STEM_BWD(4, true);
    else SCSFM_STEM_BWD(4, false);
  } else {
    if (g_f0) SCSFM_STEM_BWD(2, true);
    else SCSFM_STEM_BWD(2, false);
  }
  return launch_status();
}

}  // extern "C"
