// The depth decoder's fused glue with the bias of the convolution in front of it folded in (include/scsfm_decb.h).
//
// The convolutions of DepthDecoder run without their bias.  What ATen does for a biased MIOpen convolution -- a
// broadcast add over the whole output after the forward, grad_output.sum((0, 2, 3)) over the whole gradient in the
// backward -- rides here on the glue kernels that touch every one of those elements anyway: the forward adds bias[c]
// (wave-uniform) in front of the ELU or the sigmoid, the backward sums what it stores.
//
// Work split, fold order, child order and ELU-gradient form are those of csrc_nets/scsfm_decoder.hip, restated here
// so that libscsfm_nets.so stays what it is: a wave owns one segment of kChunk = 256 consecutive elements of one row,
// a lane handles kPer = 4 of them, 64 apart; row, plane and channel are wave-uniform.  The activation gradients are
// bit for bit those of scsfm_nets_pad_bwd_f32(elu = 1) / scsfm_nets_up_cat_pad_bwd_f32.
//
// Bias sum (the house rule of csrc_enc/scsfm_encoder.hip): every lane adds the values it stores in fp64, j = 0..3 in
// order, a masked lane adds 0; the wave adds its lanes by the fixed shuffle tree and lane 0 stores one fp64 partial per
// segment in ws[seg]; bias_sum_kernel, one workgroup per channel, then adds the channel's B * per partials in a fixed
// order (thread t takes partials t, t + 256, ..., then the tree, then the four waves in ascending order) and rounds
// once to fp32.  No floating-point atomics, no grid barrier, no ticket: the same input gives the same bits.
//
// Disparity head: each step is one fp32 operation in the order of ATen's chain (conv + bias, sigmoid, mul, add), so no
// multiply and add may be contracted into an fma anywhere in this file.
#include <hip/hip_runtime.h>

#include "scsfm_decb.h"

#pragma clang fp contract(off)

namespace scsfm_decb {

constexpr int kWave = 64;
constexpr int kWaves = 4;  // per workgroup
constexpr int kPer = 4;    // elements per lane
constexpr int kChunk = kWave * kPer;
constexpr int kThreads = kWave * kWaves;

__device__ inline int imin(int a, int b) { return a < b ? a : b; }
__device__ inline int refl(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
__device__ inline float elu(float x) { return x > 0.f ? x : expm1f(x); }
__device__ inline float elu_grad(float g, float r) { return r <= 0.f ? g * (r + 1.f) : g; }

// this wave's segment (wave-uniform) and lane; false when the wave has no segment
__device__ inline bool segment(int nseg, int& seg, int& lane) {
  seg = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
  lane = threadIdx.x & (kWave - 1);
  return seg < nseg;
}

// the reflection-pad backward of entry (y, x) of an H x W plane from its padded gradient g, in the order of
// csrc_nets/scsfm_decoder.hip: 0 + g[y+1][x+1] (= in), + g[y+1][0] if x == 1, + g[y+1][W+1] if x == W-2, then the same
// three steps for padded row 0 if y == 1 and for padded row H+1 if y == H-2
__device__ inline float fold(const float* __restrict__ g, int Wp, int H, int W, int y, int x, float in) {
  float acc = 0.f;
  acc += in;
  const float* r = g + (y + 1) * Wp;
  if (x == 1) acc += r[0];
  if (x == W - 2) acc += r[W + 1];
  auto row = [&](const float* r) {
    acc += r[x + 1];
    if (x == 1) acc += r[0];
    if (x == W - 2) acc += r[W + 1];
  };
  if (y == 1) row(g);
  if (y == H - 2) row(g + (H + 1) * Wp);
  return acc;
}

// sum over the wave by a fixed tree; the total is in lane 0
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d);
  return v;
}

// the wave's partial of segment seg: every lane takes part (masked lanes bring 0)
__device__ inline void store_partial(double s, int seg, int lane, double* __restrict__ ws) {
  s = wave_sum(s);
  if (lane == 0) ws[seg] = s;
}

// (the kernels that are no templates are static: the library exports the C ABI of its header and nothing else)
// out[plane][p][q] = R(E(x + bias[c]))[plane][p][q]; rows = planes * (H+2)
static __global__ __launch_bounds__(kThreads) void bias_elu_pad_fwd_kernel(int nseg, int nchunk, int C, int H, int W,
                                                                            const float* __restrict__ x,
                                                                            const float* __restrict__ bias,
                                                                            float* __restrict__ out) {
  int seg, lane;
  if (!segment(nseg, seg, lane)) return;
  const int Hp = H + 2, Wp = W + 2;
  const int row = seg / nchunk, q0 = (seg - row * nchunk) * kChunk + lane;
  const int plane = row / Hp, p = row - plane * Hp;
  const float bc = bias[plane % C];
  const float* src = x + (plane * H + refl(p - 1, H)) * W;
  float* dst = out + row * Wp;
  float v[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) v[j] = src[refl(imin(q0 + j * kWave, Wp - 1) - 1, W)];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int q = q0 + j * kWave;
    if (q < Wp) dst[q] = elu(v[j] + bc);
  }
}

// out[b][c][p][q] = R(cat[U(E(a + bias[c])), skip]); rows = B * (Ca+Cs) * (2H+2)
static __global__ __launch_bounds__(kThreads) void bias_up_cat_pad_fwd_kernel(int nseg, int nchunk, int Ca, int Cs,
                                                                               int H, int W,
                                                                               const float* __restrict__ a,
                                                                               const float* __restrict__ bias,
                                                                               const float* __restrict__ skip,
                                                                               float* __restrict__ out) {
  int seg, lane;
  if (!segment(nseg, seg, lane)) return;
  const int H2 = 2 * H, W2 = 2 * W, Hp = H2 + 2, Wp = W2 + 2, Ct = Ca + Cs;
  const int row = seg / nchunk, q0 = (seg - row * nchunk) * kChunk + lane;
  const int plane = row / Hp, p = row - plane * Hp;
  const int b = plane / Ct, c = plane - b * Ct;
  const int Y = refl(p - 1, H2);
  float* dst = out + row * Wp;
  float v[kPer];
  if (c < Ca) {
    const float bc = bias[c];
    const float* src = a + ((b * Ca + c) * H + (Y >> 1)) * W;
#pragma unroll
    for (int j = 0; j < kPer; ++j) v[j] = src[refl(imin(q0 + j * kWave, Wp - 1) - 1, W2) >> 1];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int q = q0 + j * kWave;
      if (q < Wp) dst[q] = elu(v[j] + bc);
    }
  } else {
    const float* src = skip + ((b * Cs + (c - Ca)) * H2 + Y) * W2;
#pragma unroll
    for (int j = 0; j < kPer; ++j) v[j] = src[refl(imin(q0 + j * kWave, Wp - 1) - 1, W2)];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int q = q0 + j * kWave;
      if (q < Wp) dst[q] = v[j];
    }
  }
}

// g_x[plane][y][x] = E'(r) * fold(gp)[y][x]; rows = planes * H; SUM: ws[seg] = the segment's sum of g_x
template <bool SUM>
__global__ __launch_bounds__(kThreads) void bias_elu_pad_bwd_kernel(int nseg, int nchunk, int H, int W,
                                                                     const float* __restrict__ gp,
                                                                     const float* __restrict__ out,
                                                                     float* __restrict__ g_x, double* __restrict__ ws) {
  int seg, lane;
  if (!segment(nseg, seg, lane)) return;
  const int Hp = H + 2, Wp = W + 2;
  const int row = seg / nchunk, x0 = (seg - row * nchunk) * kChunk + lane;
  const int plane = row / H, y = row - plane * H;
  const float* g = gp + plane * Hp * Wp;
  const int ro = (y + 1) * Wp + 1;  // (interior offset of row y)
  float v[kPer], r[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int x = imin(x0 + j * kWave, W - 1);
    v[j] = g[ro + x];
    r[j] = out[plane * Hp * Wp + ro + x];
  }
  float* dst = g_x + row * W;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int x = x0 + j * kWave;
    const float f = elu_grad(fold(g, Wp, H, W, y, imin(x, W - 1), v[j]), r[j]);
    if (x < W) dst[x] = f;
    if (SUM) s += x < W ? (double)f : 0.0;
  }
  if (SUM) store_partial(s, seg, lane, ws);
}

// the first B*Ca*H rows: g_a[b][c][y][x] = E'(r) * sum of the four folded children (2y|2y+1, 2x|2x+1), row-major;
// the next B*Cs*2H rows: g_skip[b][c][Y][X] = fold(gp[b][Ca+c])[Y][X]; SUM: ws[seg] = the segment's sum of g_a
template <bool SUM>
__global__ __launch_bounds__(kThreads) void bias_up_cat_pad_bwd_kernel(int nseg_a, int nchunk_a, int nseg, int nchunk_s,
                                                                        int Ca, int Cs, int H, int W,
                                                                        const float* __restrict__ gp,
                                                                        const float* __restrict__ out,
                                                                        float* __restrict__ g_a,
                                                                        float* __restrict__ g_skip,
                                                                        double* __restrict__ ws) {
  int seg, lane;
  if (!segment(nseg, seg, lane)) return;
  const int H2 = 2 * H, W2 = 2 * W, Hp = H2 + 2, Wp = W2 + 2, Ct = Ca + Cs;
  if (seg < nseg_a) {
    const int row = seg / nchunk_a, x0 = (seg - row * nchunk_a) * kChunk + lane;
    const int plane = row / H, y = row - plane * H;
    const int b = plane / Ca, c = plane - b * Ca;
    const float* g = gp + (b * Ct + c) * Hp * Wp;
    const int ro = (2 * y + 1) * Wp + 1;  // (interior offset of child row 2y; 2y+1 follows at + Wp)
    float v[kPer][4], r[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int x = imin(x0 + j * kWave, W - 1);
      v[j][0] = g[ro + 2 * x];
      v[j][1] = g[ro + 2 * x + 1];
      v[j][2] = g[ro + Wp + 2 * x];
      v[j][3] = g[ro + Wp + 2 * x + 1];
      r[j] = out[(b * Ct + c) * Hp * Wp + ro + 2 * x];
    }
    float* dst = g_a + row * W;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int x = x0 + j * kWave, xc = imin(x, W - 1);
      float acc = 0.f;
      acc += fold(g, Wp, H2, W2, 2 * y, 2 * xc, v[j][0]);
      acc += fold(g, Wp, H2, W2, 2 * y, 2 * xc + 1, v[j][1]);
      acc += fold(g, Wp, H2, W2, 2 * y + 1, 2 * xc, v[j][2]);
      acc += fold(g, Wp, H2, W2, 2 * y + 1, 2 * xc + 1, v[j][3]);
      const float f = elu_grad(acc, r[j]);
      if (x < W) dst[x] = f;
      if (SUM) s += x < W ? (double)f : 0.0;
    }
    if (SUM) store_partial(s, seg, lane, ws);
  } else {
    seg -= nseg_a;
    const int row = seg / nchunk_s, x0 = (seg - row * nchunk_s) * kChunk + lane;
    const int plane = row / H2, Y = row - plane * H2;
    const int b = plane / Cs, c = plane - b * Cs;
    const float* g = gp + (b * Ct + Ca + c) * Hp * Wp;
    const int ro = (Y + 1) * Wp + 1;
    float v[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) v[j] = g[ro + imin(x0 + j * kWave, W2 - 1)];
    float* dst = g_skip + row * W2;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int x = x0 + j * kWave;
      const float f = fold(g, Wp, H2, W2, Y, imin(x, W2 - 1), v[j]);
      if (x < W2) dst[x] = f;
    }
  }
}

// a plane of the head is one row of N = H*W elements: y = 1 / (1 + expf(-(x + bias[c]))), out = alpha * y + beta
static __global__ __launch_bounds__(kThreads) void disp_head_fwd_kernel(int nseg, int nchunk, int C, int N,
                                                                         const float* __restrict__ x,
                                                                         const float* __restrict__ bias, float alpha,
                                                                         float beta, float* __restrict__ y,
                                                                         float* __restrict__ out) {
  int seg, lane;
  if (!segment(nseg, seg, lane)) return;
  const int plane = seg / nchunk, i0 = (seg - plane * nchunk) * kChunk + lane;
  const float bc = bias[plane % C];
  const float* src = x + plane * N;
  float v[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) v[j] = src[imin(i0 + j * kWave, N - 1)];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = i0 + j * kWave;
    const float s = 1.f / (1.f + expf(-(v[j] + bc)));
    const float m = alpha * s;
    if (i < N) {
      y[plane * N + i] = s;
      out[plane * N + i] = m + beta;
    }
  }
}

// g_x = ((g_out * alpha) * (1 - y)) * y; SUM: ws[seg] = the segment's sum of g_x
template <bool SUM>
__global__ __launch_bounds__(kThreads) void disp_head_bwd_kernel(int nseg, int nchunk, int N, float alpha,
                                                                  const float* __restrict__ g_out,
                                                                  const float* __restrict__ y, float* __restrict__ g_x,
                                                                  double* __restrict__ ws) {
  int seg, lane;
  if (!segment(nseg, seg, lane)) return;
  const int plane = seg / nchunk, i0 = (seg - plane * nchunk) * kChunk + lane;
  float g[kPer], s[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = plane * N + imin(i0 + j * kWave, N - 1);
    g[j] = g_out[i];
    s[j] = y[i];
  }
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = i0 + j * kWave;
    const float f = ((g[j] * alpha) * (1.f - s[j])) * s[j];
    if (i < N) g_x[plane * N + i] = f;
    if (SUM) sum += i < N ? (double)f : 0.0;
  }
  if (SUM) store_partial(sum, seg, lane, ws);
}

// g_bias[c] = the sum of channel c's partials: plane (b, c) owns ws[(b*C + c) * per .. + per); n = B * per
static __global__ __launch_bounds__(kThreads) void bias_sum_kernel(int C, int per, int n, const double* __restrict__ ws,
                                                                    float* __restrict__ g_bias) {
  __shared__ double red[kWaves];
  const int c = blockIdx.x;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const int b = i / per;
    s += ws[(b * C + c) * per + (i - b * per)];
  }
  s = wave_sum(s);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = red[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += red[w];
    g_bias[c] = (float)t;
  }
}

inline int ceil_div(long long a, int b) { return (int)((a + b - 1) / b); }

// every index the kernels form (elements of the largest array, segment ids, workgroups) fits a non-negative int
inline bool fits(long long planes, long long rows_per_plane, long long cols) {
  return planes > 0 && planes * rows_per_plane * cols < (1ll << 31);
}

inline int launch_status() { return (int)hipGetLastError(); }

inline int sum_bias(int B, int C, int per, const double* ws, float* g_bias, hipStream_t stream) {
  hipLaunchKernelGGL(bias_sum_kernel, dim3(C), dim3(kThreads), 0, stream, C, per, B * per, ws, g_bias);
  return launch_status();
}

}  // namespace scsfm_decb

using namespace scsfm_decb;

extern "C" {

int scsfm_decb_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_decb_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

size_t scsfm_decb_ws_bytes(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return sizeof(double) * (size_t)B * C * H * ceil_div(W, kChunk);
}

int scsfm_decb_bias_elu_pad_fwd_f32(int B, int C, int H, int W, const float* x, const float* bias, float* out,
                                    void* stream) {
  if (B <= 0 || C <= 0 || H < 2 || W < 2 || !x || !bias || !out || !fits((long long)B * C, H + 2, W + 2)) return -1;
  (void)hipGetLastError();
  const int nchunk = ceil_div(W + 2, kChunk), nseg = B * C * (H + 2) * nchunk;
  hipLaunchKernelGGL(bias_elu_pad_fwd_kernel, dim3(ceil_div(nseg, kWaves)), dim3(kThreads), 0, (hipStream_t)stream,
                     nseg, nchunk, C, H, W, x, bias, out);
  return launch_status();
}

int scsfm_decb_bias_elu_pad_bwd_f32(int B, int C, int H, int W, const float* gp, const float* out, float* g_x, void* ws,
                                    float* g_bias, void* stream) {
  if (B <= 0 || C <= 0 || H < 2 || W < 2 || !gp || !out || !g_x || (g_bias && !ws) ||
      !fits((long long)B * C, H + 2, W + 2))
    return -1;
  (void)hipGetLastError();
  const int nchunk = ceil_div(W, kChunk), nseg = B * C * H * nchunk;
  const dim3 grid(ceil_div(nseg, kWaves)), block(kThreads);
  if (!g_bias) {
    hipLaunchKernelGGL(bias_elu_pad_bwd_kernel<false>, grid, block, 0, (hipStream_t)stream, nseg, nchunk, H, W, gp, out,
                       g_x, (double*)nullptr);
    return launch_status();
  }
  hipLaunchKernelGGL(bias_elu_pad_bwd_kernel<true>, grid, block, 0, (hipStream_t)stream, nseg, nchunk, H, W, gp, out,
                     g_x, (double*)ws);
  if (const int rc = launch_status()) return rc;
  return sum_bias(B, C, H * nchunk, (const double*)ws, g_bias, (hipStream_t)stream);
}

int scsfm_decb_bias_up_cat_pad_fwd_f32(int B, int Ca, int Cs, int H, int W, const float* a, const float* bias,
                                       const float* skip, float* out, void* stream) {
  if (B <= 0 || Ca <= 0 || Cs < 0 || H < 1 || W < 1 || !a || !bias || !out || (Cs > 0 && !skip) ||
      !fits((long long)B * (Ca + Cs), 2 * H + 2, 2 * W + 2))
    return -1;
  (void)hipGetLastError();
  const int nchunk = ceil_div(2 * W + 2, kChunk), nseg = B * (Ca + Cs) * (2 * H + 2) * nchunk;
  hipLaunchKernelGGL(bias_up_cat_pad_fwd_kernel, dim3(ceil_div(nseg, kWaves)), dim3(kThreads), 0, (hipStream_t)stream,
                     nseg, nchunk, Ca, Cs, H, W, a, bias, skip, out);
  return launch_status();
}

int scsfm_decb_bias_up_cat_pad_bwd_f32(int B, int Ca, int Cs, int H, int W, const float* gp, const float* out,
                                       float* g_a, float* g_skip, void* ws, float* g_bias, void* stream) {
  if (B <= 0 || Ca <= 0 || Cs < 0 || H < 1 || W < 1 || !gp || !out || !g_a || (Cs > 0 && !g_skip) || (g_bias && !ws) ||
      !fits((long long)B * (Ca + Cs), 2 * H + 2, 2 * W + 2))
    return -1;
  (void)hipGetLastError();
  const int nchunk_a = ceil_div(W, kChunk), nchunk_s = ceil_div(2 * W, kChunk);
  const int nseg_a = B * Ca * H * nchunk_a, nseg = nseg_a + B * Cs * 2 * H * nchunk_s;
  const dim3 grid(ceil_div(nseg, kWaves)), block(kThreads);
  if (!g_bias) {
    hipLaunchKernelGGL(bias_up_cat_pad_bwd_kernel<false>, grid, block, 0, (hipStream_t)stream, nseg_a, nchunk_a, nseg,
                       nchunk_s, Ca, Cs, H, W, gp, out, g_a, g_skip, (double*)nullptr);
    return launch_status();
  }
  hipLaunchKernelGGL(bias_up_cat_pad_bwd_kernel<true>, grid, block, 0, (hipStream_t)stream, nseg_a, nchunk_a, nseg,
                     nchunk_s, Ca, Cs, H, W, gp, out, g_a, g_skip, (double*)ws);
  if (const int rc = launch_status()) return rc;
  return sum_bias(B, Ca, H * nchunk_a, (const double*)ws, g_bias, (hipStream_t)stream);
}

int scsfm_decb_disp_head_fwd_f32(int B, int C, int H, int W, const float* x, const float* bias, float alpha, float beta,
                                 float* y, float* out, void* stream) {
  if (B <= 0 || C <= 0 || H < 1 || W < 1 || !x || !bias || !y || !out || !fits((long long)B * C, H, W)) return -1;
  (void)hipGetLastError();
  const int N = H * W, nchunk = ceil_div(N, kChunk), nseg = B * C * nchunk;
  hipLaunchKernelGGL(disp_head_fwd_kernel, dim3(ceil_div(nseg, kWaves)), dim3(kThreads), 0, (hipStream_t)stream, nseg,
                     nchunk, C, N, x, bias, alpha, beta, y, out);
  return launch_status();
}

int scsfm_decb_disp_head_bwd_f32(int B, int C, int H, int W, float alpha, const float* g_out, const float* y,
                                 float* g_x, void* ws, float* g_bias, void* stream) {
  if (B <= 0 || C <= 0 || H < 1 || W < 1 || !g_out || !y || !g_x || (g_bias && !ws) || !fits((long long)B * C, H, W))
    return -1;
  (void)hipGetLastError();
  const int N = H * W, nchunk = ceil_div(N, kChunk), nseg = B * C * nchunk;
  const dim3 grid(ceil_div(nseg, kWaves)), block(kThreads);
  if (!g_bias) {
    hipLaunchKernelGGL(disp_head_bwd_kernel<false>, grid, block, 0, (hipStream_t)stream, nseg, nchunk, N, alpha, g_out,
                       y, g_x, (double*)nullptr);
    return launch_status();
  }
  hipLaunchKernelGGL(disp_head_bwd_kernel<true>, grid, block, 0, (hipStream_t)stream, nseg, nchunk, N, alpha, g_out, y,
                     g_x, (double*)ws);
  if (const int rc = launch_status()) return rc;
  return sum_bias(B, C, nchunk, (const double*)ws, g_bias, (hipStream_t)stream);
}

}  // extern "C"
