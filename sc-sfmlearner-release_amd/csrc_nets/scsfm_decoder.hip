// Fused glue of DispResNet's depth decoder (include/scsfm_nets.h): reflection pad, ELU, 2x nearest upsampling and the
// skip concatenation that sit between the decoder's 3x3 convolutions, forward and backward, each one pass over HBM.
//
// Work split: a wave owns one segment of kChunk = 256 consecutive elements of one output row (a row of the padded
// output in the forward, of the unpadded gradient in the backward) and a lane handles kPer = 4 of them, 64 apart, so
// that every load and store instruction of a wave covers 256 contiguous bytes and each lane keeps four independent
// loads in flight.  The row (plane, y) of a segment is wave-uniform, so the channel branch of the concatenation and
// the reflected source row cost no divergence; only the lanes on the reflected border columns diverge.
//
// Exactness (the point of this file: the convolutions must see the tensors ATen's chain produces, bit for bit):
//  - forward: copies plus x > 0 ? x : expm1f(x), ATen's ELU with alpha = scale = input_scale = 1;
//  - backward: ATen's reflection-pad backward zero-fills its output and adds every padded-gradient entry into it with
//    atomics, so an interior entry is 0 + g (which maps -0 to +0, kept here) and a border entry 0 + g1 + g2, which
//    is the same in either order; only the corner entries (four terms, unordered in ATen) take this file's fixed
//    order.  The 2x2 children of an upsampled element are then summed as ATen's upsample_nearest2d backward does,
//    from 0 in row-major order, and the ELU gradient is ATen's result form g * (r + 1) for r <= 0.
#include <hip/hip_runtime.h>

#include "scsfm_nets.h"

namespace scsfm_nets {

constexpr int kWave = 64;
constexpr int kWaves = 4;  // per workgroup
constexpr int kPer = 4;    // elements per lane
constexpr int kChunk = kWave * kPer;

__device__ inline int refl(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
__device__ inline float elu(float x) { return x > 0.f ? x : expm1f(x); }
__device__ inline float elu_grad(float g, float r) { return r <= 0.f ? g * (r + 1.f) : g; }

// this wave's segment (wave-uniform) and lane; false when the wave has no segment
__device__ inline bool segment(int nseg, int& seg, int& lane) {
  seg = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
  lane = threadIdx.x & (kWave - 1);
  return seg < nseg;
}

// The reflection-pad backward of one entry (y, x) of an H x W plane from its padded gradient g ((H+2) x (W+2)):
// 0 + the padded entries that reflect onto it, row by row (y+1, then 0 when y == 1, then H+1 when y == H-2), each row
// at columns x+1, then 0 when x == 1, then W+1 when x == W-2.  `in` is the first of them, g[y+1][x+1]: the callers
// load every lane's interior entries up front, so that those loads are in flight together, and only the few lanes
// and (wave-uniform) rows on a reflected border load more.
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

// out[plane][p][q] = R(E?(x))[plane][p][q]; rows = planes * (H+2)
template <bool ELU>
__global__ __launch_bounds__(kWave* kWaves) void pad_fwd_kernel(int nseg, int nchunk, int H, int W,
                                                                  const float* __restrict__ x, float* __restrict__ out) {
  int seg, lane;
  if (!segment(nseg, seg, lane)) return;
  const int Hp = H + 2, Wp = W + 2;
  const int row = seg / nchunk, q0 = (seg - row * nchunk) * kChunk + lane;
  const int plane = row / Hp, p = row - plane * Hp;
  const float* src = x + (plane * H + refl(p - 1, H)) * W;
  float* dst = out + row * Wp;
  float v[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) v[j] = src[refl(min(q0 + j * kWave, Wp - 1) - 1, W)];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int q = q0 + j * kWave;
    if (q < Wp) dst[q] = ELU ? elu(v[j]) : v[j];
  }
}

// out[b][c][p][q] = R(cat[U(E(a)), skip]); rows = B * (Ca+Cs) * (2H+2)
__global__ __launch_bounds__(kWave* kWaves) void up_cat_pad_fwd_kernel(int nseg, int nchunk, int Ca, int Cs, int H,
                                                                        int W, const float* __restrict__ a,
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
    const float* src = a + ((b * Ca + c) * H + (Y >> 1)) * W;
#pragma unroll
    for (int j = 0; j < kPer; ++j) v[j] = src[refl(min(q0 + j * kWave, Wp - 1) - 1, W2) >> 1];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int q = q0 + j * kWave;
      if (q < Wp) dst[q] = elu(v[j]);
    }
  } else {
    const float* src = skip + ((b * Cs + (c - Ca)) * H2 + Y) * W2;
#pragma unroll
    for (int j = 0; j < kPer; ++j) v[j] = src[refl(min(q0 + j * kWave, Wp - 1) - 1, W2)];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int q = q0 + j * kWave;
      if (q < Wp) dst[q] = v[j];
    }
  }
}

// g_x[plane][y][x] = fold(gp)[y][x] (times the ELU gradient at out's interior); rows = planes * H
template <bool ELU>
__global__ __launch_bounds__(kWave* kWaves) void pad_bwd_kernel(int nseg, int nchunk, int H, int W,
                                                                  const float* __restrict__ gp,
                                                                  const float* __restrict__ out,
                                                                  float* __restrict__ g_x) {
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
    const int x = min(x0 + j * kWave, W - 1);
    v[j] = g[ro + x];
    if (ELU) r[j] = out[plane * Hp * Wp + ro + x];
  }
  float* dst = g_x + row * W;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int x = x0 + j * kWave;
    const float f = fold(g, Wp, H, W, y, min(x, W - 1), v[j]);
    if (x < W) dst[x] = ELU ? elu_grad(f, r[j]) : f;
  }
}

// the first B*Ca*H rows: g_a[b][c][y][x] = E'(r) * sum of the four folded children (2y|2y+1, 2x|2x+1), row-major;
// the next B*Cs*2H rows: g_skip[b][c][Y][X] = fold(gp[b][Ca+c])[Y][X]
__global__ __launch_bounds__(kWave* kWaves) void up_cat_pad_bwd_kernel(int nseg_a, int nchunk_a, int nseg, int nchunk_s,
                                                                        int Ca, int Cs, int H, int W,
                                                                        const float* __restrict__ gp,
                                                                        const float* __restrict__ out,
                                                                        float* __restrict__ g_a,
                                                                        float* __restrict__ g_skip) {
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
      const int x = min(x0 + j * kWave, W - 1);
      v[j][0] = g[ro + 2 * x];
      v[j][1] = g[ro + 2 * x + 1];
      v[j][2] = g[ro + Wp + 2 * x];
      v[j][3] = g[ro + Wp + 2 * x + 1];
      r[j] = out[(b * Ct + c) * Hp * Wp + ro + 2 * x];
    }
    float* dst = g_a + row * W;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int x = x0 + j * kWave, xc = min(x, W - 1);
      float acc = 0.f;
      acc += fold(g, Wp, H2, W2, 2 * y, 2 * xc, v[j][0]);
      acc += fold(g, Wp, H2, W2, 2 * y, 2 * xc + 1, v[j][1]);
      acc += fold(g, Wp, H2, W2, 2 * y + 1, 2 * xc, v[j][2]);
      acc += fold(g, Wp, H2, W2, 2 * y + 1, 2 * xc + 1, v[j][3]);
      if (x < W) dst[x] = elu_grad(acc, r[j]);
    }
  } else {
    seg -= nseg_a;
    const int row = seg / nchunk_s, x0 = (seg - row * nchunk_s) * kChunk + lane;
    const int plane = row / H2, Y = row - plane * H2;
    const int b = plane / Cs, c = plane - b * Cs;
    const float* g = gp + (b * Ct + Ca + c) * Hp * Wp;
    const int ro = (Y + 1) * Wp + 1;
    float v[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) v[j] = g[ro + min(x0 + j * kWave, W2 - 1)];
    float* dst = g_skip + row * W2;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int x = x0 + j * kWave;
      const float f = fold(g, Wp, H2, W2, Y, min(x, W2 - 1), v[j]);
      if (x < W2) dst[x] = f;
    }
  }
}

inline int ceil_div(long long a, int b) { return (int)((a + b - 1) / b); }

// every index the kernels form (elements of the largest array, segment ids, workgroups) fits a non-negative int
inline bool fits(long long planes, long long rows_per_plane, long long cols) {
  return planes > 0 && planes * rows_per_plane * cols < (1ll << 31);
}

inline int launch_status() { return (int)hipGetLastError(); }

}  // namespace scsfm_nets

using namespace scsfm_nets;

extern "C" {

int scsfm_nets_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_nets_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

int scsfm_nets_pad_fwd_f32(int B, int C, int H, int W, int elu, const float* x, float* out, void* stream) {
  if (B <= 0 || C <= 0 || H < 2 || W < 2 || !x || !out || !fits((long long)B * C, H + 2, W + 2)) return -1;
  (void)hipGetLastError();
  const int nchunk = ceil_div(W + 2, kChunk), nseg = B * C * (H + 2) * nchunk;
  const dim3 grid(ceil_div(nseg, kWaves)), block(kWave * kWaves);
  if (elu)
    hipLaunchKernelGGL(pad_fwd_kernel<true>, grid, block, 0, (hipStream_t)stream, nseg, nchunk, H, W, x, out);
  else
    hipLaunchKernelGGL(pad_fwd_kernel<false>, grid, block, 0, (hipStream_t)stream, nseg, nchunk, H, W, x, out);
  return launch_status();
}

int scsfm_nets_pad_bwd_f32(int B, int C, int H, int W, int elu, const float* gp, const float* out, float* g_x,
                           void* stream) {
  if (B <= 0 || C <= 0 || H < 2 || W < 2 || !gp || !g_x || (elu && !out) || !fits((long long)B * C, H + 2, W + 2))
    return -1;
  (void)hipGetLastError();
  const int nchunk = ceil_div(W, kChunk), nseg = B * C * H * nchunk;
  const dim3 grid(ceil_div(nseg, kWaves)), block(kWave * kWaves);
  if (elu)
    hipLaunchKernelGGL(pad_bwd_kernel<true>, grid, block, 0, (hipStream_t)stream, nseg, nchunk, H, W, gp, out, g_x);
  else
    hipLaunchKernelGGL(pad_bwd_kernel<false>, grid, block, 0, (hipStream_t)stream, nseg, nchunk, H, W, gp, out, g_x);
  return launch_status();
}

int scsfm_nets_up_cat_pad_fwd_f32(int B, int Ca, int Cs, int H, int W, const float* a, const float* skip, float* out,
                                  void* stream) {
  if (B <= 0 || Ca <= 0 || Cs < 0 || H < 1 || W < 1 || !a || !out || (Cs > 0 && !skip) ||
      !fits((long long)B * (Ca + Cs), 2 * H + 2, 2 * W + 2))
    return -1;
  (void)hipGetLastError();
  const int nchunk = ceil_div(2 * W + 2, kChunk), nseg = B * (Ca + Cs) * (2 * H + 2) * nchunk;
  hipLaunchKernelGGL(up_cat_pad_fwd_kernel, dim3(ceil_div(nseg, kWaves)), dim3(kWave * kWaves), 0, (hipStream_t)stream,
                     nseg, nchunk, Ca, Cs, H, W, a, skip, out);
  return launch_status();
}

int scsfm_nets_up_cat_pad_bwd_f32(int B, int Ca, int Cs, int H, int W, const float* gp, const float* out, float* g_a,
                                  float* g_skip, void* stream) {
  if (B <= 0 || Ca <= 0 || Cs < 0 || H < 1 || W < 1 || !gp || !out || !g_a || (Cs > 0 && !g_skip) ||
      !fits((long long)B * (Ca + Cs), 2 * H + 2, 2 * W + 2))
    return -1;
  (void)hipGetLastError();
  const int nchunk_a = ceil_div(W, kChunk), nchunk_s = ceil_div(2 * W, kChunk);
  const int nseg_a = B * Ca * H * nchunk_a, nseg = nseg_a + B * Cs * 2 * H * nchunk_s;
  hipLaunchKernelGGL(up_cat_pad_bwd_kernel, dim3(ceil_div(nseg, kWaves)), dim3(kWave * kWaves), 0, (hipStream_t)stream,
                     nseg_a, nchunk_a, nseg, nchunk_s, Ca, Cs, H, W, gp, out, g_a, g_skip);
  return launch_status();
}

}  // extern "C"
