// The backward of the depth decoder's full-resolution tail in one streaming pass (include/scsfm_dgrad.h).
//
// At level 0, Q = R(E(b + bias)) feeds the disparity head alone: out = alpha * sigmoid(conv3x3(Q, w) + bias_h) + beta.
// Its backward used to be four launches: the head's sigmoid backward (g), MIOpen's data gradient of the 16 -> 1
// convolution, which writes the gradient gQ of the padded tensor, the reflection-pad fold + ELU' that reads gQ back, and
// the per-channel bias sums.  Here one kernel reads Q, y and g_out once and writes g and g_b once; gQ never exists.
//
// Work split: a workgroup of four waves owns a tile of kTH = 8 rows x kTW = 64 columns of one image.  It first computes
// g on the tile and a halo of one pixel (zero outside the image) into LDS -- the halo's values are recomputed from the
// same expression by the neighbouring workgroups, the tile's owner alone stores them -- then every lane takes one
// column and two rows (wave v: rows v and v + 4), reads the 3 x 3 window of g around its pixel from LDS and walks the
// 16 channels: one 256-byte run of Q and of g_b per wave and channel.  The head's 144 weights are wave-uniform.
//
// Fold: gE[i][j] sums gQ over the padded positions that the reflection pad filled from (i, j): the interior position
// and, on rows 1 / H - 2 and columns 1 / W - 2, the border positions, in the order of csrc_decb's fold().  Every g that
// those positions touch inside the image lies in the 3 x 3 window of (i, j), so the tile's halo of one suffices.
//
// Sums (the house rule of csrc_decb/scsfm_decoder_bias.hip): every lane adds what it stores in fp64 in a fixed order, the
// wave adds its lanes by the fixed shuffle tree, the four waves are added in ascending order and the workgroup leaves
// 17 fp64 partials (16 channels of g_b, then g) in ws; sums_kernel, one workgroup per sum, adds the partials of all
// workgroups in a fixed order and rounds once to fp32.  No atomics: the same input gives the same bits.
//
// g is one fp32 operation per step, in the order of csrc_decb's disp_head_bwd_kernel, so nothing here may be contracted
// into an fma.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "scsfm_dgrad.h"

#pragma clang fp contract(off)

namespace scsfm_dgrad {

constexpr int kC = 16;  // channels of the tail
constexpr int kWave = 64;
constexpr int kWaves = 4;  // per workgroup
constexpr int kThreads = kWave * kWaves;
constexpr int kTW = 64, kTH = 8;             // the tile of a workgroup
constexpr int kLW = kTW + 2, kLH = kTH + 2;  // with its halo, in LDS
constexpr int kSums = kC + 1;                // per workgroup: 16 channels of g_b, then g

__device__ inline float elu_grad(float g, float r) { return r <= 0.f ? g * (r + 1.f) : g; }

// sum over the wave by a fixed tree; the total is in lane 0
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d);
  return v;
}

// SUM: ws[0..16][workgroup] = the workgroup's sums of g_b per channel and of g
template <bool SUM>
__global__ __launch_bounds__(kThreads) void head_tail_bwd_kernel(int H, int W, int tiles_x, int tiles_y, float alpha,
                                                                  const float* __restrict__ q,
                                                                  const float* __restrict__ y,
                                                                  const float* __restrict__ g_out,
                                                                  const float* __restrict__ w, float* __restrict__ g,
                                                                  float* __restrict__ g_b, double* __restrict__ ws) {
  __shared__ float tile[kLH * kLW];
  __shared__ double red[kWaves][kSums];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
  int t = blockIdx.x;
  const int tx = t % tiles_x;
  t /= tiles_x;
  const int ty = t % tiles_y, b = t / tiles_y;
  const int i0 = ty * kTH, j0 = tx * kTW;

  // g on the tile and its halo; 0 outside the image
  for (int e = tid; e < kLH * kLW; e += kThreads) {
    const int li = e / kLW, lj = e - li * kLW;
    const int gi = i0 + li - 1, gj = j0 + lj - 1;
    float v = 0.f;
    if (gi >= 0 && gi < H && gj >= 0 && gj < W) {
      const int idx = (b * H + gi) * W + gj;
      v = g_out[idx];
      if (y) {
        const float s = y[idx];
        v = ((v * alpha) * (1.f - s)) * s;
      }
      if (li >= 1 && li <= kTH && lj >= 1 && lj <= kTW) g[idx] = v;
    }
    tile[e] = v;
  }
  __syncthreads();

  const int Hp = H + 2, Wp = W + 2;
  const int j = j0 + lane;
  double sum[kSums];
#pragma unroll
  for (int c = 0; c < kSums; ++c) sum[c] = 0.0;

  // g at image position (gi, gj), 0 outside the image; inside the image only positions of this tile and its halo are
  // asked for
  auto gat = [&](int gi, int gj) -> float {
    return gi >= 0 && gi < H && gj >= 0 && gj < W ? tile[(gi - i0 + 1) * kLW + (gj - j0 + 1)] : 0.f;
  };
  // gQ of channel weights wc at padded position (p, qq)
  auto gq = [&](const float* wc, int p, int qq) -> float {
    float a = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s) a += wc[r * 3 + s] * gat(p - r, qq - s);
    return a;
  };

#pragma unroll
  for (int k = 0; k < kTH / kWaves; ++k) {
    const int li = wv + k * kWaves, i = i0 + li;
    if (i < H && j < W) {
      const float* tp = tile + (li + 1) * kLW + lane + 1;
      float G[3][3];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) G[a][c] = tp[(a - 1) * kLW + (c - 1)];
      const bool border = i == 1 || i == H - 2 || j == 1 || j == W - 2;
      const float* qp = q + ((b * kC) * Hp + i + 1) * Wp + j + 1;
      float* dst = g_b + ((b * kC) * H + i) * W + j;
      float r[kC];
#pragma unroll
      for (int c = 0; c < kC; ++c) r[c] = qp[c * Hp * Wp];
#pragma unroll
      for (int c = 0; c < kC; ++c) {
        const float* wc = w + c * 9;
        float in = 0.f;
#pragma unroll
        for (int rr = 0; rr < 3; ++rr)
#pragma unroll
          for (int s = 0; s < 3; ++s) in += wc[rr * 3 + s] * G[2 - rr][2 - s];
        float acc = in;
        if (border) {
          acc = 0.f;
          acc += in;
          if (j == 1) acc += gq(wc, i + 1, 0);
          if (j == W - 2) acc += gq(wc, i + 1, W + 1);
          auto row = [&](int p) {
            acc += gq(wc, p, j + 1);
            if (j == 1) acc += gq(wc, p, 0);
            if (j == W - 2) acc += gq(wc, p, W + 1);
          };
          if (i == 1) row(0);
          if (i == H - 2) row(H + 1);
        }
        const float f = elu_grad(acc, r[c]);
        dst[c * H * W] = f;
        if (SUM) sum[c] += (double)f;
      }
      if (SUM) sum[kC] += (double)G[1][1];
    }
  }

  if (SUM) {
#pragma unroll
    for (int c = 0; c < kSums; ++c) {
      const double v = wave_sum(sum[c]);
      if (lane == 0) red[wv][c] = v;
    }
    __syncthreads();
    if (tid < kSums) {
      double v = red[0][tid];
#pragma unroll
      for (int k = 1; k < kWaves; ++k) v += red[k][tid];
      ws[tid * gridDim.x + blockIdx.x] = v;
    }
  }
}

// workgroup c adds sum c of the n workgroups' partials ws[c][0..n): thread t takes partials t, t + 256, ..., then the
// tree, then the four waves in ascending order; c < 16 -> g_bias_b[c], c = 16 -> g_bias_head[0]; a NULL destination is
// skipped
static __global__ __launch_bounds__(kThreads) void sums_kernel(int n, const double* __restrict__ ws,
                                                                float* __restrict__ g_bias_b,
                                                                float* __restrict__ g_bias_head) {
  __shared__ double red[kWaves];
  const int c = blockIdx.x;
  float* dst = c < kC ? (g_bias_b ? g_bias_b + c : nullptr) : g_bias_head;
  if (!dst) return;
  double s = 0.0;
  for (int k = threadIdx.x; k < n; k += kThreads) s += ws[c * n + k];
  s = wave_sum(s);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = red[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) v += red[k];
    *dst = (float)v;
  }
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// workgroups of a call; 0 for a shape the call rejects: every index the kernels form (elements of q, workgroups times
// 17) fits a non-negative int
inline long long workgroups(int B, int C, int H, int W) {
  if (B <= 0 || C != kC || H < 2 || W < 2) return 0;
  if ((long long)B * C * (H + 2ll) * (W + 2ll) >= (1ll << 31)) return 0;
  return (long long)B * ceil_div(H, kTH) * ceil_div(W, kTW);
}

}  // namespace scsfm_dgrad

using namespace scsfm_dgrad;

extern "C" {

int scsfm_dgrad_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_dgrad_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

int scsfm_dgrad_head_tail_covers(int C) { return C == kC ? 1 : 0; }

size_t scsfm_dgrad_head_tail_ws_bytes(int B, int C, int H, int W) {
  return sizeof(double) * kSums * (size_t)workgroups(B, C, H, W);
}

int scsfm_dgrad_head_tail_bwd_f32(int B, int C, int H, int W, float alpha, const float* q, const float* y,
                                  const float* g_out, const float* w, float* g, float* g_b, void* ws, size_t ws_bytes,
                                  float* g_bias_b, float* g_bias_head, void* stream) {
  const long long nwg = workgroups(B, C, H, W);
  const bool sum = g_bias_b || g_bias_head;
  if (nwg == 0 || !q || !g_out || !w || !g || !g_b) return SCSFM_ERR_ARG;
  if (sum && (!ws || ((uintptr_t)ws & 7) || ws_bytes < sizeof(double) * kSums * (size_t)nwg)) return SCSFM_ERR_ARG;
  (void)hipGetLastError();
  const int tiles_x = ceil_div(W, kTW), tiles_y = ceil_div(H, kTH);
  const dim3 grid((unsigned)nwg), block(kThreads);
  if (!sum) {
    hipLaunchKernelGGL(head_tail_bwd_kernel<false>, grid, block, 0, (hipStream_t)stream, H, W, tiles_x, tiles_y, alpha,
                       q, y, g_out, w, g, g_b, (double*)nullptr);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(head_tail_bwd_kernel<true>, grid, block, 0, (hipStream_t)stream, H, W, tiles_x, tiles_y, alpha, q,
                     y, g_out, w, g, g_b, (double*)ws);
  if (const int rc = (int)hipGetLastError()) return rc;
  hipLaunchKernelGGL(sums_kernel, dim3(kSums), block, 0, (hipStream_t)stream, (int)nwg, (const double*)ws, g_bias_b,
                     g_bias_head);
  return (int)hipGetLastError();
}

}  // extern "C"
