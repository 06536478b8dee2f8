// The data gradient of the depth decoder's low-channel 3x3 convolutions on the exact-fp32 matrix instruction
// v_mfma_f32_16x16x4_f32 (include/scsfm_dgrad.h: scsfm_dgrad_conv3x3_f32).
//
//     dx[n][ci][p][q] = sum over co, r, s of  w[co][ci][r][s] * dy[n][co][p - r][q - s]        (dy = 0 outside H x W)
//
// M = Cin (one or two blocks of 16), N = 16 consecutive pixels of a row of dx, K = (r, s, co) = 144 in 36 steps of four
// output channels.  Both tensors are read and written as they lie (NCHW).  A lane's A value of step (r, s, g) is
// w[co = 4 g + (lane >> 4)][ci = lane & 15][r][s]: the 36 (72 for Cin = 32) values stay in registers for the whole
// workgroup.  Its B value is dy[co][p - r][q0 + (lane & 15) - s], read from the workgroup's dy tile in LDS: the tile of
// kTP x kTQ = 8 x 64 pixels of dx needs 10 x 66 pixels of each of the 16 dy planes, stored with zeros where it hangs over
// the image.  The plane stride is 16 (mod 32) floats, so the two planes x 16 pixels of a ds_read_b32 lane group hit 32
// different banks.  Wave v takes rows v and v + 4 of the tile, four blocks of 16 pixels each; an accumulator register
// holds 16 consecutive pixels of one input channel, stored as a 64-byte run.  Every output element is written by one
// lane from one accumulator: no workspace, no reduction across workgroups, the same bits call after call.
#include <hip/hip_runtime.h>

#include "scsfm_dgrad.h"

#ifndef SCSFM_WRW_F32X4
typedef float f32x4 __attribute__((ext_vector_type(4)));
#endif

namespace scsfm_dgrad_conv {

constexpr int kCout = 16;
constexpr int kWave = 64;
constexpr int kWaves = 4;
constexpr int kThreads = kWave * kWaves;
constexpr int kTP = 8, kTQ = 64;             // the tile of dx of a workgroup
constexpr int kLH = kTP + 2, kLW = kTQ + 2;  // the rows and columns of dy it needs
constexpr int kPlane = 672;                  // >= kLH * kLW = 660, 16 (mod 32)
constexpr int kSteps = 36;                   // 9 taps x 4 groups of 4 output channels
constexpr int kBatch = 14;                   // loads of a thread in flight while the tile is staged

// NB: blocks of 16 input channels (Cin = 16 NB)
template <int NB>
__global__ __launch_bounds__(kThreads) void conv3x3_dgrad_kernel(int H, int W, int tiles_q, int tiles_p,
                                                                  const float* __restrict__ dy,
                                                                  const float* __restrict__ w, float* __restrict__ dx) {
  __shared__ float tile[kCout * kPlane];
  constexpr int Cin = 16 * NB;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;
  int t = blockIdx.x;
  const int tq = t % tiles_q;
  t /= tiles_q;
  const int tp = t % tiles_p, n = t / tiles_p;
  const int p0 = tp * kTP, q0 = tq * kTQ;
  const int Hp = H + 2, Wp = W + 2;

  // the weights of this lane: a[m][step], step = (r * 3 + s) * 4 + g
  float a[NB][kSteps];
#pragma unroll
  for (int m = 0; m < NB; ++m)
#pragma unroll
    for (int rs = 0; rs < 9; ++rs)
#pragma unroll
      for (int g = 0; g < 4; ++g) a[m][rs * 4 + g] = w[((4 * g + quad) * Cin + 16 * m + col) * 9 + rs];

  // dy rows p0 - 2 .. p0 + kTP - 1, columns q0 - 2 .. q0 + kTQ - 1 of the 16 planes, 0 outside the image; kBatch loads of a
  // thread are in flight before the first is stored
  constexpr int kElems = kCout * kLH * kLW;
  for (int e0 = tid; e0 < kElems; e0 += kBatch * kThreads) {
    float v[kBatch];
    int at[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int e = e0 + u * kThreads;
      const int co = e / (kLH * kLW), rem = e - co * (kLH * kLW);
      const int lr = rem / kLW, lc = rem - lr * kLW;
      const int gi = p0 - 2 + lr, gj = q0 - 2 + lc;
      at[u] = e < kElems ? co * kPlane + rem : -1;
      v[u] = 0.f;
      if (e < kElems && gi >= 0 && gi < H && gj >= 0 && gj < W) v[u] = dy[((n * kCout + co) * H + gi) * W + gj];
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u)
      if (at[u] >= 0) tile[at[u]] = v[u];
  }
  __syncthreads();

#pragma unroll 1
  for (int k = 0; k < kTP / kWaves; ++k) {
    const int lp = wv + k * kWaves, p = p0 + lp;
#pragma unroll 1
    for (int cb = 0; cb < kTQ / 16; ++cb) {
      f32x4 acc[NB];
#pragma unroll
      for (int m = 0; m < NB; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
      // this lane's B values: plane 4 g + quad, row lp + 2 - r, column cb * 16 + col + 2 - s
      const float* base = tile + quad * kPlane + (lp + 2) * kLW + cb * 16 + col + 2;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float b = base[4 * g * kPlane - r * kLW - s];
#pragma unroll
            for (int m = 0; m < NB; ++m)
              acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][(r * 3 + s) * 4 + g], b, acc[m], 0, 0, 0);
          }
      const int q = q0 + cb * 16 + col;
      if (p < Hp && q < Wp) {
#pragma unroll
        for (int m = 0; m < NB; ++m)
#pragma unroll
          for (int i = 0; i < 4; ++i) dx[((n * Cin + 16 * m + 4 * quad + i) * Hp + p) * Wp + q] = acc[m][i];
      }
    }
  }
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// workgroups of a call; 0 for a shape the call rejects: every index the kernels form fits a non-negative int
inline long long workgroups(int B, int Cin, int Cout, int H, int W) {
  if (B <= 0 || Cout != kCout || (Cin != 16 && Cin != 32) || H < 1 || W < 1) return 0;
  if ((long long)B * (Cin > Cout ? Cin : Cout) * (H + 2ll) * (W + 2ll) >= (1ll << 31)) return 0;
  return (long long)B * ceil_div(H + 2, kTP) * ceil_div(W + 2, kTQ);
}

}  // namespace scsfm_dgrad_conv

using namespace scsfm_dgrad_conv;

extern "C" {

int scsfm_dgrad_conv3x3_covers(int Cin, int Cout) { return Cout == kCout && (Cin == 16 || Cin == 32) ? 1 : 0; }

int scsfm_dgrad_conv3x3_f32(int B, int Cin, int Cout, int H, int W, const float* dy, const float* w, float* dx,
                            void* stream) {
  const long long nwg = workgroups(B, Cin, Cout, H, W);
  if (nwg == 0 || !dy || !w || !dx) return SCSFM_ERR_ARG;
  (void)hipGetLastError();
  const int tiles_q = ceil_div(W + 2, kTQ), tiles_p = ceil_div(H + 2, kTP);
  const dim3 grid((unsigned)nwg), block(kThreads);
  if (Cin == 16)
    hipLaunchKernelGGL(conv3x3_dgrad_kernel<1>, grid, block, 0, (hipStream_t)stream, H, W, tiles_q, tiles_p, dy, w, dx);
  else
    hipLaunchKernelGGL(conv3x3_dgrad_kernel<2>, grid, block, 0, (hipStream_t)stream, H, W, tiles_q, tiles_p, dy, w, dx);
  return (int)hipGetLastError();
}

}  // extern "C"
