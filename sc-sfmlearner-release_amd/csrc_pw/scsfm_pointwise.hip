// The weight gradient and the stride-2 data gradient of the encoders' 1x1 convolutions (include/scsfm_pw.h) on the
// exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32.  Both read and write NCHW as it lies.
//
// Weight gradient.  dW[co][ci] = sum over the output pixels of dy[co][pixel] * x[ci][sampled pixel]: a GEMM with
// M = Cout, N = Cin and K = the B * Ho * Wo output pixels.  The output pixels of an image are numbered flat
// (p = y * Wo + x), so a plane of dy is one contiguous run and, for stride 1, so is a plane of x; for stride 2 a pixel's
// x value lies at (2 y) * W + 2 x: only the sampled rows are touched.  A workgroup of four waves takes one 128 x 64
// (Cout x Cin) tile (blockIdx.y) and every gridDim.x-th chunk of 32 pixels: it stages the chunk's 128 dy rows and 64 x
// rows in LDS, plane stride 34 = 2 (mod 32) floats, so that the 16 planes x 2 pixels of a ds_read_b32 lane group hit 32
// different banks (a lane's A value is dy[co = lane & 15][pixel 4 k + (lane >> 4)], its B value
// x[ci = lane & 15][the same pixel]).  Wave v owns Cout blocks 2 v and 2 v + 1 and all four Cin blocks: eight
// independent accumulators.  The next chunk's loads are issued before the current chunk multiplies.  Pixels past the
// image are staged as zeros in both operands.  The workgroup stores one fp32 partial (its tile of dW) at ws[g];
// sum_kernel adds the partials of every entry in fp64 in a fixed order and rounds once, as scsfm_wrw's does.
//
// Data gradient (stride 2).  dx[ci][2 y][2 x] = sum over co of w[co][ci] * dy[co][pixel]: M = Cin, N = the pixels, flat
// over the batch, K = Cout.  A workgroup takes 64 input channels (blockIdx.y) x 64 pixels and walks Cout in chunks of 32,
// staging w[32][64] and dy[32][64] in LDS with row stride 80 = 16 (mod 32) floats (a lane's A value is
// w[co = 4 k + (lane >> 4)][ci = lane & 15], its B value dy[the same co][pixel lane & 15]: 2 rows x 16 columns of a lane
// group hit 32 banks).  A wave owns 2 x 2 blocks of 16 x 16.  The lane that ends up with pixel (y, x) of channel ci
// stores the 2 x 2 cell of dx at (2 y, 2 x) -- the value and three zeros, cut at H and W -- so every element of dx is
// stored once, by one lane.
#include <hip/hip_runtime.h>

#include "scsfm_pw.h"

#ifndef SCSFM_WRW_F32X4  // (the host simulator's shim brings its own)
typedef float f32x4 __attribute__((ext_vector_type(4)));
#endif

namespace scsfm_pw {

constexpr int kWave = 64;
constexpr int kWaves = 4;
constexpr int kThreads = kWave * kWaves;
// the weight gradient
constexpr int kTM = 128, kTN = 64;  // the (Cout, Cin) tile of a workgroup
constexpr int kKP = 32;             // pixels of a chunk
constexpr int kSP = kKP + 2;        // floats per plane in LDS: 34 = 2 (mod 32)
constexpr int kSlots = 512;         // workgroups of a launch, all tiles together
constexpr int kSlices = 8, kPerBlock = kThreads / kSlices;  // sum_kernel: 8 slices of the partials x 32 entries
// the data gradient
constexpr int kDM = 64, kDN = 64;  // the (Cin, pixels) tile of a workgroup
constexpr int kKC = 32;            // output channels of a chunk
constexpr int kSD = 80;            // floats per row in LDS: 16 (mod 32)

__host__ __device__ inline int imin(int a, int b) { return a < b ? a : b; }
__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// (static: the library exports its C ABI and nothing else)
static __global__ __launch_bounds__(kThreads, 2) void wrw_kernel(int Cin, int Cout, int H, int W, int Wo, int HoWo,
                                                                 int s, int chunks_img, int nchunks, int tiles_n,
                                                                 const float* __restrict__ x,
                                                                 const float* __restrict__ dy, float* __restrict__ ws) {
  __shared__ float smem[(kTM + kTN) * kSP];
  float* const ds = smem;
  float* const xs = smem + kTM * kSP;
  constexpr int ND = kTM / 8, NX = kTN / 8;  // rows of dy and of x a thread stages

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const int q32 = tid & 31, r8 = tid >> 5;
  const int P = gridDim.x, g = blockIdx.x;
  const int co0 = (blockIdx.y / tiles_n) * kTM, ci0 = (blockIdx.y % tiles_n) * kTN;
  const int HW = H * W;

  f32x4 acc[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[m][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // a thread stages pixel q32 of the chunk for rows r8, r8 + 8, ... of both operands
  float pd[ND], px[NX];
  auto prefetch = [&](int t) {
    const int n = t / chunks_img, p = (t - n * chunks_img) * kKP + q32;
    const bool in = p < HoWo;
    const int y = p / Wo, xx = p - y * Wo;
    const float* __restrict__ dg = dy + ((size_t)n * Cout + co0 + r8) * HoWo + p;
    const float* __restrict__ xg = x + ((size_t)n * Cin + ci0 + r8) * HW + (s * y) * W + s * xx;
#pragma unroll
    for (int j = 0; j < ND; ++j) pd[j] = in ? dg[j * 8 * HoWo] : 0.f;
#pragma unroll
    for (int j = 0; j < NX; ++j) px[j] = in ? xg[j * 8 * HW] : 0.f;
  };
  auto commit = [&]() {
#pragma unroll
    for (int j = 0; j < ND; ++j) ds[(r8 + 8 * j) * kSP + q32] = pd[j];
#pragma unroll
    for (int j = 0; j < NX; ++j) xs[(r8 + 8 * j) * kSP + q32] = px[j];
  };

  const float* __restrict__ ap = ds + (wave * 32 + l15) * kSP + quad;
  const float* __restrict__ bp = xs + l15 * kSP + quad;
  if (g < nchunks) prefetch(g);
  for (int t = g; t < nchunks; t += P) {
    __syncthreads();  // (the previous chunk has been read)
    commit();
    __syncthreads();
    if (t + P < nchunks) prefetch(t + P);
#pragma unroll
    for (int k = 0; k < kKP / 4; ++k) {
      float a[2], b[4];
#pragma unroll
      for (int m = 0; m < 2; ++m) a[m] = ap[m * 16 * kSP + 4 * k];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = bp[c * 16 * kSP + 4 * k];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[m][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[c], acc[m][c], 0, 0, 0);
    }
  }

  // the instruction's C/D map: column ci = lane & 15, rows co = 4 * (lane >> 4) + i
  float* __restrict__ out = ws + (size_t)g * (Cout * Cin);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        out[(co0 + wave * 32 + m * 16 + quad * 4 + i) * Cin + ci0 + c * 16 + l15] = acc[m][c][i];
}

// dw[e] = the sum over g of ws[g][e] in fp64, rounded once
static __global__ __launch_bounds__(kThreads) void sum_kernel(int G, int E, const float* __restrict__ ws,
                                                              float* __restrict__ dw) {
  __shared__ double part[kSlices][kPerBlock];
  const int j = threadIdx.x & (kPerBlock - 1), sl = threadIdx.x / kPerBlock;
  const int e = blockIdx.x * kPerBlock + j;
  double s = 0.0;
  if (e < E) {
#pragma unroll 8
    for (int g = sl; g < G; g += kSlices) s += (double)ws[(unsigned)g * (unsigned)E + (unsigned)e];
  }
  part[sl][j] = s;
  __syncthreads();
  if (sl == 0 && e < E) {
    double t = part[0][j];
#pragma unroll
    for (int p = 1; p < kSlices; ++p) t += part[p][j];
    dw[e] = (float)t;
  }
}

static __global__ __launch_bounds__(kThreads, 2) void dgrad_kernel(int Cin, int Cout, int H, int W, int Wo, int HoWo,
                                                                   int npix, const float* __restrict__ dy,
                                                                   const float* __restrict__ w, float* __restrict__ dx) {
  __shared__ float smem[2 * kKC * kSD];
  float* const wl = smem;
  float* const dl = smem + kKC * kSD;
  constexpr int NR = kKC / 4;  // rows of w and of dy a thread stages

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int l15 = lane & 15, quad = lane >> 4;
  const int c64 = tid & 63, r4 = tid >> 6;
  const int gp0 = blockIdx.x * kDN, ci0 = blockIdx.y * kDM;
  const int mb = 2 * (wave & 1), nb = 2 * (wave >> 1);
  const int HW = H * W;

  f32x4 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[m][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // a thread stages column c64 (an input channel of w, a pixel of dy) of rows r4, r4 + 4, ... of the chunk
  const int gp = gp0 + c64;
  const bool in = gp < npix;
  const int n_l = gp / HoWo, p_l = gp - n_l * HoWo;
  const float* __restrict__ wg = w + (size_t)r4 * Cin + ci0 + c64;
  const float* __restrict__ dg = dy + ((size_t)n_l * Cout + r4) * HoWo + p_l;
  float pw[NR], pd[NR];
  auto prefetch = [&](int k0) {
#pragma unroll
    for (int j = 0; j < NR; ++j) pw[j] = wg[(k0 + 4 * j) * Cin];
#pragma unroll
    for (int j = 0; j < NR; ++j) pd[j] = in ? dg[(k0 + 4 * j) * HoWo] : 0.f;
  };
  auto commit = [&]() {
#pragma unroll
    for (int j = 0; j < NR; ++j) wl[(r4 + 4 * j) * kSD + c64] = pw[j];
#pragma unroll
    for (int j = 0; j < NR; ++j) dl[(r4 + 4 * j) * kSD + c64] = pd[j];
  };

  const float* __restrict__ ap = wl + quad * kSD + mb * 16 + l15;
  const float* __restrict__ bp = dl + quad * kSD + nb * 16 + l15;
  prefetch(0);
  for (int k0 = 0; k0 < Cout; k0 += kKC) {
    __syncthreads();  // (the previous chunk has been read)
    commit();
    __syncthreads();
    if (k0 + kKC < Cout) prefetch(k0 + kKC);
#pragma unroll
    for (int k = 0; k < kKC / 4; ++k) {
      float a[2], b[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) a[m] = ap[4 * k * kSD + m * 16];
#pragma unroll
      for (int c = 0; c < 2; ++c) b[c] = bp[4 * k * kSD + c * 16];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[m][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[c], acc[m][c], 0, 0, 0);
    }
  }

  // the instruction's C/D map: column pixel = lane & 15, rows ci = 4 * (lane >> 4) + i; the 2 x 2 cell of every value
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int q = gp0 + (nb + c) * 16 + l15;
    if (q < npix) {
      const int n = q / HoWo, p = q - n * HoWo;
      const int y = p / Wo, xx = p - y * Wo;
      const bool right = 2 * xx + 1 < W, below = 2 * y + 1 < H;
      float* __restrict__ o = dx + ((size_t)n * Cin + ci0 + quad * 4) * HW + (2 * y) * W + 2 * xx;
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float* __restrict__ e = o + (m * 16 + mb * 16 + i) * HW;
          e[0] = acc[m][c][i];
          if (right) e[1] = 0.f;
          if (below) {
            e[W] = 0.f;
            if (right) e[W + 1] = 0.f;
          }
        }
    }
  }
}

inline bool covers(int Cin, int Cout, int stride) {
  return (Cin == 64 || Cin == 128 || Cin == 256 || Cin == 512) && (Cout == 128 || Cout == 256 || Cout == 512) &&
         (stride == 1 || stride == 2);
}

struct Plan {
  int Ho, Wo, HoWo, chunks_img, nchunks, tiles_n, tiles, P, E, npix;
};

// the launches of a shape: false for a shape the library rejects -- every index the kernels form fits a non-negative
// int.  The grid depends on the shape alone.
inline bool plan_of(int B, int Cin, int Cout, int H, int W, int stride, Plan& p) {
  if (B <= 0 || H <= 0 || W <= 0 || !covers(Cin, Cout, stride)) return false;
  const long long lim = 1ll << 31;
  p.Ho = (H - 1) / stride + 1;
  p.Wo = (W - 1) / stride + 1;
  if ((long long)B * Cin * H * W >= lim || (long long)p.Ho * p.Wo + kKP >= lim ||
      (long long)B * Cout * p.Ho * p.Wo >= lim || (long long)B * p.Ho * p.Wo + kDN >= lim)
    return false;
  p.HoWo = p.Ho * p.Wo;
  p.npix = B * p.HoWo;
  p.chunks_img = ceil_div(p.HoWo, kKP);
  p.nchunks = B * p.chunks_img;  // (<= npix + B: checked above with room to spare, B <= npix)
  if ((long long)B * p.chunks_img >= lim) return false;
  p.tiles_n = Cin / kTN;
  p.tiles = (Cout / kTM) * p.tiles_n;
  p.P = imin(p.nchunks, kSlots / p.tiles);
  p.E = Cout * Cin;
  return true;
}

inline int launch_status() { return (int)hipGetLastError(); }

}  // namespace scsfm_pw

using namespace scsfm_pw;

extern "C" {

int scsfm_pw_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_pw_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

int scsfm_pw_covers(int Cin, int Cout, int stride) { return covers(Cin, Cout, stride) ? 1 : 0; }

size_t scsfm_pw_wrw_ws_bytes(int B, int Cin, int Cout, int H, int W, int stride) {
  Plan p;
  if (!plan_of(B, Cin, Cout, H, W, stride, p)) return 0;
  return sizeof(float) * (size_t)p.P * p.E;
}

int scsfm_pw_wrw_f32(int B, int Cin, int Cout, int H, int W, int stride, const float* x, const float* dy, float* dw,
                     void* ws, size_t ws_bytes, void* stream) {
  Plan p;
  if (!plan_of(B, Cin, Cout, H, W, stride, p) || !x || !dy || !dw || !ws || ((size_t)ws & 3) ||
      ws_bytes < sizeof(float) * (size_t)p.P * p.E)
    return SCSFM_ERR_ARG;
  (void)hipGetLastError();
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(wrw_kernel, dim3(p.P, p.tiles), dim3(kThreads), 0, st, Cin, Cout, H, W, p.Wo, p.HoWo, stride,
                     p.chunks_img, p.nchunks, p.tiles_n, x, dy, (float*)ws);
  if (const int rc = launch_status()) return rc;
  hipLaunchKernelGGL(sum_kernel, dim3(ceil_div(p.E, kPerBlock)), dim3(kThreads), 0, st, p.P, p.E, (const float*)ws, dw);
  return launch_status();
}

int scsfm_pw_dgrad_f32(int B, int Cin, int Cout, int H, int W, const float* dy, const float* w, float* dx,
                       void* stream) {
  Plan p;
  if (!plan_of(B, Cin, Cout, H, W, 2, p) || !dy || !w || !dx) return SCSFM_ERR_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(dgrad_kernel, dim3(ceil_div(p.npix, kDN), Cin / kDM), dim3(kThreads), 0, (hipStream_t)stream, Cin,
                     Cout, H, W, p.Wo, p.HoWo, p.npix, dy, w, dx);
  return launch_status();
}

}  // extern "C"
