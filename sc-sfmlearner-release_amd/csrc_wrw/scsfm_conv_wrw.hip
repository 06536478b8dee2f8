// The weight gradient of the depth decoder's low-channel 3x3 convolutions (include/scsfm_wrw.h).
//
//     dW[co][ci][r][s] = sum over n, h, w of  dy[n][co][h][w] * x[n][ci][h + r][w + s]
//
// as a GEMM with M = Cout, N = Cin * 9 and K = the pixels, on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32:
// one instruction multiplies a 16 (co) x 4 (pixels) block of dy with a 4 (pixels) x 16 (ci) block of x for one tap
// (r, s).  In NCHW the pixel index w is contiguous for both operands, so a lane's A value is dy[co = lane & 15][h]
// [w0 + (lane >> 4)] and its B value for tap (r, s) is x[ci = lane & 15][h + r][w0 + s + (lane >> 4)]: nothing is
// transposed.  Four pixels cost nine instructions into nine independent accumulators per 16 x 16 (co, ci) block, which
// covers the instruction's dependent latency.
//
// Work split.  A workgroup of four waves takes one 8 x 32 output tile of one image at a time: it stages the tile of dy
// (all Cout planes) and the haloed 10 x 34 tile of x (CC = 16 or 32 input planes, one "chunk"; blockIdx.y counts the
// chunks of Cin) in LDS with coalesced row loads, zero where the tile hangs over the image, so that the pixel loop needs
// no mask.  The PW = (Cout / 16) * (CC / 16) blocks of 16 x 16 (co, ci) are dealt to the waves: with PW = 4 a wave owns
// one block and all the tile's rows, with PW = 2 two waves share a block and take alternate rows, with PW = 1 (16 -> 16)
// the four waves take every fourth row.  Plane strides in LDS are 2 (mod 4) floats, which spreads the 16 planes x 2
// pixels of a ds_read_b32 lane group over the 32 banks.
//
// Reduction.  No atomics and no zero-fill.  The grid's size depends on the shape alone (grid_of); workgroup g walks
// the tiles g, g + G, ... in ascending order and keeps its accumulators in registers from the first tile to the last.
// Waves that share a block add theirs through LDS in ascending wave order; the workgroup stores one fp32 partial dW
// (its chunk's columns) at ws[g]; sum_kernel then adds the G partials of every entry in fp64 in a fixed order (thread
// slice s takes g = s, s + 8, ..., then the eight slices in ascending order) and rounds once to fp32.
#include <hip/hip_runtime.h>

#include "scsfm_wrw.h"

namespace scsfm_wrw {

constexpr int kWave = 64;
constexpr int kWaves = 4;  // per workgroup
constexpr int kThreads = kWave * kWaves;
constexpr int kTH = 8, kTW = 32;             // the output tile
constexpr int kXH = kTH + 2, kXW = kTW + 2;  // the haloed input tile
constexpr int kSX = kXH * kXW + 2;           // floats per input plane in LDS: 342 = 2 (mod 4)
constexpr int kSD = kTH * kTW + 2;           // floats per dy plane in LDS: 258 = 2 (mod 4)
constexpr int kTaps = 9;
constexpr int kSlots = 512;  // workgroups of a launch, all chunks together
constexpr int kSlices = 8, kPerBlock = kThreads / kSlices;  // sum_kernel: 8 slices of the partials x 32 entries

#ifndef SCSFM_WRW_F32X4  // (the host simulator's shim brings its own)
typedef float f32x4 __attribute__((ext_vector_type(4)));
#endif

__host__ __device__ inline int imin(int a, int b) { return a < b ? a : b; }
__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

template <int COUT, int CC>
__global__ __launch_bounds__(kThreads) void wrw_kernel(int Cin, int cout, int H, int W, int tiles_h, int tiles_w, int ntiles,
                                                       const float* __restrict__ x, const float* __restrict__ dy,
                                                       float* __restrict__ ws) {
  constexpr int NCO = COUT / 16, PW = NCO * (CC / 16), PS = kWaves / PW;
  constexpr int kSmem = CC * kSX + COUT * kSD;
  static_assert(PW * PS == kWaves, "the (co, ci) blocks of a chunk are dealt to four waves");
  static_assert(PS == 1 || kSmem >= kWaves * kTaps * 4 * kWave, "the waves' accumulators fit the staging buffer");
  static_assert(kSmem * 4 <= 80 * 1024, "two workgroups per CU");
  __shared__ float smem[kSmem];
  float* const xs = smem;
  float* const ds = smem + CC * kSX;

  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pair = wave / PS, ps = wave % PS;     // this wave's (co, ci) block and its share of the rows
  const int cob = pair % NCO, cib = pair / NCO;
  const int l15 = lane & 15, k = lane >> 4;
  const int G = gridDim.x, g = blockIdx.x, ci0 = blockIdx.y * CC;
  const int Hp = H + 2, Wp = W + 2;
  const int a_base = (cob * 16 + l15) * kSD + k;
  const int b_base = (cib * 16 + l15) * kSX + k;

  f32x4 acc[kTaps];
#pragma unroll
  for (int j = 0; j < kTaps; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // A tile's operands travel HBM -> registers -> LDS: the loads of the workgroup's next tile are issued before the
  // current tile multiplies and are waited for only after it, so their latency hides behind the matrix instructions.
  // The input tile is dealt so that a load's address is a wave-uniform base plus a per-thread constant: a wave
  // takes two consecutive rows of a plane per instruction (its halves one row each, columns 0..31), the two halo
  // columns 32 and 33 of all rows are dealt over the workgroup.
  constexpr int NM = CC * kXH / 2 / kWaves;                          // row pairs per wave
  constexpr int NHALO = (CC * kXH * 2 + kThreads - 1) / kThreads;  // halo elements per thread
  static_assert(kXH % 2 == 0 && (CC * kXH / 2) % kWaves == 0 && kTW == 32, "two rows of one plane per wave-load");
  float pm[NM], ph[NHALO], pd[COUT];
  const int plane_x = Hp * Wp, plane_d = H * W;
  const int half = lane >> 5, q32 = lane & 31;
  // the per-thread part of the addresses: unsigned 32-bit offsets from a wave-uniform pointer, so that a load needs no
  // 64-bit vector arithmetic
  const unsigned xoff = half * Wp + q32, doff = (tid >> 5) * W + q32;
  const int xlds = half * kXW + q32;
  int th = 0, tw = 0;  // the extent of the tile in the registers
  auto prefetch = [&](int t) {
    const int n = t / (tiles_h * tiles_w), rem_t = t - n * (tiles_h * tiles_w);
    const int ty = rem_t / tiles_w, tx = rem_t - ty * tiles_w;
    const int h0 = ty * kTH, w0 = tx * kTW;
    th = imin(kTH, H - h0);
    tw = imin(kTW, W - w0);
    // wave-uniform 64-bit bases; the per-lane offsets stay below 2^31 (checked by the caller)
    const float* __restrict__ xg = x + (((size_t)n * Cin + ci0) * Hp + h0) * Wp + w0;
#pragma unroll
    for (int j = 0; j < NM; ++j) {
      const int R = 2 * (wave + kWaves * j), c = R / kXH, r = R - c * kXH;  // (wave-uniform)
      pm[j] = (r + half < th + 2 && q32 < tw + 2) ? (xg + (c * plane_x + r * Wp))[xoff] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < NHALO; ++j) {
      const int i = tid + j * kThreads, R = i >> 1, q = kTW + (i & 1);
      const int c = R / kXH, r = R - c * kXH;
      ph[j] = (R < CC * kXH && r < th + 2 && q < tw + 2) ? xg[(unsigned)(c * plane_x + r * Wp + q)] : 0.f;
    }
    const float* __restrict__ dg = dy + ((size_t)n * cout * H + h0) * W + w0;
    const bool in = (tid >> 5) < th && q32 < tw;
#pragma unroll
    for (int c = 0; c < COUT; ++c) pd[c] = (in && c < cout) ? (dg + c * plane_d)[doff] : 0.f;
  };
  auto commit = [&]() {
#pragma unroll
    for (int j = 0; j < NM; ++j) {
      const int R = 2 * (wave + kWaves * j), c = R / kXH, r = R - c * kXH;
      xs[c * kSX + r * kXW + xlds] = pm[j];
    }
#pragma unroll
    for (int j = 0; j < NHALO; ++j) {
      const int i = tid + j * kThreads, R = i >> 1, q = kTW + (i & 1);
      const int c = R / kXH, r = R - c * kXH;
      if (R < CC * kXH) xs[c * kSX + r * kXW + q] = ph[j];
    }
#pragma unroll
    for (int c = 0; c < COUT; ++c) ds[c * kSD + tid] = pd[c];
  };

  if (g < ntiles) prefetch(g);
  for (int t = g; t < ntiles; t += G) {
    __syncthreads();  // (the previous tile has been read)
    commit();
    const int nrow = th, nq = (tw + 3) >> 2;
    __syncthreads();
    if (t + G < ntiles) prefetch(t + G);
    for (int h = ps; h < nrow; h += PS) {
      const float* __restrict__ ap = ds + a_base + h * kTW;
      const float* __restrict__ bp = xs + b_base + h * kXW;
      // the operands of pixel group q + 1 are read while group q multiplies (the last group reads itself again)
      float a = ap[0], b[kTaps];
#pragma unroll
      for (int j = 0; j < kTaps; ++j) b[j] = bp[(j / 3) * kXW + j % 3];
      for (int q = 0; q < nq; ++q) {
        const int qn = 4 * imin(q + 1, nq - 1);
        const float a1 = ap[qn];
        float b1[kTaps];
#pragma unroll
        for (int j = 0; j < kTaps; ++j) b1[j] = bp[qn + (j / 3) * kXW + j % 3];
#pragma unroll
        for (int j = 0; j < kTaps; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[j], acc[j], 0, 0, 0);
        a = a1;
#pragma unroll
        for (int j = 0; j < kTaps; ++j) b[j] = b1[j];
      }
    }
  }

  if constexpr (PS > 1) {
    // the waves of a block add their accumulators in ascending wave order: red[wave][register][lane]
    __syncthreads();
    float* const red = smem;
#pragma unroll
    for (int j = 0; j < kTaps; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[((wave * kTaps + j) * 4 + i) * kWave + lane] = acc[j][i];
    __syncthreads();
    if (ps == 0) {
      for (int p = 1; p < PS; ++p)
#pragma unroll
        for (int j = 0; j < kTaps; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[j][i] += red[(((wave + p) * kTaps + j) * 4 + i) * kWave + lane];
    }
  }
  if (ps == 0) {
    // the instruction's C/D map: column ci = lane & 15, rows co = 4 * (lane >> 4) + i
    float* __restrict__ out = ws + (size_t)g * (cout * Cin * kTaps);
    const int ci = ci0 + cib * 16 + l15;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = cob * 16 + k * 4 + i;
      if (co < cout) {
#pragma unroll
        for (int j = 0; j < kTaps; ++j) out[(co * Cin + ci) * kTaps + j] = acc[j][i];
      }
    }
  }
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

inline bool covers(int Cin, int Cout) {
  // (Cout = 1, a disparity head, runs as one row of a 16-row block whose other rows are zero)
  return (Cout == 1 || Cout == 16 || Cout == 32) && (Cin == 16 || Cin == 32 || Cin == 64 || Cin == 96);
}

struct Plan {
  int cc, chunks, tiles_h, tiles_w, ntiles, G, E;
};

// the launch of a shape: false for a shape the library rejects.  The grid depends on the shape alone: 512 workgroups
// over all chunks (two per CU of an MI355X, which is what 77 KB of LDS and the prefetch registers allow), fewer when
// there are fewer tiles.
inline bool plan_of(int B, int Cin, int Cout, int H, int W, Plan& p) {
  if (B <= 0 || H <= 0 || W <= 0 || !covers(Cin, Cout)) return false;
  p.cc = Cin >= 32 ? 32 : 16;
  p.chunks = Cin / p.cc;
  // per-lane offsets inside a chunk of one image, and the tile count, in 32 bits
  if ((long long)p.cc * (H + 2ll) * (W + 2ll) >= (1ll << 31) || (long long)Cout * H * W >= (1ll << 31)) return false;
  p.tiles_h = ceil_div(H, kTH);
  p.tiles_w = ceil_div(W, kTW);
  const long long nt = (long long)B * p.tiles_h * p.tiles_w;
  if (nt >= (1ll << 31)) return false;
  p.ntiles = (int)nt;
  p.G = imin(p.ntiles, kSlots / p.chunks);
  p.E = Cout * Cin * kTaps;
  return true;
}

inline int launch_status() { return (int)hipGetLastError(); }

template <int COUT, int CC>
inline void launch(const Plan& p, int Cin, int Cout, int H, int W, const float* x, const float* dy, float* ws,
                   hipStream_t stream) {
  hipLaunchKernelGGL((wrw_kernel<COUT, CC>), dim3(p.G, p.chunks), dim3(kThreads), 0, stream, Cin, Cout, H, W, p.tiles_h,
                     p.tiles_w, p.ntiles, x, dy, ws);
}

}  // namespace scsfm_wrw

using namespace scsfm_wrw;

extern "C" {

int scsfm_wrw_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_wrw_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

int scsfm_wrw_conv3x3_covers(int Cin, int Cout) { return covers(Cin, Cout) ? 1 : 0; }

size_t scsfm_wrw_conv3x3_ws_bytes(int B, int Cin, int Cout, int H, int W) {
  Plan p;
  if (!plan_of(B, Cin, Cout, H, W, p)) return 0;
  return sizeof(float) * (size_t)p.G * p.E;
}

int scsfm_wrw_conv3x3_f32(int B, int Cin, int Cout, int H, int W, const float* x, const float* dy, float* dw, void* ws,
                          size_t ws_bytes, void* stream) {
  Plan p;
  if (!plan_of(B, Cin, Cout, H, W, p) || !x || !dy || !dw || !ws || ((size_t)ws & 3) ||
      ws_bytes < sizeof(float) * (size_t)p.G * p.E)
    return -1;
  (void)hipGetLastError();
  hipStream_t st = (hipStream_t)stream;
  if (Cout <= 16 && p.cc == 16) launch<16, 16>(p, Cin, Cout, H, W, x, dy, (float*)ws, st);
  else if (Cout <= 16) launch<16, 32>(p, Cin, Cout, H, W, x, dy, (float*)ws, st);
  else if (p.cc == 16) launch<32, 16>(p, Cin, Cout, H, W, x, dy, (float*)ws, st);
  else launch<32, 32>(p, Cin, Cout, H, W, x, dy, (float*)ws, st);
  if (const int rc = launch_status()) return rc;
  hipLaunchKernelGGL(sum_kernel, dim3(ceil_div(p.E, kPerBlock)), dim3(kThreads), 0, st, p.G, p.E, (const float*)ws, dw);
  return launch_status();
}

}  // extern "C"
