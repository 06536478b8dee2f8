// The per-image work of run_inference.py (include/scsfm_vis.h).
//
//  normalise  uint8 [N, H, W, 3] -> float [N, 3, H, W], one lane per pixel: three byte loads, three coalesced stores.
//  max        one pass over the maps: every lane folds its pixels into an order-preserving uint32 key (a NaN is the
//             largest key), the wave folds with shuffles, the block through LDS, and one lane issues one integer
//             atomicMax into the image's word of `out`; a second launch of N lanes turns the keys back into floats.
//  colourise  pure streaming: 4 B read and 4 B written per pixel, four pixels per lane through 16-byte accesses, the
//             rest one per lane; the table (at most 40 KB here) is read as 32-bit words and stays in L2 / L1.
//
// Exactness: every `/` is the correctly rounded float32 division (the project's flags relax nothing) and contraction is
// off, so (v / d) * n rounds twice as numpy does.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "scsfm_vis.h"

#pragma clang fp contract(off)

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocksPerImage = 64;   // of the maximum: 64 atomics per image at the most
constexpr int kPixelsPerBlock = kThreads * 8;
constexpr long long kMaxPixels = (long long)1 << 29;  // 4 bytes out per pixel: every byte offset fits 32 bits
constexpr int kMaxTable = 1 << 24;                    // (float) table_n is exact

struct alignas(16) Float4 { float x, y, z, w; };
struct alignas(16) Word4 { uint32_t x, y, z, w; };

// ---- normalise ----

__device__ inline float normalise(unsigned char b) { return ((float)b / 255.0f - 0.45f) / 0.225f; }

__global__ void __launch_bounds__(kThreads)
normalise_kernel(unsigned total, unsigned HW, const unsigned char* __restrict__ in, float* __restrict__ out) {
  const unsigned gid = blockIdx.x * kThreads + threadIdx.x;
  if (gid >= total) return;
  const unsigned n = gid / HW, p = gid - n * HW;
  const unsigned char* __restrict__ px = in + 3ll * gid;
  float* __restrict__ o = out + 3ll * n * HW + p;
  o[0] = normalise(px[0]);
  o[HW] = normalise(px[1]);
  o[2ll * HW] = normalise(px[2]);
}

// ---- maximum ----

constexpr uint32_t kNanKey = 0xffffffffu;

// float bits -> uint32 with the order of the floats (negative below positive); a NaN of either sign above everything.
// No float maps to 0, which therefore stands for "nothing seen".
__device__ inline uint32_t ordered(float z) {
  const uint32_t b = __builtin_bit_cast(uint32_t, z);
  if (z != z) return kNanKey;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ inline uint32_t unordered_bits(uint32_t o) {
  if (o == kNanKey) return 0x7fc00000u;
  return (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
}

// block b of image n folds pixels b * kThreads + t, + blocks * kThreads, ...   (every lane reaches every shuffle)
__global__ void __launch_bounds__(kThreads)
max_kernel(unsigned HW, unsigned blocks, const float* __restrict__ in, uint32_t* __restrict__ keys) {
  __shared__ uint32_t wave_key[kWaves];
  const unsigned n = blockIdx.x / blocks, b = blockIdx.x - n * blocks;
  const float* __restrict__ img = in + (long long)n * HW;
  uint32_t key = 0u;
  for (unsigned i = b * kThreads + threadIdx.x; i < HW; i += blocks * kThreads) {
    const uint32_t k = ordered(img[i]);
    key = k > key ? k : key;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t other = __shfl_down(key, (unsigned)d, 64);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63u) == 0u) wave_key[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x == 0u) {
    for (int w = 1; w < kWaves; ++w) key = wave_key[w] > key ? wave_key[w] : key;
    atomicMax(keys + n, key);
  }
}

__global__ void __launch_bounds__(kThreads) decode_kernel(unsigned N, uint32_t* __restrict__ keys) {
  const unsigned gid = blockIdx.x * kThreads + threadIdx.x;
  if (gid < N) keys[gid] = unordered_bits(keys[gid]);
}

// ---- colourise ----

__device__ inline uint32_t colour(float x, float d, float nf, int last, bool reciprocal,
                                  const uint32_t* __restrict__ table) {
  const float v = reciprocal ? 1.0f / x : x;
  const float xa = (v / d) * nf;
  const bool bad = xa != xa;
  int idx = xa >= nf ? last : (int)(xa > 0.0f ? xa : 0.0f);  // (a NaN fails both comparisons: entry 0, not used)
  idx = idx < 0 ? 0 : (idx > last ? last : idx);
  const uint32_t word = table[idx];
  return bad ? 0u : word;
}

// lanes [0, n_vec) take pixels 4 gid .. 4 gid + 3, lanes [n_vec, n_vec + total - 4 n_vec) one of the remaining pixels
__global__ void __launch_bounds__(kThreads)
colourise_kernel(unsigned total, unsigned n_vec, unsigned HW, const float* __restrict__ in,
                 const uint32_t* __restrict__ table, float nf, int last, const float* __restrict__ divisors,
                 float max_value, int reciprocal, uint32_t* __restrict__ out) {
  const unsigned gid = blockIdx.x * kThreads + threadIdx.x;
  const bool rec = reciprocal != 0;
  if (gid < n_vec) {
    const Float4 x = reinterpret_cast<const Float4*>(in)[gid];
    const float xs[4] = {x.x, x.y, x.z, x.w};
    uint32_t ws[4];
    unsigned n = (4u * gid) / HW, r = 4u * gid - n * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (r >= HW) { r -= HW; ++n; }  // (r grows by one per pixel: one step is enough, also for HW == 1)
      const float d = divisors ? divisors[n] : max_value;
      ws[k] = colour(xs[k], d, nf, last, rec, table);
      ++r;
    }
    Word4 w;
    w.x = ws[0]; w.y = ws[1]; w.z = ws[2]; w.w = ws[3];
    reinterpret_cast<Word4*>(out)[gid] = w;
    return;
  }
  const unsigned p = 4u * n_vec + (gid - n_vec);
  if (p >= total) return;
  const float d = divisors ? divisors[p / HW] : max_value;
  out[p] = colour(in[p], d, nf, last, rec, table);
}

inline int ceil_div(long long a, int b) { return (int)((a + b - 1) / b); }
inline int launch_status() { return (int)hipGetLastError(); }
inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" {

int scsfm_vis_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_vis_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

int scsfm_vis_normalise_u8(int N, int H, int W, const unsigned char* in, float* out, void* stream) {
  if (N < 1 || H < 1 || W < 1 || !in || !out || !aligned(out, 4)) return SCSFM_VIS_ERR_ARG;
  const long long total = (long long)N * H * W;
  if (total >= kMaxPixels) return SCSFM_VIS_ERR_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(normalise_kernel, dim3(ceil_div(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     (unsigned)total, (unsigned)(H * W), in, out);
  return launch_status();
}

int scsfm_vis_image_max(int N, int HW, const float* in, float* out, void* stream) {
  if (N < 1 || HW < 1 || !in || !out || !aligned(in, 4) || !aligned(out, 4)) return SCSFM_VIS_ERR_ARG;
  if ((long long)N * HW >= kMaxPixels) return SCSFM_VIS_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* keys = reinterpret_cast<uint32_t*>(out);
  int blocks = ceil_div(HW, kPixelsPerBlock);
  if (blocks > kMaxBlocksPerImage) blocks = kMaxBlocksPerImage;
  (void)hipGetLastError();
  const hipError_t rc = hipMemsetAsync(keys, 0, (size_t)N * sizeof(uint32_t), s);
  if (rc != hipSuccess) return (int)rc;
  hipLaunchKernelGGL(max_kernel, dim3((unsigned)N * (unsigned)blocks), dim3(kThreads), 0, s, (unsigned)HW,
                     (unsigned)blocks, in, keys);
  hipLaunchKernelGGL(decode_kernel, dim3(ceil_div(N, kThreads)), dim3(kThreads), 0, s, (unsigned)N, keys);
  return launch_status();
}

int scsfm_vis_colourise(int N, int H, int W, const float* in, const unsigned char* table, int table_n,
                        const float* divisors, double max_value, int reciprocal, unsigned char* out, void* stream) {
  if (N < 1 || H < 1 || W < 1 || !in || !table || table_n < 1 || table_n > kMaxTable || !out) return SCSFM_VIS_ERR_ARG;
  if (!aligned(in, 4) || !aligned(table, 4) || !aligned(out, 4) || (divisors && !aligned(divisors, 4)))
    return SCSFM_VIS_ERR_ARG;
  const long long total = (long long)N * H * W;
  if (total >= kMaxPixels) return SCSFM_VIS_ERR_ARG;
  // 16-byte accesses only where both buffers allow them
  const long long n_vec = (aligned(in, 16) && aligned(out, 16)) ? total / 4 : 0;
  const long long lanes = n_vec + (total - 4 * n_vec);
  (void)hipGetLastError();
  hipLaunchKernelGGL(colourise_kernel, dim3(ceil_div(lanes, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     (unsigned)total, (unsigned)n_vec, (unsigned)(H * W), in, reinterpret_cast<const uint32_t*>(table),
                     (float)table_n, table_n - 1, divisors, (float)max_value, reciprocal,
                     reinterpret_cast<uint32_t*>(out));
  return launch_status();
}

}  // extern "C"
