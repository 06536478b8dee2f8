// The validation pictures of train.py --log-output (include/scsfm_vlog.h).
//
//  input      float [N, 3, H, W] -> 0.45f + x * 0.225f, planar floats and / or interleaved bytes; one lane per pixel:
//             three coalesced loads, three coalesced stores, three byte stores.
//  target     the target disparity of a ground-truth depth, one lane per pixel.
//  max        one pass over the maps: every lane folds its pixels into an order-preserving uint32 key (a NaN is the
//             largest key), the wave folds with shuffles, the block through LDS, and one lane issues one integer
//             atomicMax into the image's word of `out`; a second launch of N lanes turns the keys back into floats.
//  map        one lane per pixel: 4 B read, one 16-byte table entry (the tables, at most 160 KB, stay in L2), four
//             coalesced plane stores and / or one 32-bit word of bytes.  Three pictures of one image are made per
//             validation pass, so the launches, not the bytes, are what this costs: nothing here is vectorised further.
//
// Exactness: every `/` is the correctly rounded float32 division (the project's flags relax nothing) and contraction is
// off, so x * 0.225f + 0.45f and (x / d) * n round twice as numpy does.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "scsfm_vlog.h"

#pragma clang fp contract(off)

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocksPerImage = 64;   // of the maximum: 64 atomics per image at the most
constexpr int kPixelsPerBlock = kThreads * 8;
constexpr long long kMaxPixels = (long long)1 << 29;  // 4 floats out per pixel: every element index fits 32 bits
constexpr int kMaxTable = 1 << 24;                    // (float) table_n is exact

struct alignas(16) Float4 { float x, y, z, w; };

// (uint8) min(max(255 v, 0), 255); a NaN fails the first comparison and becomes 0
__device__ inline uint32_t to_byte(float v) {
  float t = 255.0f * v;
  t = t > 0.0f ? t : 0.0f;
  t = t < 255.0f ? t : 255.0f;
  return (uint32_t)(int)t;
}

// ---- the input picture ----

__global__ void __launch_bounds__(kThreads)
input_kernel(unsigned total, unsigned HW, const float* __restrict__ in, float* __restrict__ out_f,
             unsigned char* __restrict__ out_u8) {
  const unsigned gid = blockIdx.x * kThreads + threadIdx.x;
  if (gid >= total) return;
  const unsigned n = gid / HW, p = gid - n * HW;
  const size_t base = (size_t)3 * n * HW + p;
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float scaled = in[base + (size_t)c * HW] * 0.225f;
    v[c] = 0.45f + scaled;
  }
  if (out_f) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out_f[base + (size_t)c * HW] = v[c];
  }
  if (out_u8) {
    unsigned char* __restrict__ px = out_u8 + (size_t)3 * gid;
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = (unsigned char)to_byte(v[c]);
  }
}

// ---- the target disparity ----

__global__ void __launch_bounds__(kThreads)
target_kernel(unsigned total, const float* __restrict__ in, float* __restrict__ out) {
  const unsigned gid = blockIdx.x * kThreads + threadIdx.x;
  if (gid >= total) return;
  const float d = in[gid];
  float r = 1.0f / (d == 0.0f ? 1000.0f : d);
  r = r < 0.0f ? 0.0f : r;  // (a NaN fails both comparisons and stays)
  r = r > 10.0f ? 10.0f : r;
  out[gid] = r;
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
  const float* __restrict__ img = in + (size_t)n * HW;
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

// ---- a map as a picture ----

__global__ void __launch_bounds__(kThreads)
map_kernel(unsigned total, unsigned HW, const float* __restrict__ in, const Float4* __restrict__ table, float nf,
           int last, const float* __restrict__ divisors, float max_value, float* __restrict__ out_f,
           uint32_t* __restrict__ out_u8) {
  const unsigned gid = blockIdx.x * kThreads + threadIdx.x;
  if (gid >= total) return;
  const unsigned n = gid / HW, p = gid - n * HW;
  const float d = divisors ? divisors[n] : max_value;
  const float xa = (in[gid] / d) * nf;
  const bool bad = xa != xa;
  int idx = xa >= nf ? last : (int)(xa > 0.0f ? xa : 0.0f);  // (a NaN fails both comparisons: entry 0, not used)
  idx = idx < 0 ? 0 : (idx > last ? last : idx);
  Float4 c = table[idx];
  if (bad) c.x = c.y = c.z = c.w = 0.0f;
  if (out_f) {
    float* __restrict__ o = out_f + (size_t)4 * n * HW + p;
    o[0] = c.x;
    o[HW] = c.y;
    o[(size_t)2 * HW] = c.z;
    o[(size_t)3 * HW] = c.w;
  }
  if (out_u8) out_u8[gid] = to_byte(c.x) | (to_byte(c.y) << 8) | (to_byte(c.z) << 16) | (to_byte(c.w) << 24);
}

inline int ceil_div(long long a, int b) { return (int)((a + b - 1) / b); }
inline int launch_status() { return (int)hipGetLastError(); }
inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" {

int scsfm_vlog_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_vlog_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

int scsfm_vlog_input_picture(int N, int H, int W, const float* in, float* out_f, unsigned char* out_u8, void* stream) {
  if (N < 1 || H < 1 || W < 1 || !in || (!out_f && !out_u8)) return SCSFM_VLOG_ERR_ARG;
  if (!aligned(in, 4) || !aligned(out_f, 4)) return SCSFM_VLOG_ERR_ARG;
  const long long total = (long long)N * H * W;
  if (total >= kMaxPixels) return SCSFM_VLOG_ERR_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(input_kernel, dim3(ceil_div(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     (unsigned)total, (unsigned)(H * W), in, out_f, out_u8);
  return launch_status();
}

int scsfm_vlog_target_disparity(int N, int HW, const float* in, float* out, void* stream) {
  if (N < 1 || HW < 1 || !in || !out || !aligned(in, 4) || !aligned(out, 4)) return SCSFM_VLOG_ERR_ARG;
  const long long total = (long long)N * HW;
  if (total >= kMaxPixels) return SCSFM_VLOG_ERR_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(target_kernel, dim3(ceil_div(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     (unsigned)total, in, out);
  return launch_status();
}

int scsfm_vlog_image_max(int N, int HW, const float* in, float* out, void* stream) {
  if (N < 1 || HW < 1 || !in || !out || !aligned(in, 4) || !aligned(out, 4)) return SCSFM_VLOG_ERR_ARG;
  if ((long long)N * HW >= kMaxPixels) return SCSFM_VLOG_ERR_ARG;
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

int scsfm_vlog_map_picture(int N, int H, int W, const float* in, const float* table, int table_n,
                           const float* divisors, double max_value, float* out_f, unsigned char* out_u8, void* stream) {
  if (N < 1 || H < 1 || W < 1 || !in || !table || table_n < 1 || table_n > kMaxTable || (!out_f && !out_u8))
    return SCSFM_VLOG_ERR_ARG;
  if (!aligned(in, 4) || !aligned(table, 16) || !aligned(divisors, 4) || !aligned(out_f, 4) || !aligned(out_u8, 4))
    return SCSFM_VLOG_ERR_ARG;
  const long long total = (long long)N * H * W;
  if (total >= kMaxPixels) return SCSFM_VLOG_ERR_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(map_kernel, dim3(ceil_div(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     (unsigned)total, (unsigned)(H * W), in, reinterpret_cast<const Float4*>(table), (float)table_n,
                     table_n - 1, divisors, (float)max_value, out_f, reinterpret_cast<uint32_t*>(out_u8));
  return launch_status();
}

}  // extern "C"
