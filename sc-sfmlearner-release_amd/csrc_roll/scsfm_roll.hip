// A volume that follows the camera (include/scsfm_roll.h): the shift of the five planes by whole voxels and the extraction
// of the surface points that leave with it.
//
//  shift_kernel      a pure streaming kernel: one thread per group of four consecutive floats of dst, the groups laid at
//                    16-byte boundaries of the address over the whole buffer of 5 nvox floats (so nx, and a plane's size,
//                    need be no multiple of 4: a group may span two rows or two planes).  The source of a dst element e is
//                    the element e + delta with one delta for the whole volume, delta = sx + nx (sy + ny sz); an element
//                    is kept when its voxel's source lies inside the volume.  A group whose four sources are all inside is
//                    one 16-byte load at 4-byte alignment (a dwordx4 global load needs no more) and one aligned 16-byte
//                    store; a group with none inside stores zeros and loads nothing; a mixed group loads the kept elements
//                    one by one.  The first and last group of a buffer that is not 16-byte aligned are partial.  One
//                    launch with one thread per group: at 2^29 voxels 2.6 million workgroups, far below the limit of a
//                    one-dimensional grid, and no loop that a cap would need.
//  count_kernel /    libscsfm_fuse.so's extraction restated (csrc_fuse/scsfm_fuse.hip: one workgroup per chunk of 1024
//  extract_kernel    consecutive voxels, one voxel per lane in four steps of 256, three ballots per step, the lane's place
//                    the number of set bits below it) with the keep box: a chunk whose voxels and their neighbours all lie
//                    inside it stores a count of 0 and returns before any load, a voxel of which that holds loads nothing,
//                    and a crossing is kept only when an end of its edge lies outside the box.
//  scan_kernel       one workgroup: the exclusive scan of the chunks' counts and the total.
//
// Arithmetic: the header's order, one rounding per operation (the pragma keeps the compiler from contracting a multiply
// and an add); the shift moves bits and computes nothing.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "scsfm_roll.h"

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kPlanes = SCSFM_ROLL_PLANES;
constexpr int kChunk = SCSFM_ROLL_CHUNK;
constexpr int kSteps = kChunk / kThreads;
constexpr int kScanPer = 8;  // counts per thread and step of the scan
constexpr int kWsHead = 4;   // ints in front of the counts

struct Dims {
  int nx, ny, nz;
};

struct Box {
  int x0, x1, y0, y1, z0, z1;
};

__device__ inline bool inside(const Box& k, int x, int y, int z) {
  return x >= k.x0 && x < k.x1 && y >= k.y0 && y < k.y1 && z >= k.z0 && z < k.z1;
}

// ---- the shift ----

// four floats as one access: the store at a 16-byte boundary, the load at the source's 4-byte alignment, which is all a
// dwordx4 global load asks for.  (The host simulator has no vector types of clang's kind: it copies 16 bytes.)
#ifdef __HOSTSIM__
struct Quad {
  float v[4];
};
inline Quad load4(const float* p) {
  Quad q;
  __builtin_memcpy(&q, p, 16);
  return q;
}
inline void store4(float* p, Quad q) { __builtin_memcpy(p, &q, 16); }
inline Quad zero4() { return Quad{{0.0f, 0.0f, 0.0f, 0.0f}}; }
#else
typedef float Quad __attribute__((ext_vector_type(4)));
typedef Quad QuadAt4 __attribute__((aligned(4)));
__device__ inline Quad load4(const float* p) { return *reinterpret_cast<const QuadAt4*>(p); }
__device__ inline void store4(float* p, Quad q) { *reinterpret_cast<Quad*>(p) = q; }
__device__ inline Quad zero4() { return Quad{0.0f, 0.0f, 0.0f, 0.0f}; }
#endif

// lead: floats between the 16-byte boundary below dst and dst (0 .. 3); total = 5 nvox (< 2^32); |sx| <= nx, |sy| <= ny,
// |sz| <= nz (the host clamps: beyond that everything is zero all the same)
__global__ __launch_bounds__(kThreads) void shift_kernel(Dims v, int sx, int sy, int sz, long long delta, int lead,
                                                         unsigned total, const float* __restrict__ src,
                                                         float* __restrict__ dst) {
  const long long group = (long long)blockIdx.x * kThreads + (long long)threadIdx.x;
  const long long e0 = 4 * group - lead;  // the group's first element; negative only in the first group
  if (e0 >= (long long)total) return;
  const unsigned nvox = (unsigned)v.nx * (unsigned)v.ny * (unsigned)v.nz;
  const unsigned first = e0 < 0 ? 0u : (unsigned)e0;
  const unsigned i = first % nvox;
  int x = (int)(i % (unsigned)v.nx);
  const unsigned row = i / (unsigned)v.nx;
  int y = (int)(row % (unsigned)v.ny), z = (int)(row / (unsigned)v.ny);
  bool valid[4], keep[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long e = e0 + j;
    valid[j] = e >= 0 && e < (long long)total;
    keep[j] = false;
    if (valid[j]) {
      const int ax = x + sx, ay = y + sy, az = z + sz;
      keep[j] = ax >= 0 && ax < v.nx && ay >= 0 && ay < v.ny && az >= 0 && az < v.nz;
      if (++x == v.nx) {
        x = 0;
        if (++y == v.ny) {
          y = 0;
          if (++z == v.nz) z = 0;  // (the next plane)
        }
      }
    }
  }
  if (keep[0] && keep[1] && keep[2] && keep[3]) {  // (kept elements are valid ones: the whole group is inside dst)
    store4(dst + e0, load4(src + (e0 + delta)));
    return;
  }
  if (valid[0] && valid[3] && !(keep[0] || keep[1] || keep[2] || keep[3])) {
    store4(dst + e0, zero4());
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // a group on the border of the kept box, or a partial one at an end of the buffer
    if (valid[j]) dst[e0 + j] = keep[j] ? src[e0 + j + delta] : 0.0f;
  }
}

// ---- the leaving extraction ----

struct Grid {
  int nx, ny, nz;
  float ox, oy, oz, voxel;
};

__device__ inline float centre(float o, int i, float s) {
  float c = (float)i + 0.5f;
  c = c * s;
  return o + c;
}

// the crossings of the chunk's step: three ballots, the lane's place among them and the step's total.  Every thread of
// the workgroup takes part in every step.
struct Place {
  int below, total;
};

__device__ inline Place place(bool e0, bool e1, bool e2, int* s_wave) {
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const unsigned long long b0 = __ballot(e0), b1 = __ballot(e1), b2 = __ballot(e2);
  const unsigned long long lower = (1ull << lane) - 1ull;
  int below = __popcll(b0 & lower) + __popcll(b1 & lower) + __popcll(b2 & lower);
  const int mine = __popcll(b0) + __popcll(b1) + __popcll(b2);
  __syncthreads();  // (the previous step's totals have been read)
  if (lane == 0) s_wave[wave] = mine;
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) {
    const int n = s_wave[k];
    if (k < wave) below += n;
    total += n;
  }
  return {below, total};
}

__device__ inline unsigned char colour_byte(float ca, float cb, float frac) {
  float c = cb - ca;
  c = frac * c;
  c = ca + c;
  c = c >= 0.0f ? c : 0.0f;
  c = c <= 1.0f ? c : 1.0f;
  c = c * 255.0f;
  c = c + 0.5f;
  return (unsigned char)(int)c;
}

// Do the voxels first .. last (linear indices, first <= last) and their +x / +y / +z neighbours inside the volume all lie
// inside the keep box?  Exact for a run inside one row; a run over several rows is taken as whole rows, one over several
// slices as whole slices: conservative, and it decides only what may be skipped, never a value.
__device__ inline bool chunk_is_kept(const Grid& v, const Box& k, int first, int last) {
  const int xa = first % v.nx, ra = first / v.nx, ya = ra % v.ny, za = ra / v.ny;
  const int xb = last % v.nx, rb = last / v.nx, yb = rb % v.ny, zb = rb / v.ny;
  const bool one_slice = za == zb, one_row = ra == rb;
  const int x_lo = one_row ? xa : 0, x_hi = one_row ? xb : v.nx - 1;
  const int y_lo = one_slice ? ya : 0, y_hi = one_slice ? yb : v.ny - 1;
  const int x_far = x_hi + 1 < v.nx ? x_hi + 1 : x_hi, y_far = y_hi + 1 < v.ny ? y_hi + 1 : y_hi;
  const int z_far = zb + 1 < v.nz ? zb + 1 : zb;
  return x_lo >= k.x0 && x_far < k.x1 && y_lo >= k.y0 && y_far < k.y1 && za >= k.z0 && z_far < k.z1;
}

template <bool kWrite>
__global__ __launch_bounds__(kThreads) void extract_kernel(Grid v, Box keep, const float* __restrict__ volume,
                                                           float min_weight, int* __restrict__ counts,
                                                           const int* __restrict__ offsets, int capacity,
                                                           float* __restrict__ xyz, unsigned char* __restrict__ rgb) {
  __shared__ int s_wave[kWaves];
  const int tid = (int)threadIdx.x;
  const int nvox = v.nx * v.ny * v.nz;
  const int chunk = (int)blockIdx.x;
  const int first = chunk * kChunk, last = first + kChunk - 1 < nvox - 1 ? first + kChunk - 1 : nvox - 1;
  if (chunk_is_kept(v, keep, first, last)) {  // (the same in every thread)
    if (!kWrite && tid == 0) counts[chunk] = 0;
    return;
  }
  const float* __restrict__ tsdf = volume;
  const float* __restrict__ weight = volume + (size_t)nvox;
  int running = kWrite ? offsets[chunk] : 0;
  for (int step = 0; step < kSteps; ++step) {
    const int i = first + step * kThreads + tid;
    bool e[3] = {false, false, false};
    int nb[3] = {0, 0, 0};
    int x = 0, y = 0, z = 0;
    float ta = 0.0f;
    if (i < nvox) {
      x = i % v.nx;
      const int row = i / v.nx;
      y = row % v.ny;
      z = row / v.ny;
      nb[0] = i + 1, nb[1] = i + v.nx, nb[2] = i + v.nx * v.ny;
      const bool in_a = inside(keep, x, y, z);
      // an edge can leave only when it exists and an end of it lies outside the box
      const bool may[3] = {x + 1 < v.nx && !(in_a && inside(keep, x + 1, y, z)),
                           y + 1 < v.ny && !(in_a && inside(keep, x, y + 1, z)),
                           z + 1 < v.nz && !(in_a && inside(keep, x, y, z + 1))};
      if (may[0] || may[1] || may[2]) {
        ta = tsdf[i];
        const bool seen = weight[i] >= min_weight;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (seen && may[k]) e[k] = weight[nb[k]] >= min_weight && ((ta < 0.0f) != (tsdf[nb[k]] < 0.0f));
        }
      }
    }
    const Place p = place(e[0], e[1], e[2], s_wave);
    if (kWrite) {
      int k_out = running + p.below;
      const float c[3] = {centre(v.ox, x, v.voxel), centre(v.oy, y, v.voxel), centre(v.oz, z, v.voxel)};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (e[k]) {
          if (k_out < capacity) {
            const float tb = tsdf[nb[k]];
            float frac = ta - tb;
            frac = ta / frac;
            float along = frac * v.voxel;
            along = c[k] + along;
            float* o = xyz + 3 * (size_t)k_out;
            o[0] = k == 0 ? along : c[0];
            o[1] = k == 1 ? along : c[1];
            o[2] = k == 2 ? along : c[2];
            unsigned char* q = rgb + 3 * (size_t)k_out;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              const float* plane = volume + (size_t)(2 + ch) * nvox;
              q[ch] = colour_byte(plane[i], plane[nb[k]], frac);
            }
          }
          ++k_out;
        }
      }
    }
    running += p.total;
  }
  if (!kWrite && tid == 0) counts[chunk] = running;
}

// exclusive scan of counts[0 .. n) into offsets, the total into *total: one workgroup, kThreads * kScanPer counts a step
__global__ __launch_bounds__(kThreads) void scan_kernel(int n, const int* __restrict__ counts, int* __restrict__ offsets,
                                                        int* __restrict__ total) {
  __shared__ int s_wave[kWaves];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  int carry = 0;
  for (int base = 0; base < n; base += kThreads * kScanPer) {
    const int k0 = base + tid * kScanPer;
    int c[kScanPer];
    int sum = 0;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
      c[j] = k0 + j < n ? counts[k0 + j] : 0;
      sum += c[j];
    }
    int incl = sum;
    for (int d = 1; d < kWave; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    __syncthreads();  // (the previous step's totals have been read)
    if (lane == kWave - 1) s_wave[wave] = incl;
    __syncthreads();
    int before = carry, all = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      if (k < wave) before += s_wave[k];
      all += s_wave[k];
    }
    int run = before + incl - sum;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
      if (k0 + j < n) offsets[k0 + j] = run;
      run += c[j];
    }
    carry += all;
  }
  if (tid == 0) *total = carry;
}

// ---- host side ----

// nvox, or 0 for sizes the library rejects
inline long long voxels(int nx, int ny, int nz) {
  if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
  const long long slice = (long long)nx * ny;  // (stepwise: the product of three ints can pass 2^63)
  if (slice > SCSFM_ROLL_MAX_VOXELS || slice * nz > SCSFM_ROLL_MAX_VOXELS) return 0;
  return slice * nz;
}

inline bool positive(float x) { return x > 0.0f && std::isfinite(x); }  // (false for a NaN)

inline int chunks(long long nvox) { return (int)((nvox + kChunk - 1) / kChunk); }

inline int clamp(int s, int n) { return s < -n ? -n : (s > n ? n : s); }

}  // namespace

extern "C" {

int scsfm_roll_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc_fuse/scsfm_fuse.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_roll_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

int scsfm_roll_shift(int nx, int ny, int nz, int sx, int sy, int sz, const float* src, float* dst, void* stream) {
  const long long nvox = voxels(nx, ny, nz);
  if (!nvox || !src || !dst || ((uintptr_t)src & 3) != 0 || ((uintptr_t)dst & 3) != 0) return SCSFM_ROLL_ERR_ARG;
  const size_t bytes = (size_t)nvox * kPlanes * sizeof(float);
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
  if (s0 < d0 + bytes && d0 < s0 + bytes) return SCSFM_ROLL_ERR_ARG;  // (the two overlap)
  sx = clamp(sx, nx), sy = clamp(sy, ny), sz = clamp(sz, nz);
  const long long delta = (long long)sx + (long long)nx * ((long long)sy + (long long)ny * sz);
  const int lead = (int)((d0 & 15) / 4);
  const long long total = nvox * kPlanes;                      // (at most 5 2^29 < 2^32)
  const long long groups = (total + lead + 3) / 4;
  const long long blocks = (groups + kThreads - 1) / kThreads;  // (at most 2 621 441)
  const Dims v = {nx, ny, nz};
  (void)hipGetLastError();
  hipLaunchKernelGGL(shift_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, v, sx, sy, sz, delta,
                     lead, (unsigned)total, src, dst);
  return (int)hipGetLastError();
}

size_t scsfm_roll_ws_bytes(int nx, int ny, int nz) {
  const long long nvox = voxels(nx, ny, nz);
  if (!nvox) return 0;
  return sizeof(int) * (size_t)(kWsHead + 2 * chunks(nvox));
}

int scsfm_roll_count(int nx, int ny, int nz, int x0, int x1, int y0, int y1, int z0, int z1, const float* volume,
                     float min_weight, void* ws, size_t ws_bytes, void* stream) {
  const long long nvox = voxels(nx, ny, nz);
  if (!nvox || !volume || !ws || ((uintptr_t)ws & 15) != 0 || ((uintptr_t)volume & 3) != 0 || !(min_weight >= 1.0f) ||
      !std::isfinite(min_weight) || ws_bytes < scsfm_roll_ws_bytes(nx, ny, nz))
    return SCSFM_ROLL_ERR_ARG;
  const Grid v = {nx, ny, nz, 0.0f, 0.0f, 0.0f, 1.0f};
  const Box keep = {x0, x1, y0, y1, z0, z1};
  const int n = chunks(nvox);
  int* head = (int*)ws;
  (void)hipGetLastError();
  hipLaunchKernelGGL((extract_kernel<false>), dim3((unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, v, keep, volume,
                     min_weight, head + kWsHead, (const int*)nullptr, 0, (float*)nullptr, (unsigned char*)nullptr);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, n, head + kWsHead, head + kWsHead + n,
                     head);
  return (int)hipGetLastError();
}

int scsfm_roll_extract(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, int x0, int x1, int y0, int y1,
                       int z0, int z1, const float* volume, float min_weight, const void* ws, size_t ws_bytes,
                       int capacity, float* xyz, unsigned char* rgb, void* stream) {
  const long long nvox = voxels(nx, ny, nz);
  if (!nvox || !volume || !ws || ((uintptr_t)ws & 15) != 0 || ((uintptr_t)volume & 3) != 0 || !(min_weight >= 1.0f) ||
      !std::isfinite(min_weight) || ws_bytes < scsfm_roll_ws_bytes(nx, ny, nz) || capacity < 0 ||
      (capacity > 0 && (!xyz || !rgb)) || !std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(oz) ||
      !positive(voxel))
    return SCSFM_ROLL_ERR_ARG;
  if (capacity == 0) return 0;
  const Grid v = {nx, ny, nz, ox, oy, oz, voxel};
  const Box keep = {x0, x1, y0, y1, z0, z1};
  const int n = chunks(nvox);
  const int* head = (const int*)ws;
  (void)hipGetLastError();
  hipLaunchKernelGGL((extract_kernel<true>), dim3((unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, v, keep, volume,
                     min_weight, (int*)nullptr, head + kWsHead + n, capacity, xyz, rgb);
  return (int)hipGetLastError();
}

}  // extern "C"
