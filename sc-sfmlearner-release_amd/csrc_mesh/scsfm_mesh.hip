// An indexed triangle mesh of the surface in a fused volume by marching tetrahedra (include/scsfm_mesh.h).
//
//  mesh_kernel<mode>  one workgroup (256 threads) per chunk of 1024 consecutive voxels, one voxel per lane in four steps
//                     of 256, as csrc_fuse/scsfm_fuse.hip's extract_kernel.  A lane reads the eight corners of the cell
//                     whose minimum voxel is its own (the y + 1 and z + 1 rows are rows along x, read by consecutive
//                     lanes) into two 8-bit masks, "seen" and "negative"; everything else is integer work on those.  A
//                     voxel that is not seen itself owns no vertex and no triangle (every tetrahedron holds corner 0)
//                     and reads nothing more.  One body serves the three passes, so they cannot disagree:
//                       kCount      the vertices and the triangles of the chunk -> two counts
//                       kVertices   the vertices, each voxel's first index and its 7-bit mask
//                       kTriangles  the triangles; an index is the owner's first index plus the set bits below the
//                                   edge's bit in the owner's mask: two loads, no search
//                     A lane's place among the wave's items is the sum over the bits of its count of the set bits
//                     below it in that bit's ballot; the waves' totals meet in LDS (8 ints: nothing else is staged);
//                     the chunk's base comes from scan_kernel.
//  scan_kernel        two workgroups, one per list: the exclusive scan of the chunks' counts in 64 bits and the total.
//
// Arithmetic: the header's order, one rounding per operation (the pragma keeps hipcc from contracting a multiply and an
// add); `/` is the correctly rounded expansion and fp32 denormals are kept on gfx950.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "scsfm_mesh.h"

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kChunk = SCSFM_MESH_CHUNK;
constexpr int kSteps = kChunk / kThreads;
constexpr int kScanPer = 8;  // counts per thread and step of the scan
static_assert(kScanPer * kThreads * 12LL * kChunk <= INT_MAX, "a step of the scan fits an int");

enum Mode { kCount, kVertices, kTriangles };

// corner of the cell that edge type e leads to (the header's offsets: +x +y +z +xy +xz +yz +xyz)
constexpr unsigned kEdgeCorner = 1u | 2u << 3 | 4u << 6 | 3u << 9 | 5u << 12 | 6u << 15 | 7u << 18;
// edge type of the offset d = q - p (3 bits at 3 d; d = 1 .. 7)
constexpr unsigned kEdgeOf = 0u << 3 | 1u << 6 | 3u << 9 | 2u << 12 | 4u << 15 | 5u << 18 | 6u << 21;
// the middle corners of the six tetrahedra (0, a, b, 7)
constexpr unsigned kTetA = 1u | 1u << 3 | 2u << 6 | 2u << 9 | 4u << 12 | 4u << 15;
constexpr unsigned kTetB = 3u | 5u << 3 | 3u << 6 | 6u << 9 | 5u << 12 | 6u << 15;
// The triangles of a 4-bit case (bit j: corner j of the tetrahedron's list is negative), from the header's I / O rule:
// bits 24 .. 25 the number of triangles, then 4 bits a vertex, first triangle first: the edge's two corners as places in
// the corner list, the lower in bits 0 .. 1 (the owner), the higher in bits 2 .. 3.
__device__ const unsigned kTri[16] = {0x0000000u, 0x1000c84u, 0x1000d94u, 0x29d8dc8u, 0x1000e98u, 0x29e4ec4u,
                                      0x28e4ed4u, 0x1000edcu, 0x1000edcu, 0x2de4e84u, 0x2ce4e94u, 0x1000e98u,
                                      0x2cd8d98u, 0x1000d94u, 0x1000c84u, 0x0000000u};

struct Grid {
  int nx, ny, nz;
  float ox, oy, oz, voxel;
};

// the workspace (the header's layout)
struct Ws {
  long long* head;  // V, T
  int* vcount;
  int* tcount;
  long long* voff;
  long long* toff;
  int* first;
  unsigned char* mask;
};

__host__ __device__ inline Ws carve(void* ws, int chunks, long long nvox) {
  char* p = (char*)ws;
  Ws w;
  w.head = (long long*)p;
  w.vcount = (int*)(p + 16);
  w.tcount = w.vcount + chunks;
  w.voff = (long long*)(p + 16 + 8 * (size_t)chunks);
  w.toff = w.voff + chunks;
  w.first = (int*)(p + 16 + 24 * (size_t)chunks);
  w.mask = (unsigned char*)(w.first + nvox);
  return w;
}

__device__ inline float centre(float o, int i, float s) {
  float c = (float)i + 0.5f;
  c = c * s;
  return o + c;
}

// a NaN coordinate is stored as the quiet NaN 0x7fc00000, whatever sign and payload the division left
__device__ inline float plain_nan(float x) { return x != x ? __builtin_nanf("") : x; }

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

// the lane's place among the workgroup's items of this step (n of them in this lane, n < 2^kBits) and the step's total.
// Every thread of the workgroup takes part in every step.
struct Place {
  int below, total;
};

template <int kBits>
__device__ inline Place place(int n, int* s_wave) {
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const unsigned long long lower = (1ull << lane) - 1ull;
  int below = 0, mine = 0;
#pragma unroll
  for (int bit = 0; bit < kBits; ++bit) {
    const unsigned long long b = __ballot((n >> bit) & 1);
    below += __popcll(b & lower) << bit;
    mine += __popcll(b) << bit;
  }
  __syncthreads();  // (the previous step's totals have been read)
  if (lane == 0) s_wave[wave] = mine;
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) {
    const int m = s_wave[k];
    if (k < wave) below += m;
    total += m;
  }
  return {below, total};
}

__device__ inline int corner_step(int k, int nx, int nxy) { return (k & 1) + ((k >> 1) & 1) * nx + (k >> 2) * nxy; }

template <int kMode>
__global__ __launch_bounds__(kThreads) void mesh_kernel(Grid v, const float* __restrict__ volume, float min_weight,
                                                        void* ws_raw, int capacity, float* __restrict__ xyz,
                                                        unsigned char* __restrict__ rgb, int* __restrict__ tri) {
  __shared__ int s_wave[2][kWaves];
  const int tid = (int)threadIdx.x;
  const int nxy = v.nx * v.ny;
  const int nvox = nxy * v.nz;
  const int chunk = (int)blockIdx.x;
  const Ws w = carve(ws_raw, (int)gridDim.x, nvox);
  const float* __restrict__ tsdf = volume;
  const float* __restrict__ weight = volume + (size_t)nvox;
  if (kMode != kCount && (w.head[0] > INT_MAX || w.head[1] > INT_MAX)) return;  // (refused, never wrapped)
  long long run_v = kMode == kVertices ? w.voff[chunk] : 0, run_t = kMode == kTriangles ? w.toff[chunk] : 0;
  for (int step = 0; step < kSteps; ++step) {
    const int i = chunk * kChunk + step * kThreads + tid;
    unsigned seen = 0u, neg = 0u;
    int x = 0, y = 0, z = 0;
    float ta = 0.0f;
    if (i < nvox && weight[i] >= min_weight) {
      x = i % v.nx;
      const int row = i / v.nx;
      y = row % v.ny;
      z = row / v.ny;
      ta = tsdf[i];
      seen = 1u, neg = ta < 0.0f ? 1u : 0u;
      const unsigned room = (x + 1 < v.nx ? 1u : 0u) | (y + 1 < v.ny ? 2u : 0u) | (z + 1 < v.nz ? 4u : 0u);
#pragma unroll
      for (int k = 1; k < 8; ++k) {
        if ((room & k) == (unsigned)k) {
          const int j = i + corner_step(k, v.nx, nxy);
          if (weight[j] >= min_weight) {
            seen |= 1u << k;
            if (tsdf[j] < 0.0f) neg |= 1u << k;
          }
        }
      }
    }
    // the seven edges the voxel owns
    unsigned edges = 0u;
    if (kMode != kTriangles) {
      const unsigned differs = (neg ^ (0u - (neg & 1u))) & seen & 0xfeu;  // corners seen and of the other sign
#pragma unroll
      for (int e = 0; e < 7; ++e) edges |= ((differs >> ((kEdgeCorner >> (3 * e)) & 7u)) & 1u) << e;
      if (!(seen & 1u)) edges = 0u;
    }
    // the six tetrahedra of the cell: their 4-bit cases (0 where a corner is not seen) and the number of triangles
    unsigned cases = 0u;
    int ntri = 0;
    if (kMode != kVertices) {
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const unsigned a = (kTetA >> (3 * k)) & 7u, b = (kTetB >> (3 * k)) & 7u;
        const unsigned need = 0x81u | 1u << a | 1u << b;
        if ((seen & need) == need) {
          const unsigned c4 = (neg & 1u) | ((neg >> a) & 1u) << 1 | ((neg >> b) & 1u) << 2 | ((neg >> 7) & 1u) << 3;
          const int inside = __popcll((unsigned long long)c4);
          ntri += inside == 2 ? 2 : (inside & 1);
          cases |= c4 << (4 * k);
        }
      }
    }
    if (kMode != kTriangles) {
      const Place p = place<3>(__popcll((unsigned long long)edges), s_wave[0]);
      if (kMode == kVertices) {
        const long long k0 = run_v + p.below;
        if (i < nvox) {
          w.first[i] = (int)k0;
          w.mask[i] = (unsigned char)edges;
        }
        if (edges) {
          int k_out = (int)k0;
          const float c[3] = {centre(v.ox, x, v.voxel), centre(v.oy, y, v.voxel), centre(v.oz, z, v.voxel)};
#pragma unroll
          for (int e = 0; e < 7; ++e) {
            if ((edges >> e) & 1u) {
              if (k_out < capacity) {
                const unsigned q = (kEdgeCorner >> (3 * e)) & 7u;
                const int j = i + corner_step((int)q, v.nx, nxy);
                const float tb = tsdf[j];
                float frac = ta - tb;
                frac = ta / frac;
                float along = frac * v.voxel;
                float* o = xyz + 3 * (size_t)k_out;
                o[0] = (q & 1u) ? plain_nan(c[0] + along) : c[0];
                o[1] = (q & 2u) ? plain_nan(c[1] + along) : c[1];
                o[2] = (q & 4u) ? plain_nan(c[2] + along) : c[2];
                unsigned char* u = rgb + 3 * (size_t)k_out;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                  const float* plane = volume + (size_t)(2 + ch) * nvox;
                  u[ch] = colour_byte(plane[i], plane[j], frac);
                }
              }
              ++k_out;
            }
          }
        }
      }
      run_v += p.total;
    }
    if (kMode != kVertices) {
      const Place p = place<4>(ntri, s_wave[1]);
      if (kMode == kTriangles && ntri) {
        int k_out = (int)(run_t + p.below);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const unsigned c4 = (cases >> (4 * k)) & 15u;
          if (c4 == 0u || c4 == 15u) continue;
          const unsigned word = kTri[c4];
          const int n = (int)(word >> 24);
          const unsigned corners = 0u | ((kTetA >> (3 * k)) & 7u) << 3 | ((kTetB >> (3 * k)) & 7u) << 6 | 7u << 9;
          const bool flip = (((unsigned)SCSFM_MESH_FLIP(k)) >> c4) & 1u;
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            if (t < n) {
              if (k_out < capacity) {
                int idx[3];
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                  const unsigned code = (word >> (4 * (3 * t + s))) & 15u;
                  const unsigned p0 = (corners >> (3 * (code & 3u))) & 7u, p1 = (corners >> (3 * (code >> 2))) & 7u;
                  const unsigned e = (kEdgeOf >> (3 * (p1 - p0))) & 7u;
                  const int owner = i + corner_step((int)p0, v.nx, nxy);
                  idx[s] = w.first[owner] + __popcll((unsigned long long)(w.mask[owner] & ((1u << e) - 1u)));
                }
                int* o = tri + 3 * (size_t)k_out;
                o[0] = idx[0];
                o[1] = flip ? idx[2] : idx[1];
                o[2] = flip ? idx[1] : idx[2];
              }
              ++k_out;
            }
          }
        }
      }
      run_t += p.total;
    }
  }
  if (kMode == kCount && tid == 0) {
    w.vcount[chunk] = (int)run_v;
    w.tcount[chunk] = (int)run_t;
  }
}

// exclusive scan of a list of n counts into 64-bit offsets and its total: workgroup 0 the vertices', 1 the triangles'.
// A step takes kThreads * kScanPer counts, whose sum fits an int; the carry between the steps is 64 bits wide.
__global__ __launch_bounds__(kThreads) void scan_kernel(int n, void* ws_raw, long long nvox) {
  __shared__ int s_wave[kWaves];
  const Ws w = carve(ws_raw, n, nvox);
  const int which = (int)blockIdx.x;
  const int* __restrict__ counts = which ? w.tcount : w.vcount;
  long long* __restrict__ offsets = which ? w.toff : w.voff;
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  long long carry = 0;
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
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      if (k < wave) before += s_wave[k];
      all += s_wave[k];
    }
    long long run = carry + (before + incl - sum);
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
      if (k0 + j < n) offsets[k0 + j] = run;
      run += c[j];
    }
    carry += all;
  }
  if (tid == 0) w.head[which] = carry;
}

// ---- host side ----

// nvox, or 0 for sizes the library rejects
inline long long voxels(int nx, int ny, int nz) {
  if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
  const long long slice = (long long)nx * ny;  // (stepwise: the product of three ints can pass 2^63)
  if (slice > SCSFM_MESH_MAX_VOXELS || slice * nz > SCSFM_MESH_MAX_VOXELS) return 0;
  return slice * nz;
}

inline bool positive(float x) { return x > 0.0f && std::isfinite(x); }  // (false for a NaN)

inline int chunks(long long nvox) { return (int)((nvox + kChunk - 1) / kChunk); }

inline bool bad_common(long long nvox, int nx, int ny, int nz, const float* volume, float min_weight, const void* ws,
                       size_t ws_bytes) {
  return !nvox || !volume || ((uintptr_t)volume & 3) != 0 || !ws || ((uintptr_t)ws & 15) != 0 ||
         !(min_weight >= 1.0f) || !std::isfinite(min_weight) || ws_bytes < scsfm_mesh_ws_bytes(nx, ny, nz);
}

}  // namespace

extern "C" {

int scsfm_mesh_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_mesh_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

size_t scsfm_mesh_ws_bytes(int nx, int ny, int nz) {
  const long long nvox = voxels(nx, ny, nz);
  if (!nvox) return 0;
  const size_t bytes = 16 + 24 * (size_t)chunks(nvox) + 5 * (size_t)nvox;
  return (bytes + 15) & ~(size_t)15;
}

int scsfm_mesh_count(int nx, int ny, int nz, const float* volume, float min_weight, void* ws, size_t ws_bytes,
                     void* stream) {
  const long long nvox = voxels(nx, ny, nz);
  if (bad_common(nvox, nx, ny, nz, volume, min_weight, ws, ws_bytes)) return SCSFM_MESH_ERR_ARG;
  const Grid v = {nx, ny, nz, 0.0f, 0.0f, 0.0f, 1.0f};
  const int n = chunks(nvox);
  (void)hipGetLastError();
  hipLaunchKernelGGL((mesh_kernel<kCount>), dim3((unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, v, volume,
                     min_weight, ws, 0, (float*)nullptr, (unsigned char*)nullptr, (int*)nullptr);
  const int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(scan_kernel, dim3(2), dim3(kThreads), 0, (hipStream_t)stream, n, ws, nvox);
  return (int)hipGetLastError();
}

int scsfm_mesh_vertices(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, const float* volume,
                        float min_weight, void* ws, size_t ws_bytes, size_t n_vertices, int capacity, float* xyz,
                        unsigned char* rgb, void* stream) {
  const long long nvox = voxels(nx, ny, nz);
  if (bad_common(nvox, nx, ny, nz, volume, min_weight, ws, ws_bytes) || n_vertices > (size_t)INT_MAX || capacity < 0 ||
      (capacity > 0 && (!xyz || !rgb || ((uintptr_t)xyz & 3) != 0)) || !std::isfinite(ox) || !std::isfinite(oy) ||
      !std::isfinite(oz) || !positive(voxel))
    return SCSFM_MESH_ERR_ARG;
  const Grid v = {nx, ny, nz, ox, oy, oz, voxel};
  (void)hipGetLastError();
  hipLaunchKernelGGL((mesh_kernel<kVertices>), dim3((unsigned)chunks(nvox)), dim3(kThreads), 0, (hipStream_t)stream, v,
                     volume, min_weight, ws, capacity, xyz, rgb, (int*)nullptr);
  return (int)hipGetLastError();
}

int scsfm_mesh_triangles(int nx, int ny, int nz, const float* volume, float min_weight, const void* ws, size_t ws_bytes,
                         size_t n_vertices, size_t n_triangles, int capacity, int* tri, void* stream) {
  const long long nvox = voxels(nx, ny, nz);
  if (bad_common(nvox, nx, ny, nz, volume, min_weight, ws, ws_bytes) || n_vertices > (size_t)INT_MAX ||
      n_triangles > (size_t)INT_MAX || capacity < 0 || (capacity > 0 && (!tri || ((uintptr_t)tri & 3) != 0)))
    return SCSFM_MESH_ERR_ARG;
  if (capacity == 0) return 0;
  const Grid v = {nx, ny, nz, 0.0f, 0.0f, 0.0f, 1.0f};
  (void)hipGetLastError();
  hipLaunchKernelGGL((mesh_kernel<kTriangles>), dim3((unsigned)chunks(nvox)), dim3(kThreads), 0, (hipStream_t)stream, v,
                     volume, min_weight, const_cast<void*>(ws), capacity, (float*)nullptr, (unsigned char*)nullptr, tri);
  return (int)hipGetLastError();
}

}  // extern "C"
