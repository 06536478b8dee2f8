// Adam over every parameter tensor in one launch (include/scsfm_opt.h).  Seven streams -- read p, g, m, v; write p, m, v
// -- 28 bytes per element, no reuse, no LDS: the kernel is bound by memory traffic and hides latency with occupancy.
//
// Work split: workgroup i reads entry i of the chunk map, {tensor, chunk}, and that tensor's record of the table; both are
// uniform over the workgroup.  A chunk is kChunk = 2048 consecutive elements of one tensor (the last one of a tensor is
// shorter).  Where the chunk's four addresses are 16-byte aligned a thread takes kUnroll = 2 units of four floats, 256
// units apart, and the up to three elements behind the last whole unit go one to a thread; otherwise a thread takes eight
// single floats, 256 apart.  All loads of a thread are issued before the first use.
//
// Arithmetic: the header's order, one rounding per line.  The pragma below keeps the compiler from contracting a
// multiply and an add of two statements into one fused operation (hipcc's default is -ffp-contract=fast), `/` and sqrtf
// are the correctly rounded expansions, and fp32 denormals are kept on gfx950.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "scsfm_opt.h"

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kThreads = 256;
constexpr int kChunk = SCSFM_OPT_CHUNK;
constexpr int kUnroll = 2;                          // 16-byte units in flight per thread and stream
constexpr int kScalar = kChunk / kThreads;          // 4-byte units per thread on the scalar path
static_assert(kChunk == kThreads * 4 * kUnroll, "a chunk is kUnroll 16-byte units per thread");

struct Record {
  float* p;
  const float* g;
  long long off;
  int n;
  float step_size, bc2_sqrt, wd;
};
static_assert(sizeof(Record) == SCSFM_OPT_RECORD_BYTES, "the table's record is the header's");

// an entry of the chunk map
struct Entry {
  int tensor, chunk;
};

struct Consts {
  float b1c, b2, b2c, eps;
};

// one element: the header's lines, in its order
__device__ inline void adam(float& p, float g, float& m, float& v, const Record& r, const Consts& c) {
  float t;
  if (r.wd != 0.0f) {
    t = r.wd * p;
    g = g + t;
  }
  t = g - m;
  t = c.b1c * t;
  m = m + t;
  const float a = v * c.b2;
  t = c.b2c * g;
  t = t * g;
  v = a + t;
  float d = sqrtf(v);
  d = d / r.bc2_sqrt;
  d = d + c.eps;
  t = m / d;
  t = r.step_size * t;
  p = p - t;
}

__device__ inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__global__ __launch_bounds__(kThreads) void adam_kernel(const Record* __restrict__ table, int n_tensors,
                                                        const Entry* __restrict__ map, float* __restrict__ exp_avg,
                                                        float* __restrict__ exp_avg_sq, Consts c) {
  const Entry e = map[blockIdx.x];
  if (e.tensor < 0 || e.tensor >= n_tensors || e.chunk < 0) return;
  const Record r = table[e.tensor];
  const long long start = (long long)e.chunk * kChunk;
  if (start >= r.n || !r.g) return;
  const int len = (int)(r.n - start < kChunk ? r.n - start : kChunk);
  float* __restrict__ p = r.p + start;
  const float* __restrict__ g = r.g + start;
  float* __restrict__ m = exp_avg + r.off + start;
  float* __restrict__ v = exp_avg_sq + r.off + start;
  const int tid = (int)threadIdx.x;
  if (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v)) {
    const int units = len >> 2;
    float4 P[kUnroll], G[kUnroll], M[kUnroll], V[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int i = tid + u * kThreads;
      if (i < units) {
        P[u] = reinterpret_cast<const float4*>(p)[i];
        G[u] = reinterpret_cast<const float4*>(g)[i];
        M[u] = reinterpret_cast<const float4*>(m)[i];
        V[u] = reinterpret_cast<const float4*>(v)[i];
      }
    }
    // the elements behind the last whole unit (fewer than four, in a tensor's last chunk only)
    const int j = (units << 2) + tid;
    float pj = 0, gj = 0, mj = 0, vj = 0;
    if (j < len) { pj = p[j]; gj = g[j]; mj = m[j]; vj = v[j]; }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int i = tid + u * kThreads;
      if (i < units) {
        adam(P[u].x, G[u].x, M[u].x, V[u].x, r, c);
        adam(P[u].y, G[u].y, M[u].y, V[u].y, r, c);
        adam(P[u].z, G[u].z, M[u].z, V[u].z, r, c);
        adam(P[u].w, G[u].w, M[u].w, V[u].w, r, c);
        reinterpret_cast<float4*>(p)[i] = P[u];
        reinterpret_cast<float4*>(m)[i] = M[u];
        reinterpret_cast<float4*>(v)[i] = V[u];
      }
    }
    if (j < len) {
      adam(pj, gj, mj, vj, r, c);
      p[j] = pj; m[j] = mj; v[j] = vj;
    }
  } else {
    float P[kScalar], G[kScalar], M[kScalar], V[kScalar];
#pragma unroll
    for (int u = 0; u < kScalar; ++u) {
      const int i = tid + u * kThreads;
      if (i < len) { P[u] = p[i]; G[u] = g[i]; M[u] = m[i]; V[u] = v[i]; }
    }
#pragma unroll
    for (int u = 0; u < kScalar; ++u) {
      const int i = tid + u * kThreads;
      if (i < len) {
        adam(P[u], G[u], M[u], V[u], r, c);
        p[i] = P[u]; m[i] = M[u]; v[i] = V[u];
      }
    }
  }
}

inline bool unit_interval(double b) { return b >= 0.0 && b < 1.0; }  // (false for a NaN)

}  // namespace

extern "C" {

int scsfm_opt_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_opt_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

int scsfm_opt_adam_step_f32(const void* table, int n_tensors, const void* chunk_map, int n_chunks, float* exp_avg,
                            float* exp_avg_sq, double beta1, double beta2, double eps, void* stream) {
  if (!table || !chunk_map || !exp_avg || !exp_avg_sq || n_tensors <= 0 || n_chunks <= 0 || !unit_interval(beta1) ||
      !unit_interval(beta2) || !(eps >= 0.0) || !std::isfinite(eps) || ((uintptr_t)table & 7) != 0 ||
      ((uintptr_t)chunk_map & 7) != 0 || ((uintptr_t)exp_avg & 15) != 0 || ((uintptr_t)exp_avg_sq & 15) != 0)
    return -1;
  (void)hipGetLastError();
  const Consts c = {(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps};
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, (hipStream_t)stream,
                     (const Record*)table, n_tensors, (const Entry*)chunk_map, exp_avg, exp_avg_sq, c);
  return (int)hipGetLastError();
}

}  // extern "C"
