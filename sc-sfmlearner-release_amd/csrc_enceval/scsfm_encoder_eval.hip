// The ResNet encoder's glue in eval mode (include/scsfm_enceval.h): BatchNorm from the running statistics fused with the
// residual add and the ReLU behind it, the stem's BatchNorm / ReLU fused with its 3x3 / stride 2 / pad 1 max-pool, and
// that max-pool alone.  Eval-mode BatchNorm is a per-channel affine map: one launch per operation, no reduction, no
// workspace, no LDS, no barrier.  Everything here is bound by memory traffic.
//
// Work split: the unit of work is a WAVE's task, not a workgroup's, and a task lies inside one (b, c) plane, so the
// channel is wave-uniform -- its four per-channel values are fetched and invstd = 1 / sqrt(running_var + eps) is formed
// once per task (the wave's index goes through readfirstlane, so the compiler keeps the channel and those loads scalar).
// The four waves of a workgroup take four consecutive tasks, which may be four different planes: layer 4 at 256 x 832
// has planes of 8 x 26 = 208 floats, 52 16-byte units, and a workgroup per plane would idle 204 of 256 threads there.
// A grid of at most kMaxBlocks workgroups strides over the tasks.
//
// BatchNorm (bn_eval_kernel): a plane is H*W contiguous floats, cut into units of V floats (V = 4, one 16-byte access,
// when H*W is a multiple of 4 -- every plane base is 16-byte aligned then -- and the pointers are; V = 1 otherwise) and
// into chunks of kUnroll * 64 units.  A lane's kUnroll units are 64 units apart, so every access of the wave covers
// 1 KiB (V = 4) of consecutive bytes, and all loads of a task are issued before the first use.
//
// Stem / pool (pool_kernel): a lane owns one pooled row's strip of V input columns (V = 4: W % 4 == 0, one 16-byte load
// per input row and two pooled columns; V = 2 with guarded scalar accesses and one pooled column otherwise) and reads
// the three input rows 2ph-1 .. 2ph+1 of its windows plus the one column to the left of the strip.  The lanes of a wave
// lie side by side along a row and consecutive pooled rows follow each other, so the left column and the row shared
// with the pooled row above are served by the caches: DRAM sees x once.  The lane stores relu(bn(x)) of its rows 2ph and
// 2ph+1 (every entry of f0 has exactly one owner) and the pooled values; the scan is row-major, "take the candidate if
// it is greater or a NaN" (include/scsfm_enc.h's rule; only the value is kept).
#include <hip/hip_runtime.h>

#include "scsfm_enceval.h"

namespace scsfm_enceval {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kUnroll = 4;        // units in flight per lane in the BatchNorm kernel
constexpr int kMaxBlocks = 8192;  // 8 workgroups of 4 waves per CU on 256 CUs, four rounds

template <int V>
struct Pack {
  float v[V];
};
template <int V>
__device__ inline Pack<V> load(const float* __restrict__ p);
template <>
__device__ inline Pack<1> load<1>(const float* __restrict__ p) {
  return {{p[0]}};
}
template <>
__device__ inline Pack<4> load<4>(const float* __restrict__ p) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  return {{t.x, t.y, t.z, t.w}};
}
__device__ inline void store(float* __restrict__ p, const Pack<1>& a) { p[0] = a.v[0]; }
__device__ inline void store(float* __restrict__ p, const Pack<4>& a) {
  float4 t;
  t.x = a.v[0]; t.y = a.v[1]; t.z = a.v[2]; t.w = a.v[3];
  *reinterpret_cast<float4*>(p) = t;
}

__device__ inline int imin(int a, int b) { return a < b ? a : b; }
__device__ inline int imax(int a, int b) { return a > b ? a : b; }

__device__ inline float relu(float v) { return v > 0.f ? v : (v != v ? v : 0.f); }

// one channel's map; the expression is csrc_enc/scsfm_encoder.hip's bn_value(xhat) with the running statistics
struct Affine {
  float mean, invstd, ga, be;
};
__device__ inline Affine affine_of(int c, float eps, const float* __restrict__ gamma, const float* __restrict__ beta,
                                   const float* __restrict__ running_mean, const float* __restrict__ running_var) {
  return {running_mean[c], 1.0f / sqrtf(running_var[c] + eps), gamma[c], beta[c]};
}
__device__ inline float bn_value(float x, const Affine& a) { return fmaf((x - a.mean) * a.invstd, a.ga, a.be); }

// this wave's index in the workgroup, as a scalar
__device__ inline int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// tasks = planes * chunks (at most the number of elements, below 2^31: t + stride cannot wrap); a plane has `per` units
// of V floats
template <int V, int MODE>
__global__ __launch_bounds__(kThreads) void bn_eval_kernel(unsigned tasks, int C, int HW, int per, int chunks, float eps,
                                                            const float* __restrict__ x,
                                                            const float* __restrict__ identity,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            const float* __restrict__ running_mean,
                                                            const float* __restrict__ running_var,
                                                            float* __restrict__ y) {
  const int lane = threadIdx.x & (kWave - 1);
  const unsigned stride = gridDim.x * kWaves;
  for (unsigned t = blockIdx.x * kWaves + wave_index(); t < tasks; t += stride) {
    const int plane = (int)(t / (unsigned)chunks), chunk = (int)(t - (unsigned)plane * (unsigned)chunks);
    const Affine a = affine_of(plane % C, eps, gamma, beta, running_mean, running_var);
    const size_t base = (size_t)plane * HW;
    const int u0 = chunk * (kUnroll * kWave) + lane;
    if (u0 >= per) continue;
    Pack<V> p[kUnroll], r[kUnroll];
    size_t off[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      off[j] = base + (size_t)imin(u0 + j * kWave, per - 1) * V;
      p[j] = load<V>(x + off[j]);
      if (MODE == 2) r[j] = load<V>(identity + off[j]);
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      if (u0 + j * kWave < per) {
        Pack<V> o;
#pragma unroll
        for (int k = 0; k < V; ++k) {
          float v = bn_value(p[j].v[k], a);
          if (MODE == 2) v += r[j].v[k];
          o.v[k] = MODE == 0 ? v : relu(v);
        }
        store(y + off[j], o);
      }
    }
  }
}

// one candidate of the scan: taken if it is greater than the best so far, or a NaN
__device__ inline void take(float v, float& best) {
  if (v > best || v != v) best = v;
}

// tasks = planes * chunks; a plane has PH * Wq items (a pooled row's strip of V columns), 64 to a chunk.
// FUSED: x goes through relu(bn(.)) first and the result is stored to f0; otherwise x is pooled as it is.
template <int V, bool FUSED>
__global__ __launch_bounds__(kThreads) void pool_kernel(unsigned tasks, int C, int H, int W, int PH, int PW, int Wq,
                                                         int chunks, float eps, const float* __restrict__ x,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ running_mean,
                                                         const float* __restrict__ running_var, float* __restrict__ f0,
                                                         float* __restrict__ pooled) {
  constexpr int NP = V / 2;
  const int lane = threadIdx.x & (kWave - 1);
  const int items = PH * Wq;
  const unsigned stride = gridDim.x * kWaves;
  for (unsigned t = blockIdx.x * kWaves + wave_index(); t < tasks; t += stride) {
    const int plane = (int)(t / (unsigned)chunks), chunk = (int)(t - (unsigned)plane * (unsigned)chunks);
    Affine a = {0.f, 1.f, 1.f, 0.f};
    if (FUSED) a = affine_of(plane % C, eps, gamma, beta, running_mean, running_var);
    const int item = chunk * kWave + lane;
    if (item >= items) continue;
    const int ph = item / Wq, col0 = (item - ph * Wq) * V;
    const size_t base = (size_t)plane * H * W;
    const float* xp = x + base;
    // v[r][0] is the column left of the strip, v[r][1..V] the strip, of rows 2ph-1, 2ph, 2ph+1 (clamped into the plane:
    // what lies outside is loaded from a neighbour and never looked at)
    float v[3][V + 1];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float* row = xp + (size_t)imin(imax(2 * ph - 1 + r, 0), H - 1) * W;
      v[r][0] = row[imax(col0 - 1, 0)];
      if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(row + col0);
        v[r][1] = q.x; v[r][2] = q.y; v[r][3] = q.z; v[r][4] = q.w;
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v[r][1 + j] = row[imin(col0 + j, W - 1)];
      }
    }
    if (FUSED) {
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int j = 0; j <= V; ++j) v[r][j] = relu(bn_value(v[r][j], a));
#pragma unroll
      for (int r = 1; r < 3; ++r) {
        const int h = 2 * ph - 1 + r;
        if (h < H) {
          float* row = f0 + base + (size_t)h * W;
          if constexpr (V == 4) {
            float4 q;
            q.x = v[r][1]; q.y = v[r][2]; q.z = v[r][3]; q.w = v[r][4];
            *reinterpret_cast<float4*>(row + col0) = q;
          } else {
#pragma unroll
            for (int j = 0; j < V; ++j)
              if (col0 + j < W) row[col0 + j] = v[r][1 + j];
          }
        }
      }
    }
    float best[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) best[q] = -INFINITY;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int h = 2 * ph - 1 + r;
      if (h < 0 || h >= H) continue;
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        // window q of the strip: columns col0 + 2q - 1 .. col0 + 2q + 1, the middle one always inside the plane
        if (col0 + 2 * q > 0) take(v[r][2 * q], best[q]);
        take(v[r][2 * q + 1], best[q]);
        if (col0 + 2 * q + 1 < W) take(v[r][2 * q + 2], best[q]);
      }
    }
    float* dst = pooled + (size_t)plane * PH * PW + (size_t)ph * PW + col0 / 2;
    if constexpr (V == 4) {
      float2 q;
      q.x = best[0]; q.y = best[1];
      *reinterpret_cast<float2*>(dst) = q;
    } else {
      dst[0] = best[0];
    }
  }
}

inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

inline bool shape_ok(int B, int C, int H, int W) {
  return B > 0 && C > 0 && H > 0 && W > 0 && (long long)B * C * H * W < (1ll << 31);
}

inline bool eps_ok(double eps) { return eps >= 0.0 && eps <= 1.7976931348623157e308; }  // (false for a NaN)

inline bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

inline int blocks_for(long long tasks) {
  const long long n = ceil_div(tasks, kWaves);
  return (int)(n < kMaxBlocks ? n : kMaxBlocks);
}

inline int launch_status() { return (int)hipGetLastError(); }

template <int V, bool FUSED>
inline void launch_pool(int B, int C, int H, int W, float eps, const float* x, const float* gamma, const float* beta,
                        const float* running_mean, const float* running_var, float* f0, float* pooled, void* stream) {
  const int PH = (H - 1) / 2 + 1, PW = (W - 1) / 2 + 1, Wq = (W + V - 1) / V;
  const int chunks = (int)ceil_div((long long)PH * Wq, kWave);
  const long long tasks = (long long)B * C * chunks;
  hipLaunchKernelGGL((pool_kernel<V, FUSED>), dim3(blocks_for(tasks)), dim3(kThreads), 0, (hipStream_t)stream,
                     (unsigned)tasks, C, H, W, PH, PW, Wq, chunks, eps, x, gamma, beta, running_mean, running_var, f0,
                     pooled);
}

}  // namespace scsfm_enceval

using namespace scsfm_enceval;

#define SCSFM_ENCEVAL_LAUNCH(V, MODE)                                                                       \
  hipLaunchKernelGGL((bn_eval_kernel<V, MODE>), grid, block, 0, (hipStream_t)stream, (unsigned)tasks, C, HW, per, \
                     chunks, (float)eps, x, identity, gamma, beta, running_mean, running_var, y)
#define SCSFM_ENCEVAL_BY_MODE(V)                  \
  do {                                            \
    if (mode == 0) SCSFM_ENCEVAL_LAUNCH(V, 0);      \
    else if (mode == 1) SCSFM_ENCEVAL_LAUNCH(V, 1); \
    else SCSFM_ENCEVAL_LAUNCH(V, 2);                \
  } while (0)

extern "C" {

int scsfm_enceval_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_enceval_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

int scsfm_enceval_bn_f32(int B, int C, int H, int W, int mode, double eps, const float* x, const float* identity,
                         const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                         float* y, void* stream) {
  if (!shape_ok(B, C, H, W) || mode < 0 || mode > 2 || !eps_ok(eps) || !x || (mode == 2 && !identity) || !gamma ||
      !beta || !running_mean || !running_var || !y)
    return -1;
  (void)hipGetLastError();
  const int HW = H * W;
  const bool vec = HW % 4 == 0 && aligned16(x) && aligned16(y) && (mode != 2 || aligned16(identity));
  const int per = vec ? HW / 4 : HW;
  const int chunks = (int)ceil_div(per, kUnroll * kWave);
  const long long tasks = (long long)B * C * chunks;
  const dim3 grid(blocks_for(tasks)), block(kThreads);
  if (vec) SCSFM_ENCEVAL_BY_MODE(4);
  else SCSFM_ENCEVAL_BY_MODE(1);
  return launch_status();
}

int scsfm_enceval_bn_relu_pool_f32(int B, int C, int H, int W, double eps, const float* x, const float* gamma,
                                   const float* beta, const float* running_mean, const float* running_var, float* f0,
                                   float* pooled, void* stream) {
  if (!shape_ok(B, C, H, W) || !eps_ok(eps) || !x || !gamma || !beta || !running_mean || !running_var || !f0 || !pooled)
    return -1;
  (void)hipGetLastError();
  // (W % 4 == 0: every row of x and f0 starts 16-byte aligned and every pooled row, W / 2 floats, 8-byte aligned)
  if (W % 4 == 0 && aligned16(x) && aligned16(f0) && aligned16(pooled))
    launch_pool<4, true>(B, C, H, W, (float)eps, x, gamma, beta, running_mean, running_var, f0, pooled, stream);
  else
    launch_pool<2, true>(B, C, H, W, (float)eps, x, gamma, beta, running_mean, running_var, f0, pooled, stream);
  return launch_status();
}

int scsfm_enceval_maxpool_f32(int B, int C, int H, int W, const float* x, float* out, void* stream) {
  if (!shape_ok(B, C, H, W) || !x || !out) return -1;
  (void)hipGetLastError();
  if (W % 4 == 0 && aligned16(x) && aligned16(out))
    launch_pool<4, false>(B, C, H, W, 0.f, x, nullptr, nullptr, nullptr, nullptr, nullptr, out, stream);
  else
    launch_pool<2, false>(B, C, H, W, 0.f, x, nullptr, nullptr, nullptr, nullptr, nullptr, out, stream);
  return launch_status();
}

}  // extern "C"
