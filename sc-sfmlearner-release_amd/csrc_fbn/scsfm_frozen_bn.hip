// The backward of the ResNet encoder's BatchNorm with frozen statistics (include/scsfm_fbn.h), fused with the backward of
// the residual add and the ReLU behind it.  The forward is csrc_enceval's bn_eval_kernel; with the running statistics
// held, the map is affine per channel, so
//     dx = m * scale[c],  scale[c] = gamma[c] * invstd[c],  m = g  or  y <= 0 ? 0 : g
// needs no sum: unlike the training-mode backward of csrc_enc this is ONE pass over the data.  The launch that streams g,
// y (and x) and stores dx (and d_identity) also accumulates dbeta = sum m and dgamma = sum m * xhat, when they are asked
// for.  Everything here is bound by memory traffic: 12 bytes per element in mode 1 without parameter gradients, 16 with.
//
// Work split (csrc_enceval's): the unit of work is a WAVE's task, a task lies inside one (b, c) plane, so the channel is
// wave-uniform -- scale, mean and invstd are formed once per task from scalar loads.  A plane is H*W contiguous floats,
// cut into units of V floats (V = 4, one 16-byte access, when H*W is a multiple of 4 and the pointers are aligned; V = 1
// otherwise) and into chunks of kUnroll * 64 units.  A lane's kUnroll units are 64 units apart, and all loads of a task
// are issued before the first use.  The four waves of a workgroup take four consecutive tasks, which may be four planes
// (layer 4's planes are 208 floats).  A grid of at most kMaxBlocks workgroups strides over the tasks.
//
// Sums: a lane accumulates its units in double, the wave reduces with __shfl_down (every lane of the wave takes part: a
// lane past the plane's end contributes zeros), and lane 0 stores the pair into the TASK's slot of the workspace --
// indexed by the task, not by the workgroup, so a slot's content does not depend on the grid.  finish_kernel then gives
// a wave to each channel: lane l adds the channel's slots l, l + 64, ... in that order, the wave reduces as above, and
// lane 0 stores fp32.  Every slot that is read was stored by the first launch: no zero-fill, no atomics, a fixed order.
#include <hip/hip_runtime.h>

#include "scsfm_fbn.h"

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kUnroll = 2;        // units in flight per lane and stream (three streams with parameter gradients)
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

// this wave's index in the workgroup, as a scalar
__device__ inline int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// the wave's sum, valid in lane 0; the same tree for every call
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d, kWave);
  return v;
}

// tasks = planes * chunks (at most the number of elements, below 2^31: t + stride cannot wrap); a plane has `per` units
// of V floats.  PARAMS: x is read and the task's (sum m * xhat, sum m) goes to ws[2t], ws[2t + 1].
template <int V, int MODE, bool PARAMS>
__global__ __launch_bounds__(kThreads) void bn_bwd_kernel(unsigned tasks, int C, int HW, int per, int chunks, float eps,
                                                           const float* __restrict__ g, const float* __restrict__ x,
                                                           const float* __restrict__ y,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ running_mean,
                                                           const float* __restrict__ running_var,
                                                           float* __restrict__ dx, float* __restrict__ d_identity,
                                                           double* __restrict__ ws) {
  const int lane = threadIdx.x & (kWave - 1);
  const unsigned stride = gridDim.x * kWaves;
  for (unsigned t = blockIdx.x * kWaves + wave_index(); t < tasks; t += stride) {
    const int plane = (int)(t / (unsigned)chunks), chunk = (int)(t - (unsigned)plane * (unsigned)chunks);
    const int c = plane % C;
    const float invstd = 1.0f / sqrtf(running_var[c] + eps);
    const float scale = gamma[c] * invstd;
    float mean = 0.f;
    if (PARAMS) mean = running_mean[c];
    const size_t base = (size_t)plane * HW;
    const int u0 = chunk * (kUnroll * kWave) + lane;
    Pack<V> pg[kUnroll], py[kUnroll], px[kUnroll];
    size_t off[kUnroll];
    // (a unit past the plane's end is loaded from the plane's last unit and never looked at)
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      off[j] = base + (size_t)imin(u0 + j * kWave, per - 1) * V;
      pg[j] = load<V>(g + off[j]);
      if (MODE != 0) py[j] = load<V>(y + off[j]);
      if (PARAMS) px[j] = load<V>(x + off[j]);
    }
    double sum_g = 0.0, sum_b = 0.0;
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      if (u0 + j * kWave < per) {
        Pack<V> m, o;
#pragma unroll
        for (int k = 0; k < V; ++k) {
          m.v[k] = (MODE != 0 && py[j].v[k] <= 0.f) ? 0.f : pg[j].v[k];
          o.v[k] = m.v[k] * scale;
          if (PARAMS) {
            const float xhat = (px[j].v[k] - mean) * invstd;
            sum_g += (double)m.v[k] * (double)xhat;
            sum_b += (double)m.v[k];
          }
        }
        store(dx + off[j], o);
        if (MODE == 2) store(d_identity + off[j], m);
      }
    }
    if (PARAMS) {
      sum_g = wave_sum(sum_g);
      sum_b = wave_sum(sum_b);
      if (lane == 0) {
        ws[2 * (size_t)t] = sum_g;
        ws[2 * (size_t)t + 1] = sum_b;
      }
    }
  }
}

// one wave per channel: the channel's slots are those of its B planes, `chunks` to a plane, numbered b * chunks + k
__global__ __launch_bounds__(kThreads) void finish_kernel(int B, int C, int chunks, const double* __restrict__ ws,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int lane = threadIdx.x & (kWave - 1);
  const int c = blockIdx.x * kWaves + wave_index();
  if (c >= C) return;
  const int n = B * chunks;
  double sum_g = 0.0, sum_b = 0.0;
  for (int i = lane; i < n; i += kWave) {
    const int b = i / chunks, k = i - b * chunks;
    const size_t t = ((size_t)b * C + c) * chunks + k;
    sum_g += ws[2 * t];
    sum_b += ws[2 * t + 1];
  }
  sum_g = wave_sum(sum_g);
  sum_b = wave_sum(sum_b);
  if (lane == 0) {
    dgamma[c] = (float)sum_g;
    dbeta[c] = (float)sum_b;
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

// the scalar path has the most tasks: the workspace is sized for it, whatever the pointers' alignment turns out to be
inline size_t workspace_bytes(int B, int C, int H, int W) {
  return (size_t)B * C * (size_t)ceil_div((long long)H * W, kUnroll * kWave) * 2 * sizeof(double);
}

}  // namespace

#define SCSFM_FBN_LAUNCH(V, MODE, PARAMS)                                                                           \
  hipLaunchKernelGGL((bn_bwd_kernel<V, MODE, PARAMS>), grid, block, 0, (hipStream_t)stream, (unsigned)tasks, C, HW, \
                     per, chunks, (float)eps, g, x, y, gamma, running_mean, running_var, dx, d_identity, (double*)ws)
#define SCSFM_FBN_BY_MODE(V, PARAMS)                      \
  do {                                                    \
    if (mode == 0) SCSFM_FBN_LAUNCH(V, 0, PARAMS);        \
    else if (mode == 1) SCSFM_FBN_LAUNCH(V, 1, PARAMS);   \
    else SCSFM_FBN_LAUNCH(V, 2, PARAMS);                  \
  } while (0)

extern "C" {

int scsfm_fbn_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_fbn_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

size_t scsfm_fbn_workspace_bytes(int B, int C, int H, int W) {
  return shape_ok(B, C, H, W) ? workspace_bytes(B, C, H, W) : 0;
}

int scsfm_fbn_bn_bwd_f32(int B, int C, int H, int W, int mode, double eps, const float* g, const float* x, const float* y,
                         const float* gamma, const float* running_mean, const float* running_var, float* dx,
                         float* d_identity, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
  if (!shape_ok(B, C, H, W) || mode < 0 || mode > 2 || !eps_ok(eps) || !g || (mode != 0 && !y) || !gamma ||
      !running_var || !dx || (mode == 2 && !d_identity))
    return -1;
  const bool params = dgamma != nullptr;
  if ((dbeta != nullptr) != params) return -1;
  if (params && (!x || !running_mean || !ws || ((size_t)ws & 7) != 0 || ws_bytes < workspace_bytes(B, C, H, W)))
    return -1;
  (void)hipGetLastError();
  const int HW = H * W;
  const bool vec = HW % 4 == 0 && aligned16(g) && aligned16(dx) && (mode == 0 || aligned16(y)) &&
                   (mode != 2 || aligned16(d_identity)) && (!params || aligned16(x));
  const int per = vec ? HW / 4 : HW;
  const int chunks = (int)ceil_div(per, kUnroll * kWave);
  const long long tasks = (long long)B * C * chunks;
  const dim3 grid(blocks_for(tasks)), block(kThreads);
  if (params) {
    if (vec) SCSFM_FBN_BY_MODE(4, true);
    else SCSFM_FBN_BY_MODE(1, true);
    const int status = launch_status();
    if (status != 0) return status;
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)ceil_div(C, kWaves)), block, 0, (hipStream_t)stream, B, C, chunks,
                       (const double*)ws, dgamma, dbeta);
  } else {
    if (vec) SCSFM_FBN_BY_MODE(4, false);
    else SCSFM_FBN_BY_MODE(1, false);
  }
  return launch_status();
}

}  // extern "C"
