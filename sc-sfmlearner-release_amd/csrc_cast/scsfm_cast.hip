// Ray casting of the fused TSDF volume (include/scsfm_cast.h).
//
//  views_kernel  one lane per view: the pose's twelve doubles rounded once, and the intrinsics.
//  mask_kernel   one workgroup per run of 31 bricks along x in one (By, Bz): lane t takes the voxel column x = 248 c + t
//                (249 columns: the bricks' nine-wide ranges overlap by one) and walks the up to 9 x 9 rows of the
//                bricks' range in y and z, so a wave reads consecutive floats of the tsdf and weight planes; the
//                columns' flags meet in LDS and 31 lanes write the bricks' bytes.  A streaming pass: a voxel is read
//                (9 / 8)^2 times.
//  cast_kernel   one thread per pixel, one workgroup (256 threads) per 16 x 16 pixel tile of one view, a wave an 8 x 8
//                block of it: neighbouring rays walk neighbouring voxels and share cache lines.  The view record is the
//                same for the whole workgroup and is read through uniform (scalar) loads.  The march carries only the
//                previous sample's T and validity; the gradient and the colours are formed at the hit alone, from the
//                corners of the two samples of the event, whose coordinates are the same arithmetic again.
//
// The cull (kCull).  A sample whose base voxel lies in an unmarked brick cannot be inside: it is either invalid, or all
// eight of its corners are valid (weight >= min_weight) with t >= 0 -- the mask's nine-wide range covers the corners of
// every cell whose base is in the brick -- and a lerp fl(t0 + fl(f fl(t1 - t0))) of non-negative values with 0 <= f < 1
// is non-negative in fp32.  With t1 >= t0 every term is >= 0.  With t1 < t0: t1 - t0 >= -t0, and -t0 is representable, so
// d = fl(t1 - t0) >= -t0 because rounding is monotone; d < 0 and 0 <= f < 1 give f d >= d >= -t0, so fl(f d) >= -t0 for the
// same reason; then t0 + fl(f d) >= 0 exactly, and so is its rounding.  T is seven such lerps.  (A corner that is a NaN or
// +infinity is not "< 0" and can only turn T into a NaN or +infinity, never into a negative value; a T that is a NaN is
// not inside.)  An event needs an inside sample at k-1 or at
// k.  So the kernel computes every sample's coordinates (the header's arithmetic, cheap), looks its brick's byte up (64 K
// bricks for 512 x 128 x 512 voxels: they stay in cache) and fetches the eight corners only for a sample whose own
// brick, its predecessor's or its successor's is marked: when sample k is inside, k-1 and k+1 have been evaluated too,
// and a sample that was skipped takes part in no event, as none could involve it.  With mask == NULL every sample is
// evaluated, which is the baseline and the proof that the cull changes no bit.
//
// Arithmetic: the header's order, one rounding per operation.  The pragma keeps the compiler from contracting a multiply
// and an add into one fused operation (hipcc's default is -ffp-contract=fast); `/` and sqrtf are the correctly rounded
// expansions and fp32 denormals are kept on gfx950.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "scsfm_cast.h"

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kThreads = 256;
constexpr int kView = SCSFM_CAST_VIEW;
constexpr int kBrick = SCSFM_CAST_BRICK;
constexpr int kTile = 16;                             // a workgroup's tile of pixels is kTile x kTile
constexpr int kRun = 31;                              // bricks along x per workgroup of the mask kernel
constexpr int kCols = kRun * kBrick + 1;              // voxel columns they cover
static_assert(kTile * kTile == kThreads, "one thread per pixel of the tile");
static_assert(kCols <= kThreads, "one lane per voxel column");

struct Grid {
  int nx, ny, nz;
  float ox, oy, oz, voxel;
};

__device__ inline int bricks(int n) { return (n + kBrick - 1) / kBrick; }

// ---- views ----

__global__ __launch_bounds__(kThreads) void views_kernel(int n, const double* __restrict__ c2w,
                                                         const float* __restrict__ K, float* __restrict__ view) {
  const int f = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (f >= n) return;
  const double* p = c2w + 12 * (size_t)f;
  float* o = view + kView * (size_t)f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    o[3 * i] = (float)p[4 * i], o[3 * i + 1] = (float)p[4 * i + 1], o[3 * i + 2] = (float)p[4 * i + 2];
    o[9 + i] = (float)p[4 * i + 3];
  }
  o[12] = K[0], o[13] = K[4], o[14] = K[2], o[15] = K[5];
}

// ---- the brick mask ----

__global__ __launch_bounds__(kThreads) void mask_kernel(int nx, int ny, int nz, const float* __restrict__ volume,
                                                        float min_weight, unsigned char* __restrict__ mask) {
  __shared__ int s_flag[kThreads];
  const int tid = (int)threadIdx.x;
  const int nbx = bricks(nx), nby = bricks(ny);
  const int runs = (nbx + kRun - 1) / kRun;
  const int run = (int)blockIdx.x % runs, By = ((int)blockIdx.x / runs) % nby, Bz = (int)blockIdx.x / (runs * nby);
  const int x = run * (kRun * kBrick) + tid;
  const int y0 = By * kBrick, z0 = Bz * kBrick;
  const int y1 = y0 + kBrick < ny ? y0 + kBrick : ny - 1, z1 = z0 + kBrick < nz ? z0 + kBrick : nz - 1;  // (inclusive)
  const size_t nvox = (size_t)nx * ny * nz;
  int flag = 0;
  if (tid < kCols && x < nx) {
    for (int z = z0; z <= z1; ++z) {
      for (int y = y0; y <= y1; ++y) {
        const size_t at = ((size_t)z * ny + y) * nx + x;
        const float t = volume[at], w = volume[nvox + at];
        flag |= (w >= min_weight && t < 0.0f) ? 1 : 0;
      }
    }
  }
  s_flag[tid] = flag;
  __syncthreads();
  const int Bx = run * kRun + tid;
  if (tid < kRun && Bx < nbx) {
    int any = 0;
#pragma unroll
    for (int i = 0; i <= kBrick; ++i) any |= s_flag[kBrick * tid + i];
    mask[((size_t)Bz * nby + By) * nbx + Bx] = (unsigned char)any;
  }
}

// ---- the cast ----

struct March {
  float min_weight, near_s, step;
  int n_steps, V, H, W;
};

struct Ray {
  float c[3], w[3];
};

// the cell of a point: in range or not, the base voxel and the three fractions
struct Cell {
  bool in;
  int bx, by, bz;
  float fx, fy, fz;
};

__device__ inline float sample_at(const March& m, int k) {
  float s = (float)k * m.step;
  return m.near_s + s;
}

__device__ inline float coordinate(float c, float w, float s, float o, float voxel) {
  float p = s * w;
  p = c + p;
  p = p - o;
  p = p / voxel;
  return p - 0.5f;
}

__device__ inline Cell locate(const Grid& v, const Ray& r, float s) {
  const float gx = coordinate(r.c[0], r.w[0], s, v.ox, v.voxel);
  const float gy = coordinate(r.c[1], r.w[1], s, v.oy, v.voxel);
  const float gz = coordinate(r.c[2], r.w[2], s, v.oz, v.voxel);
  Cell c;
  // on the floats, before any conversion: a NaN or a huge value fails and converts nothing
  c.in = gx >= 0.0f && gx < (float)(v.nx - 1) && gy >= 0.0f && gy < (float)(v.ny - 1) && gz >= 0.0f &&
         gz < (float)(v.nz - 1);
  c.bx = c.by = c.bz = 0;
  c.fx = c.fy = c.fz = 0.0f;
  if (c.in) {
    c.bx = (int)gx, c.by = (int)gy, c.bz = (int)gz;
    c.fx = gx - (float)c.bx, c.fy = gy - (float)c.by, c.fz = gz - (float)c.bz;
  }
  return c;
}

__device__ inline float lerp(float a, float b, float f) {
  float d = b - a;
  d = f * d;
  return a + d;
}

// the eight corners of a cell of one plane: q[i + 2 j + 4 k] is the voxel (bx + i, by + j, bz + k)
__device__ inline void corners(const Grid& v, const float* __restrict__ plane, const Cell& c, float q[8]) {
  const int row = v.nx, slice = v.nx * v.ny;
  const float* p = plane + ((size_t)c.bz * v.ny + c.by) * v.nx + c.bx;
  q[0] = p[0], q[1] = p[1], q[2] = p[row], q[3] = p[row + 1];
  q[4] = p[slice], q[5] = p[slice + 1], q[6] = p[slice + row], q[7] = p[slice + row + 1];
}

__device__ inline float trilinear(const float q[8], const Cell& c) {
  const float e00 = lerp(q[0], q[1], c.fx), e10 = lerp(q[2], q[3], c.fx);
  const float e01 = lerp(q[4], q[5], c.fx), e11 = lerp(q[6], q[7], c.fx);
  const float e0 = lerp(e00, e10, c.fy), e1 = lerp(e01, e11, c.fy);
  return lerp(e0, e1, c.fz);
}

__device__ inline void gradient(const float q[8], const Cell& c, float g[3]) {
  // G_x: the x-differences, reduced along y then z
  g[0] = lerp(lerp(q[1] - q[0], q[3] - q[2], c.fy), lerp(q[5] - q[4], q[7] - q[6], c.fy), c.fz);
  // G_y: the y-differences, along x then z
  g[1] = lerp(lerp(q[2] - q[0], q[3] - q[1], c.fx), lerp(q[6] - q[4], q[7] - q[5], c.fx), c.fz);
  // G_z: the z-differences, along x then y
  g[2] = lerp(lerp(q[4] - q[0], q[5] - q[1], c.fx), lerp(q[6] - q[2], q[7] - q[3], c.fx), c.fy);
}

__device__ inline bool seen(const Grid& v, const float* __restrict__ weight, const Cell& c, float min_weight) {
  float q[8];
  corners(v, weight, c, q);
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 8; ++i) ok = ok && q[i] >= min_weight;
  return ok;
}

__device__ inline unsigned char unit_byte(float c) {
  c = c >= 0.0f ? c : 0.0f;
  c = c <= 1.0f ? c : 1.0f;
  c = c * 255.0f;
  c = c + 0.5f;
  return (unsigned char)(int)c;
}

__device__ inline float quiet(float x) { return x != x ? __builtin_nanf("") : x; }

template <bool kCull>
__global__ __launch_bounds__(kThreads) void cast_kernel(Grid v, March m, const float* __restrict__ volume,
                                                        const float* __restrict__ view,
                                                        const unsigned char* __restrict__ mask,
                                                        float* __restrict__ depth, float* __restrict__ normal,
                                                        unsigned char* __restrict__ rgb,
                                                        unsigned char* __restrict__ shade) {
  const int tid = (int)threadIdx.x;
  const int tiles_x = (m.W + kTile - 1) / kTile, tiles_y = (m.H + kTile - 1) / kTile;
  const int tile = (int)blockIdx.x % (tiles_x * tiles_y), f = (int)blockIdx.x / (tiles_x * tiles_y);
  // a wave is an 8 x 8 block of the tile
  const int px = (tile % tiles_x) * kTile + 8 * ((tid >> 6) & 1) + (tid & 7);
  const int py = (tile / tiles_x) * kTile + 8 * (tid >> 7) + ((tid >> 3) & 7);
  if (px >= m.W || py >= m.H) return;
  const float* __restrict__ a = view + (size_t)f * kView;  // (the same address in every lane)
  Ray r;
  {
    float dx = (float)px - a[14], dy = (float)py - a[15];
    dx = dx / a[12];
    dy = dy / a[13];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      float p = a[3 * i] * dx;
      const float q = a[3 * i + 1] * dy;
      p = p + q;
      r.w[i] = p + a[3 * i + 2];
      r.c[i] = a[9 + i];
    }
  }
  const size_t nvox = (size_t)v.nx * v.ny * v.nz;
  const float* __restrict__ tsdf = volume;
  const float* __restrict__ weight = volume + nvox;
  const int nbx = bricks(v.nx), nby = bricks(v.ny);

  // the byte of the brick of sample k's base voxel (0 out of range)
  auto marked = [&](int k) -> int {
    if (!kCull) return 1;
    if (k >= m.n_steps) return 0;
    const Cell c = locate(v, r, sample_at(m, k));
    if (!c.in) return 0;
    return (int)mask[((size_t)(c.bz >> 3) * nby + (c.by >> 3)) * nbx + (c.bx >> 3)];
  };

  bool hit = false;
  int at = 0;                       // the event's k
  float t_prev = 0.0f, t_cur = 0.0f;
  bool valid_prev = false;
  int m_prev = 0, m_cur = marked(0);
  for (int k = 0; k < m.n_steps; ++k) {
    const int m_next = marked(k + 1);
    bool valid = false;
    t_cur = 0.0f;
    if (m_prev | m_cur | m_next) {
      const Cell c = locate(v, r, sample_at(m, k));
      if (c.in && seen(v, weight, c, m.min_weight)) {
        float q[8];
        corners(v, tsdf, c, q);
        t_cur = trilinear(q, c);
        valid = true;
      }
    }
    if (valid && valid_prev && ((t_cur < 0.0f) != (t_prev < 0.0f))) {  // (k >= 1: valid_prev starts false)
      hit = t_cur < 0.0f;
      at = k;
      break;
    }
    valid_prev = valid;
    t_prev = t_cur;
    m_prev = m_cur;
    m_cur = m_next;
  }

  const size_t hw = (size_t)m.H * m.W;
  const size_t pix = ((size_t)f * m.H + py) * m.W + px;
  float d = 0.0f, n[3] = {0.0f, 0.0f, 0.0f};
  unsigned char col[3] = {0, 0, 0}, sh = 0;
  if (hit) {
    const float s0 = sample_at(m, at - 1), s1 = sample_at(m, at);
    float frac = t_prev - t_cur;
    frac = t_prev / frac;
    float ds = s1 - s0;
    ds = ds * frac;
    d = quiet(s0 + ds);
    const Cell c0 = locate(v, r, s0), c1 = locate(v, r, s1);
    if (normal || shade) {
      float q[8], g0[3], g1[3];
      corners(v, tsdf, c0, q);
      gradient(q, c0, g0);
      corners(v, tsdf, c1, q);
      gradient(q, c1, g1);
      float N[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) N[i] = lerp(g0[i], g1[i], frac);
      float len = N[0] * N[0];
      float p = N[1] * N[1];
      len = len + p;
      p = N[2] * N[2];
      len = len + p;
      len = sqrtf(len);
      if (len > 0.0f) {
#pragma unroll
        for (int i = 0; i < 3; ++i) n[i] = quiet(N[i] / len);
      }
      if (shade) {
        float dot = n[0] * r.w[0];
        p = n[1] * r.w[1];
        dot = dot + p;
        p = n[2] * r.w[2];
        dot = dot + p;
        float wl = r.w[0] * r.w[0];
        p = r.w[1] * r.w[1];
        wl = wl + p;
        p = r.w[2] * r.w[2];
        wl = wl + p;
        wl = sqrtf(wl);
        sh = unit_byte(-dot / wl);
      }
    }
    if (rgb) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float* __restrict__ plane = volume + (size_t)(2 + ch) * nvox;
        float q[8];
        corners(v, plane, c0, q);
        const float ca = trilinear(q, c0);
        corners(v, plane, c1, q);
        const float cb = trilinear(q, c1);
        col[ch] = unit_byte(lerp(ca, cb, frac));
      }
    }
  }
  depth[pix] = d;
  if (normal) {
    float* o = normal + (size_t)f * 3 * hw + (size_t)py * m.W + px;
    o[0] = n[0], o[hw] = n[1], o[2 * hw] = n[2];
  }
  if (rgb) {
    unsigned char* o = rgb + 3 * pix;
    o[0] = col[0], o[1] = col[1], o[2] = col[2];
  }
  if (shade) shade[pix] = sh;
}

// ---- host side ----

// nvox, or 0 for sizes the library rejects
inline long long voxels(int nx, int ny, int nz) {
  if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
  const long long slice = (long long)nx * ny;  // (stepwise: the product of three ints can pass 2^63)
  if (slice > SCSFM_CAST_MAX_VOXELS || slice * nz > SCSFM_CAST_MAX_VOXELS) return 0;
  return slice * nz;
}

inline bool positive(float x) { return x > 0.0f && std::isfinite(x); }  // (false for a NaN)

inline bool misaligned(const void* p, unsigned to) { return ((uintptr_t)p & (to - 1)) != 0; }

inline int host_bricks(int n) { return (n + kBrick - 1) / kBrick; }

}  // namespace

extern "C" {

int scsfm_cast_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_cast_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

int scsfm_cast_views(int n, const double* c2w, const float* K, float* view, void* stream) {
  if (n <= 0 || n > INT_MAX / kView || !c2w || !K || !view) return SCSFM_CAST_ERR_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(views_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, n, c2w, K, view);
  return (int)hipGetLastError();
}

size_t scsfm_cast_mask_bytes(int nx, int ny, int nz) {
  if (!voxels(nx, ny, nz)) return 0;
  return (size_t)host_bricks(nx) * host_bricks(ny) * host_bricks(nz);
}

int scsfm_cast_mask(int nx, int ny, int nz, const float* volume, float min_weight, unsigned char* mask, void* stream) {
  if (!voxels(nx, ny, nz) || !volume || !mask || misaligned(volume, 4) || !(min_weight >= 1.0f) ||
      !std::isfinite(min_weight))
    return SCSFM_CAST_ERR_ARG;
  const int runs = (host_bricks(nx) + kRun - 1) / kRun;
  const long long groups = (long long)runs * host_bricks(ny) * host_bricks(nz);  // (<= nvox)
  (void)hipGetLastError();
  hipLaunchKernelGGL(mask_kernel, dim3((unsigned)groups), dim3(kThreads), 0, (hipStream_t)stream, nx, ny, nz, volume,
                     min_weight, mask);
  return (int)hipGetLastError();
}

int scsfm_cast_cast(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, const float* volume,
                    float min_weight, float near_s, float step, int n_steps, int V, int H, int W, const float* view,
                    const unsigned char* mask, float* depth, float* normal, unsigned char* rgb, unsigned char* shade,
                    void* stream) {
  if (!voxels(nx, ny, nz) || V <= 0 || H <= 0 || W <= 0 || n_steps < 1 || n_steps > SCSFM_CAST_MAX_STEPS || !volume ||
      !view || !depth || misaligned(volume, 4) || misaligned(view, 4) || misaligned(depth, 4) || misaligned(normal, 4))
    return SCSFM_CAST_ERR_ARG;
  if ((long long)H * W > INT_MAX || (long long)V * 3 * H * W > INT_MAX) return SCSFM_CAST_ERR_ARG;
  if (!std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(oz) || !positive(voxel) || !positive(step) ||
      !(near_s >= 0.0f) || !std::isfinite(near_s) || !(min_weight >= 1.0f) || !std::isfinite(min_weight))
    return SCSFM_CAST_ERR_ARG;
  const Grid v = {nx, ny, nz, ox, oy, oz, voxel};
  const March m = {min_weight, near_s, step, n_steps, V, H, W};
  const long long groups = (long long)((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile) * V;  // (<= V H W)
  const dim3 grid((unsigned)groups), block(kThreads);
  (void)hipGetLastError();
  if (mask)
    hipLaunchKernelGGL((cast_kernel<true>), grid, block, 0, (hipStream_t)stream, v, m, volume, view, mask, depth, normal,
                       rgb, shade);
  else
    hipLaunchKernelGGL((cast_kernel<false>), grid, block, 0, (hipStream_t)stream, v, m, volume, view, mask, depth,
                       normal, rgb, shade);
  return (int)hipGetLastError();
}

}  // extern "C"
