// TSDF fusion of predicted depth and poses, and the extraction of surface points (include/scsfm_fuse.h).
//
//  cameras_kernel    one lane per frame: the general inverse of the camera-to-world pose in double, rounded once.
//  integrate_kernel  one workgroup (256 threads) per tile of 32 x 8 x 4 voxels, four voxels per thread.  The volume is
//                    20 bytes per voxel and every frame touches a large part of it, so the kernel is bound by memory
//                    traffic: it carries up to kMaxFrames frames per launch and applies them in registers, reading and
//                    writing a voxel once.  Wave 0 first tests the tile's bounding sphere against every frame (one lane
//                    per frame) and leaves a mask of the frames that can meet it; the loop over the frames branches on
//                    that mask, which is the same in every lane, and a tile that meets no frame returns before its
//                    loads.  The camera records of the launch sit in LDS and are read as broadcasts.
//                    Where nx is a multiple of 4 and the volume is 16-byte aligned a thread's four voxels are consecutive
//                    in x (one 16-byte load and store per plane, eight lanes to a 128-byte row segment); otherwise a
//                    thread takes one x and four rows, so that 32 consecutive lanes read 32 consecutive floats.
//                    The depth (and image) fetches are gathers at the projected pixel: neighbouring voxels project to
//                    neighbouring pixels, and a frame (0.85 MB at 256 x 832) stays in L2.
//  count_kernel /    one workgroup per chunk of 1024 consecutive voxels, one voxel per lane in four steps of 256; the
//  extract_kernel    crossings of the three edges are three ballots, a lane's place is the number of set bits below it,
//                    the waves' totals meet in LDS, and the chunk's base comes from scan_kernel's exclusive scan.
//  scan_kernel       one workgroup: the exclusive scan of the chunks' counts and the total.
//
// Arithmetic: the header's order, one rounding per operation.  The pragma keeps the compiler from contracting a multiply
// and an add into one fused operation (hipcc's default is -ffp-contract=fast); `/` is the correctly rounded expansion
// and fp32 denormals are kept on gfx950.  Only the cull's own arithmetic is free: it decides what may be skipped, with
// margins, never a value.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "scsfm_fuse.h"

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kTX = 32, kTY = 8, kTZ = 4;  // a tile of voxels: kTZ waves, each one z-slice of kTX x kTY
constexpr int kPer = 4;                    // voxels per thread
constexpr int kMaxFrames = 32;             // frames per launch (one bit each in the tile's mask)
constexpr int kCam = SCSFM_FUSE_CAM;
constexpr int kChunk = SCSFM_FUSE_CHUNK;
constexpr int kSteps = kChunk / kThreads;
constexpr int kScanPer = 8;                // counts per thread and step of the scan
constexpr int kWsHead = 4;                 // ints in front of the counts
static_assert(kTX * kTY * kTZ == kThreads * kPer, "a tile is kPer voxels per thread");
static_assert(kTX * kTY / kPer == kWave && kTZ == kWaves, "a wave is one z-slice of the tile");
static_assert(kMaxFrames <= kWave, "one lane of wave 0 per frame");

__device__ inline float centre(float o, int i, float s) {
  float c = (float)i + 0.5f;
  c = c * s;
  return o + c;
}

// ---- cameras ----

__global__ __launch_bounds__(kThreads) void cameras_kernel(int n, const double* __restrict__ c2w,
                                                           const float* __restrict__ K, float* __restrict__ cam) {
  const int f = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (f >= n) return;
  const double* p = c2w + 12 * (size_t)f;
  double a[9], t[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    a[3 * i] = p[4 * i], a[3 * i + 1] = p[4 * i + 1], a[3 * i + 2] = p[4 * i + 2], t[i] = p[4 * i + 3];
  }
  // the general inverse, as csrc_odom/scsfm_odom.hip's inverse(): adjugate / determinant, -(A^-1 t)
  const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
  const double det = (a[0] * c0 + a[1] * c1) + a[2] * c2;
  double z[9];
  z[0] = c0 / det;
  z[3] = c1 / det;
  z[6] = c2 / det;
  z[1] = (a[2] * a[7] - a[1] * a[8]) / det;
  z[4] = (a[0] * a[8] - a[2] * a[6]) / det;
  z[7] = (a[1] * a[6] - a[0] * a[7]) / det;
  z[2] = (a[1] * a[5] - a[2] * a[4]) / det;
  z[5] = (a[2] * a[3] - a[0] * a[5]) / det;
  z[8] = (a[0] * a[4] - a[1] * a[3]) / det;
  float* o = cam + kCam * (size_t)f;
#pragma unroll
  for (int i = 0; i < 9; ++i) o[i] = (float)z[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) o[9 + i] = (float)(-((z[3 * i] * t[0] + z[3 * i + 1] * t[1]) + z[3 * i + 2] * t[2]));
  o[12] = K[0], o[13] = K[4], o[14] = K[2], o[15] = K[5];
}

// ---- integration ----

struct Grid {
  int nx, ny, nz;
  float ox, oy, oz, voxel;
};

struct Fusion {
  float trunc, near_z, max_depth, max_weight;
  int F, H, W, is_disp;
};

// Can frame `c` meet a sphere of centre (x, y, z) and radius r (world)?  Conservative: false only when no point of the
// sphere passes the header's tests 1 to 5.  A voxel that contributes has near < q_z <= max_depth + trunc and a pixel
// inside the picture, that is, lies in four half-spaces through the camera centre; the picture is taken one pixel wider
// on every side, which covers the roundings of u and v.  The sphere's image under the affine map (A, t) lies in the
// sphere of radius r |A|_2 round the centre's image, and |A|_2^2 <= 1 + |A^T A - I|_F (1 + 1e-7 for a rotation).  `tol`
// covers the roundings of the centre's and of a voxel's q: each is a few ulp of |A||c| + |t| <= |q| + 2 |t|.
// Every comparison is written so that a NaN keeps the frame.
__device__ inline bool frame_meets(const float* c, float x, float y, float z, float r, const Fusion& u) {
  const float qx = c[0] * x + c[1] * y + c[2] * z + c[9];
  const float qy = c[3] * x + c[4] * y + c[5] * z + c[10];
  const float qz = c[6] * x + c[7] * y + c[8] * z + c[11];
  float e = 0.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float g = c[i] * c[j] + c[3 + i] * c[3 + j] + c[6 + i] * c[6 + j] - (i == j ? 1.0f : 0.0f);
      e += g * g;
    }
  }
  const float tol = 1e-5f * (fabsf(qx) + fabsf(qy) + fabsf(qz) + 2.0f * (fabsf(c[9]) + fabsf(c[10]) + fabsf(c[11])));
  const float re = r * sqrtf(1.0f + sqrtf(e)) * 1.001f + tol;
  bool out = (qz + re < u.near_z) || (qz - re > u.max_depth + u.trunc);
  const float fx = c[12], fy = c[13], cx = c[14], cy = c[15];
  if (fx > 0.0f) {
    const float al = -(cx + 1.5f) / fx, ar = ((float)u.W + 0.5f - cx) / fx;  // q_x >= al q_z and q_x <= ar q_z
    out = out || ((qx - al * qz) < -re * sqrtf(1.0f + al * al)) || ((ar * qz - qx) < -re * sqrtf(1.0f + ar * ar));
  }
  if (fy > 0.0f) {
    const float at = -(cy + 1.5f) / fy, ab = ((float)u.H + 0.5f - cy) / fy;
    out = out || ((qy - at * qz) < -re * sqrtf(1.0f + at * at)) || ((ab * qz - qy) < -re * sqrtf(1.0f + ab * ab));
  }
  return !out;
}

// one frame into one voxel: the header's steps 1 to 9
template <bool kColour>
__device__ inline void observe(const float* c, int f, float x, float y, float z, const Fusion& u,
                               const float* __restrict__ depth, const float* __restrict__ image, float& t, float& w,
                               float& r, float& g, float& b) {
  float qx = c[0] * x, qy = c[3] * x, qz = c[6] * x;
  float m;
  m = c[1] * y; qx = qx + m;
  m = c[4] * y; qy = qy + m;
  m = c[7] * y; qz = qz + m;
  m = c[2] * z; qx = qx + m;
  m = c[5] * z; qy = qy + m;
  m = c[8] * z; qz = qz + m;
  qx = qx + c[9];
  qy = qy + c[10];
  qz = qz + c[11];
  if (!(qz > u.near_z)) return;
  float pu = c[12] * qx, pv = c[13] * qy;
  pu = pu / qz;
  pv = pv / qz;
  pu = pu + c[14];
  pv = pv + c[15];
  const float a = pu + 0.5f, bb = pv + 0.5f;
  if (!(a >= 0.0f && a < (float)u.W && bb >= 0.0f && bb < (float)u.H)) return;
  const int px = (int)a, py = (int)bb;
  const int pix = (f * u.H + py) * u.W + px;
  float d = depth[pix];
  if (u.is_disp) d = 1.0f / d;
  if (!(d > 0.0f && d <= u.max_depth)) return;
  const float sdf = d - qz;
  if (sdf < -u.trunc) return;
  const float tn = fminf(1.0f, sdf / u.trunc);
  const float w1 = w + 1.0f;
  t = t * w;
  t = t + tn;
  t = t / w1;
  if (kColour) {
    const int hw = u.H * u.W;
    const int p0 = (3 * f * u.H + py) * u.W + px;
    float cr = image[p0] * 0.225f, cg = image[p0 + hw] * 0.225f, cb = image[p0 + 2 * hw] * 0.225f;
    cr = cr + 0.45f;
    cg = cg + 0.45f;
    cb = cb + 0.45f;
    r = r * w; r = r + cr; r = r / w1;
    g = g * w; g = g + cg; g = g / w1;
    b = b * w; b = b + cb; b = b / w1;
  }
  w = fminf(w1, u.max_weight);
}

template <bool kVec, bool kColour>
__global__ __launch_bounds__(kThreads) void integrate_kernel(Grid v, Fusion u, int f0, const float* __restrict__ cam,
                                                             const float* __restrict__ depth,
                                                             const float* __restrict__ image, float* __restrict__ volume) {
  __shared__ float s_cam[kMaxFrames * kCam];
  __shared__ unsigned s_mask;
  const int tid = (int)threadIdx.x;
  const int tiles_x = (v.nx + kTX - 1) / kTX, tiles_y = (v.ny + kTY - 1) / kTY;
  const int tile = (int)blockIdx.x;
  const int x0 = (tile % tiles_x) * kTX, y0 = ((tile / tiles_x) % tiles_y) * kTY, z0 = (tile / (tiles_x * tiles_y)) * kTZ;
  if (tid < kWave) {
    bool meets = false;
    if (tid < u.F) {
      float c[kCam];
#pragma unroll
      for (int i = 0; i < kCam; ++i) {
        c[i] = cam[(size_t)(f0 + tid) * kCam + i];
        s_cam[tid * kCam + i] = c[i];
      }
      // the centres of a whole tile's voxels span (kTX - 1, kTY - 1, kTZ - 1) voxels round its middle
      const float mx = v.ox + ((float)x0 + 0.5f * kTX) * v.voxel, my = v.oy + ((float)y0 + 0.5f * kTY) * v.voxel;
      const float mz = v.oz + ((float)z0 + 0.5f * kTZ) * v.voxel;
      const float half = 0.5f * sqrtf((float)((kTX - 1) * (kTX - 1) + (kTY - 1) * (kTY - 1) + (kTZ - 1) * (kTZ - 1)));
      meets = frame_meets(c, mx, my, mz, half * v.voxel * 1.001f, u);
    }
    const unsigned long long ballot = __ballot(meets);
    if (tid == 0) s_mask = (unsigned)ballot;
  }
  __syncthreads();
  const unsigned mask = (unsigned)__builtin_amdgcn_readfirstlane((int)s_mask);
  if (mask == 0u) return;

  // the thread's four voxels: consecutive in x (kVec), or one x and four rows
  const int lz = tid >> 6;
  const int vz = z0 + lz;
  int vx[kPer], vy[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    vx[j] = kVec ? x0 + 4 * (tid & 7) + j : x0 + (tid & 31);
    vy[j] = kVec ? y0 + ((tid >> 3) & 7) : y0 + ((tid >> 5) & 1) + 2 * j;
  }
  if (vz >= v.nz) return;
  const size_t nvox = (size_t)v.nx * v.ny * v.nz;
  bool in[kPer];
  size_t at[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    in[j] = vx[j] < v.nx && vy[j] < v.ny;
    at[j] = ((size_t)vz * v.ny + vy[j]) * v.nx + vx[j];
  }
  float T[kPer], Wt[kPer], R[kPer], G[kPer], B[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) T[j] = Wt[j] = R[j] = G[j] = B[j] = 0.0f;
  if (kVec) {
    if (!in[0]) return;  // (nx is a multiple of 4: the four are inside together)
    const float4 t4 = *reinterpret_cast<const float4*>(volume + at[0]);
    const float4 w4 = *reinterpret_cast<const float4*>(volume + nvox + at[0]);
    T[0] = t4.x, T[1] = t4.y, T[2] = t4.z, T[3] = t4.w;
    Wt[0] = w4.x, Wt[1] = w4.y, Wt[2] = w4.z, Wt[3] = w4.w;
    if (kColour) {
      const float4 r4 = *reinterpret_cast<const float4*>(volume + 2 * nvox + at[0]);
      const float4 g4 = *reinterpret_cast<const float4*>(volume + 3 * nvox + at[0]);
      const float4 b4 = *reinterpret_cast<const float4*>(volume + 4 * nvox + at[0]);
      R[0] = r4.x, R[1] = r4.y, R[2] = r4.z, R[3] = r4.w;
      G[0] = g4.x, G[1] = g4.y, G[2] = g4.z, G[3] = g4.w;
      B[0] = b4.x, B[1] = b4.y, B[2] = b4.z, B[3] = b4.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (in[j]) {
        T[j] = volume[at[j]];
        Wt[j] = volume[nvox + at[j]];
      }
      if (kColour && in[j]) {
        R[j] = volume[2 * nvox + at[j]];
        G[j] = volume[3 * nvox + at[j]];
        B[j] = volume[4 * nvox + at[j]];
      }
    }
  }
  float X[kPer], Y[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    X[j] = centre(v.ox, vx[j], v.voxel);
    Y[j] = centre(v.oy, vy[j], v.voxel);
  }
  const float Z = centre(v.oz, vz, v.voxel);
  for (int f = 0; f < u.F; ++f) {
    if (!((mask >> f) & 1u)) continue;  // (the same in every lane)
    const float* c = s_cam + f * kCam;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (kVec || in[j]) observe<kColour>(c, f0 + f, X[j], Y[j], Z, u, depth, image, T[j], Wt[j], R[j], G[j], B[j]);
    }
  }
  if (kVec) {
    *reinterpret_cast<float4*>(volume + at[0]) = make_float4(T[0], T[1], T[2], T[3]);
    *reinterpret_cast<float4*>(volume + nvox + at[0]) = make_float4(Wt[0], Wt[1], Wt[2], Wt[3]);
    if (kColour) {
      *reinterpret_cast<float4*>(volume + 2 * nvox + at[0]) = make_float4(R[0], R[1], R[2], R[3]);
      *reinterpret_cast<float4*>(volume + 3 * nvox + at[0]) = make_float4(G[0], G[1], G[2], G[3]);
      *reinterpret_cast<float4*>(volume + 4 * nvox + at[0]) = make_float4(B[0], B[1], B[2], B[3]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (in[j]) {
        volume[at[j]] = T[j];
        volume[nvox + at[j]] = Wt[j];
      }
      if (kColour && in[j]) {
        volume[2 * nvox + at[j]] = R[j];
        volume[3 * nvox + at[j]] = G[j];
        volume[4 * nvox + at[j]] = B[j];
      }
    }
  }
}

// ---- extraction ----

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

template <bool kWrite>
__global__ __launch_bounds__(kThreads) void extract_kernel(Grid v, const float* __restrict__ volume, float min_weight,
                                                           int* __restrict__ counts, const int* __restrict__ offsets,
                                                           int capacity, float* __restrict__ xyz,
                                                           unsigned char* __restrict__ rgb) {
  __shared__ int s_wave[kWaves];
  const int tid = (int)threadIdx.x;
  const int nvox = v.nx * v.ny * v.nz;
  const int chunk = (int)blockIdx.x;
  const float* __restrict__ tsdf = volume;
  const float* __restrict__ weight = volume + (size_t)nvox;
  int running = kWrite ? offsets[chunk] : 0;
  for (int step = 0; step < kSteps; ++step) {
    const int i = chunk * kChunk + step * kThreads + tid;
    bool e[3] = {false, false, false};
    int nb[3] = {0, 0, 0};
    int x = 0, y = 0, z = 0;
    float ta = 0.0f;
    if (i < nvox) {
      x = i % v.nx;
      const int row = i / v.nx;
      y = row % v.ny;
      z = row / v.ny;
      ta = tsdf[i];
      const bool seen = weight[i] >= min_weight;
      nb[0] = i + 1, nb[1] = i + v.nx, nb[2] = i + v.nx * v.ny;
      const bool has[3] = {x + 1 < v.nx, y + 1 < v.ny, z + 1 < v.nz};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (seen && has[k]) e[k] = weight[nb[k]] >= min_weight && ((ta < 0.0f) != (tsdf[nb[k]] < 0.0f));
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
  if (slice > SCSFM_FUSE_MAX_VOXELS || slice * nz > SCSFM_FUSE_MAX_VOXELS) return 0;
  return slice * nz;
}

inline bool positive(float x) { return x > 0.0f && std::isfinite(x); }  // (false for a NaN)

inline int chunks(long long nvox) { return (int)((nvox + kChunk - 1) / kChunk); }

}  // namespace

extern "C" {

int scsfm_fuse_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_fuse_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

size_t scsfm_fuse_volume_bytes(int nx, int ny, int nz) {
  return (size_t)voxels(nx, ny, nz) * SCSFM_FUSE_PLANES * sizeof(float);
}

size_t scsfm_fuse_extract_ws_bytes(int nx, int ny, int nz) {
  const long long nvox = voxels(nx, ny, nz);
  if (!nvox) return 0;
  return sizeof(int) * (size_t)(kWsHead + 2 * chunks(nvox));
}

int scsfm_fuse_cameras(int n, const double* c2w, const float* K, float* cam, void* stream) {
  if (n <= 0 || n > INT_MAX / kCam || !c2w || !K || !cam) return SCSFM_FUSE_ERR_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(cameras_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, n, c2w, K, cam);
  return (int)hipGetLastError();
}

int scsfm_fuse_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, float trunc, float near_z,
                         float max_depth, float max_weight, int F, int H, int W, const float* cam, const float* depth,
                         int is_disp, const float* image, float* volume, void* stream) {
  const long long nvox = voxels(nx, ny, nz);
  if (!nvox || F <= 0 || H <= 0 || W <= 0 || !cam || !depth || !volume || ((uintptr_t)volume & 3) != 0)
    return SCSFM_FUSE_ERR_ARG;
  if ((long long)H * W > INT_MAX || (long long)F * 3 * H * W > INT_MAX) return SCSFM_FUSE_ERR_ARG;
  if (!std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(oz) || !positive(voxel) || !positive(trunc) ||
      !(near_z >= 0.0f) || !std::isfinite(near_z) || !positive(max_depth) || !(max_weight >= 1.0f) ||
      !std::isfinite(max_weight))
    return SCSFM_FUSE_ERR_ARG;
  const Grid v = {nx, ny, nz, ox, oy, oz, voxel};
  const int tiles = ((nx + kTX - 1) / kTX) * ((ny + kTY - 1) / kTY) * ((nz + kTZ - 1) / kTZ);  // (<= nvox)
  const bool vec = nx % 4 == 0 && ((uintptr_t)volume & 15) == 0;
  (void)hipGetLastError();
  for (int f0 = 0; f0 < F; f0 += kMaxFrames) {
    const Fusion u = {trunc, near_z, max_depth, max_weight, F - f0 < kMaxFrames ? F - f0 : kMaxFrames, H, W, is_disp != 0};
    const dim3 grid((unsigned)tiles), block(kThreads);
    if (vec && image)
      hipLaunchKernelGGL((integrate_kernel<true, true>), grid, block, 0, (hipStream_t)stream, v, u, f0, cam, depth, image,
                         volume);
    else if (vec)
      hipLaunchKernelGGL((integrate_kernel<true, false>), grid, block, 0, (hipStream_t)stream, v, u, f0, cam, depth,
                         image, volume);
    else if (image)
      hipLaunchKernelGGL((integrate_kernel<false, true>), grid, block, 0, (hipStream_t)stream, v, u, f0, cam, depth,
                         image, volume);
    else
      hipLaunchKernelGGL((integrate_kernel<false, false>), grid, block, 0, (hipStream_t)stream, v, u, f0, cam, depth,
                         image, volume);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  return 0;
}

int scsfm_fuse_count(int nx, int ny, int nz, const float* volume, float min_weight, void* ws, size_t ws_bytes,
                     void* stream) {
  const long long nvox = voxels(nx, ny, nz);
  if (!nvox || !volume || !ws || ((uintptr_t)ws & 15) != 0 || !(min_weight >= 1.0f) || !std::isfinite(min_weight) ||
      ws_bytes < scsfm_fuse_extract_ws_bytes(nx, ny, nz))
    return SCSFM_FUSE_ERR_ARG;
  const Grid v = {nx, ny, nz, 0.0f, 0.0f, 0.0f, 1.0f};
  const int n = chunks(nvox);
  int* head = (int*)ws;
  (void)hipGetLastError();
  hipLaunchKernelGGL((extract_kernel<false>), dim3((unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, v, volume,
                     min_weight, head + kWsHead, (const int*)nullptr, 0, (float*)nullptr, (unsigned char*)nullptr);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, n, head + kWsHead,
                     head + kWsHead + n, head);
  return (int)hipGetLastError();
}

int scsfm_fuse_extract(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, const float* volume,
                       float min_weight, const void* ws, size_t ws_bytes, int capacity, float* xyz, unsigned char* rgb,
                       void* stream) {
  const long long nvox = voxels(nx, ny, nz);
  if (!nvox || !volume || !ws || ((uintptr_t)ws & 15) != 0 || !(min_weight >= 1.0f) || !std::isfinite(min_weight) ||
      ws_bytes < scsfm_fuse_extract_ws_bytes(nx, ny, nz) || capacity < 0 || (capacity > 0 && (!xyz || !rgb)) ||
      !std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(oz) || !positive(voxel))
    return SCSFM_FUSE_ERR_ARG;
  if (capacity == 0) return 0;
  const Grid v = {nx, ny, nz, ox, oy, oz, voxel};
  const int n = chunks(nvox);
  const int* head = (const int*)ws;
  (void)hipGetLastError();
  hipLaunchKernelGGL((extract_kernel<true>), dim3((unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, v, volume,
                     min_weight, (int*)nullptr, head + kWsHead + n, capacity, xyz, rgb);
  return (int)hipGetLastError();
}

}  // extern "C"
