// The depth consistency of a frame with its neighbours as a per-pixel confidence, and the TSDF integration weighed by it
// (include/scsfm_conf.h).
//
//  pairs_kernel      one lane per (frame, slot): the neighbour's general inverse and its product with the frame's pose in
//                    double, rounded once.
//  weights_kernel    one launch for all frames; a workgroup (256 threads) takes 1024 pixels of one frame, four per thread.
//                    Where W is a multiple of 4 and the buffers are 16-byte aligned a thread's four pixels are consecutive
//                    in x (one 16-byte load and store); otherwise a thread takes four pixels 256 apart, so that 64
//                    consecutive lanes read 64 consecutive floats.  The frame's 2 radius pair records sit in LDS and are
//                    read as broadcasts; a pixel's depth is read once and its weight written once.  The 8 radius taps are
//                    gathers into the neighbouring frames: neighbouring pixels hit neighbouring texels, and a frame
//                    (0.85 MB at 256 x 832) stays in L2.
//  integrate_kernel  csrc_fuse's integration restated (this library includes nothing of it: source ids and dependencies
//                    are per library), with one more gather per accepted observation, the pixel's weight: 32 x 8 x 4
//                    tiles, four voxels per thread, up to kMaxFrames frames per launch applied in registers, the tile's
//                    conservative frustum cull by wave 0, the 16-byte path where nx is a multiple of 4.
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

#include "scsfm_conf.h"

namespace {  // (internal linkage: the library exports exactly the header's symbols)

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kTX = 32, kTY = 8, kTZ = 4;  // a tile of voxels: kTZ waves, each one z-slice of kTX x kTY
constexpr int kPer = 4;                    // voxels (pixels) per thread
constexpr int kMaxFrames = 32;             // frames per launch of the integration (one bit each in the tile's mask)
constexpr int kRec = SCSFM_CONF_REC;
constexpr int kMaxSlots = 2 * SCSFM_CONF_MAX_RADIUS;
static_assert(kTX * kTY * kTZ == kThreads * kPer, "a tile is kPer voxels per thread");
static_assert(kTX * kTY / kPer == kWave && kTZ == kWaves, "a wave is one z-slice of the tile");
static_assert(kMaxFrames <= kWave, "one lane of wave 0 per frame");
static_assert(kMaxSlots * kRec <= kThreads, "one lane per float of the frame's records");

// ---- pairs ----

__global__ __launch_bounds__(kThreads) void pairs_kernel(int n, int radius, const double* __restrict__ c2w,
                                                         const float* __restrict__ K, float* __restrict__ pair) {
  const int k = (int)(blockIdx.x * kThreads + threadIdx.x);
  const int slots = 2 * radius;
  if (k >= n * slots) return;
  const int i = k / slots, s = k % slots;
  const int j = i + (s < radius ? s - radius : s - radius + 1);
  float* o = pair + kRec * (size_t)k;
  if (j < 0 || j >= n) {
#pragma unroll
    for (int e = 0; e < kRec; ++e) o[e] = 0.0f;
    return;
  }
  const double* p = c2w + 12 * (size_t)j;
  const double* q = c2w + 12 * (size_t)i;
  double a[9], t[3], b[9], u[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    a[3 * r] = p[4 * r], a[3 * r + 1] = p[4 * r + 1], a[3 * r + 2] = p[4 * r + 2], t[r] = p[4 * r + 3];
    b[3 * r] = q[4 * r], b[3 * r + 1] = q[4 * r + 1], b[3 * r + 2] = q[4 * r + 2], u[r] = q[4 * r + 3];
  }
  // the general inverse of the neighbour's pose: adjugate / determinant, -(A^-1 t)
  const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
  const double det = (a[0] * c0 + a[1] * c1) + a[2] * c2;
  double z[9], zt[3];
  z[0] = c0 / det;
  z[3] = c1 / det;
  z[6] = c2 / det;
  z[1] = (a[2] * a[7] - a[1] * a[8]) / det;
  z[4] = (a[0] * a[8] - a[2] * a[6]) / det;
  z[7] = (a[1] * a[6] - a[0] * a[7]) / det;
  z[2] = (a[1] * a[5] - a[2] * a[4]) / det;
  z[5] = (a[2] * a[3] - a[0] * a[5]) / det;
  z[8] = (a[0] * a[4] - a[1] * a[3]) / det;
#pragma unroll
  for (int r = 0; r < 3; ++r) zt[r] = -((z[3 * r] * t[0] + z[3 * r + 1] * t[1]) + z[3 * r + 2] * t[2]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o[3 * r + c] = (float)((z[3 * r] * b[c] + z[3 * r + 1] * b[3 + c]) + z[3 * r + 2] * b[6 + c]);
    o[9 + r] = (float)(((z[3 * r] * u[0] + z[3 * r + 1] * u[1]) + z[3 * r + 2] * u[2]) + zt[r]);
  }
  o[12] = K[0], o[13] = K[4], o[14] = K[2], o[15] = K[5];
}

// ---- weights ----

struct Frames {
  int n, radius, H, W, is_disp, min_views, reduce;
  float max_depth, floor;
};

// one neighbour into one pixel's sums: the header's steps 2a to 2h
__device__ inline void compare(const float* c, const float* __restrict__ nb, float fpx, float fpy, float d, const Frames& u,
                               int& count, float& sum, float& best) {
  float X = fpx - c[14], Y = fpy - c[15];
  X = X / c[12];
  Y = Y / c[13];
  X = X * d;
  Y = Y * d;
  float qx = c[0] * X, qy = c[3] * X, qz = c[6] * X;
  float m;
  m = c[1] * Y; qx = qx + m;
  m = c[4] * Y; qy = qy + m;
  m = c[7] * Y; qz = qz + m;
  m = c[2] * d; qx = qx + m;
  m = c[5] * d; qy = qy + m;
  m = c[8] * d; qz = qz + m;
  qx = qx + c[9];
  qy = qy + c[10];
  qz = qz + c[11];
  if (!(qz > 0.0f)) return;
  float pu = c[12] * qx, pv = c[13] * qy;
  pu = pu / qz;
  pv = pv / qz;
  pu = pu + c[14];
  pv = pv + c[15];
  const float g = floorf(pu), h = floorf(pv);
  if (!(g >= 0.0f && g < (float)u.W && h >= 0.0f && h < (float)u.H)) return;
  const int x0 = (int)g, y0 = (int)h;
  if (x0 > u.W - 2 || y0 > u.H - 2) return;
  const float* row = nb + y0 * u.W + x0;
  float d00 = row[0], d01 = row[1], d10 = row[u.W], d11 = row[u.W + 1];
  if (u.is_disp) {
    d00 = 1.0f / d00;
    d01 = 1.0f / d01;
    d10 = 1.0f / d10;
    d11 = 1.0f / d11;
  }
  if (!(d00 > 0.0f && d01 > 0.0f && d10 > 0.0f && d11 > 0.0f)) return;
  const float a = pu - g, b = pv - h;
  float top = d01 - d00, bot = d11 - d10;
  top = a * top;
  bot = a * bot;
  top = d00 + top;
  bot = d10 + bot;
  float p = bot - top;
  p = b * p;
  p = top + p;
  float num = fabsf(qz - p), den = qz + p;
  num = num / den;
  m = 1.0f - num;
  count += 1;
  sum = sum + m;
  best = m > best ? m : best;
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void weights_kernel(Frames u, int per_frame, const float* __restrict__ depth,
                                                           const float* __restrict__ pair, float* __restrict__ weight) {
  __shared__ float s_pair[kMaxSlots * kRec];
  const int tid = (int)threadIdx.x;
  const int frame = (int)blockIdx.x / per_frame, chunk = (int)blockIdx.x % per_frame;
  const int slots = 2 * u.radius;
  if (tid < slots * kRec) s_pair[tid] = pair[(size_t)frame * slots * kRec + tid];
  __syncthreads();
  const int hw = u.H * u.W;
  const float* __restrict__ mine = depth + (size_t)frame * hw;
  float* __restrict__ out = weight + (size_t)frame * hw;
  int at[kPer];
  bool in[kPer];
  float D[kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    at[k] = kVec ? chunk * (kThreads * kPer) + kPer * tid + k : chunk * (kThreads * kPer) + tid + kThreads * k;
    in[k] = at[k] < hw;
    D[k] = 0.0f;
  }
  if (kVec) {
    if (!in[0]) return;  // (hw is a multiple of 4: the four are inside together)
    const float4 d4 = *reinterpret_cast<const float4*>(mine + at[0]);
    D[0] = d4.x, D[1] = d4.y, D[2] = d4.z, D[3] = d4.w;
  } else {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      if (in[k]) D[k] = mine[at[k]];
    }
  }
  float C[kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    C[k] = 0.0f;
    if (!(kVec || in[k])) continue;
    float d = D[k];
    if (u.is_disp) d = 1.0f / d;
    if (!(d > 0.0f && d <= u.max_depth)) continue;
    const int py = at[k] / u.W, px = at[k] - py * u.W;
    const float fpx = (float)px, fpy = (float)py;
    int count = 0;
    float sum = 0.0f, best = 0.0f;
    for (int s = 0; s < slots; ++s) {
      const float* c = s_pair + s * kRec;
      if (!(c[12] > 0.0f)) continue;  // (an absent neighbour; the same in every lane)
      const int j = frame + (s < u.radius ? s - u.radius : s - u.radius + 1);
      if (j < 0 || j >= u.n) continue;  // (a record that claims a frame there is none of is never followed)
      compare(c, depth + (size_t)j * hw, fpx, fpy, d, u, count, sum, best);
    }
    float c = 0.0f;
    if (count >= u.min_views) c = u.reduce == SCSFM_CONF_MEAN ? sum / (float)count : best;
    C[k] = c >= u.floor ? c : 0.0f;
  }
  if (kVec) {
    *reinterpret_cast<float4*>(out + at[0]) = make_float4(C[0], C[1], C[2], C[3]);
  } else {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      if (in[k]) out[at[k]] = C[k];
    }
  }
}

// ---- integration ----

__device__ inline float centre(float o, int i, float s) {
  float c = (float)i + 0.5f;
  c = c * s;
  return o + c;
}

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
                               const float* __restrict__ depth, const float* __restrict__ weight,
                               const float* __restrict__ image, float& t, float& w, float& r, float& g, float& b) {
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
  const float cw = weight[pix];  // (asked for together with the depth, ahead of the depth's test: the two gathers overlap)
  if (u.is_disp) d = 1.0f / d;
  if (!(d > 0.0f && d <= u.max_depth)) return;
  if (!(cw > 0.0f && cw <= 1.0f)) return;
  const float sdf = d - qz;
  if (sdf < -u.trunc) return;
  float tn = fminf(1.0f, sdf / u.trunc);
  tn = tn * cw;
  const float w1 = w + cw;
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
    cr = cr * cw;
    cg = cg * cw;
    cb = cb * cw;
    r = r * w; r = r + cr; r = r / w1;
    g = g * w; g = g + cg; g = g / w1;
    b = b * w; b = b + cb; b = b / w1;
  }
  w = fminf(w1, u.max_weight);
}

template <bool kVec, bool kColour>
__global__ __launch_bounds__(kThreads) void integrate_kernel(Grid v, Fusion u, int f0, const float* __restrict__ cam,
                                                             const float* __restrict__ depth,
                                                             const float* __restrict__ weight,
                                                             const float* __restrict__ image, float* __restrict__ volume) {
  __shared__ float s_cam[kMaxFrames * kRec];
  __shared__ unsigned s_mask;
  const int tid = (int)threadIdx.x;
  const int tiles_x = (v.nx + kTX - 1) / kTX, tiles_y = (v.ny + kTY - 1) / kTY;
  const int tile = (int)blockIdx.x;
  const int x0 = (tile % tiles_x) * kTX, y0 = ((tile / tiles_x) % tiles_y) * kTY, z0 = (tile / (tiles_x * tiles_y)) * kTZ;
  if (tid < kWave) {
    bool meets = false;
    if (tid < u.F) {
      float c[kRec];
#pragma unroll
      for (int i = 0; i < kRec; ++i) {
        c[i] = cam[(size_t)(f0 + tid) * kRec + i];
        s_cam[tid * kRec + i] = c[i];
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
    const float* c = s_cam + f * kRec;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (kVec || in[j])
        observe<kColour>(c, f0 + f, X[j], Y[j], Z, u, depth, weight, image, T[j], Wt[j], R[j], G[j], B[j]);
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

// ---- host side ----

// nvox, or 0 for sizes the library rejects
inline long long voxels(int nx, int ny, int nz) {
  if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
  const long long slice = (long long)nx * ny;  // (stepwise: the product of three ints can pass 2^63)
  if (slice > SCSFM_CONF_MAX_VOXELS || slice * nz > SCSFM_CONF_MAX_VOXELS) return 0;
  return slice * nz;
}

inline bool positive(float x) { return x > 0.0f && std::isfinite(x); }  // (false for a NaN)

inline bool aligned(const void* p, uintptr_t to) { return p && ((uintptr_t)p & (to - 1)) == 0; }  // (false for NULL)

}  // namespace

extern "C" {

int scsfm_conf_abi_version(void) { return 1; }

#ifndef SCSFM_SOURCE_ID
#define SCSFM_SOURCE_ID "unknown"
#endif
// (behind the marker that scsfm_hip/build.py reads from the FILE, as in csrc/scsfm_warp.hip)
static const char g_source_tag[] __attribute__((used)) = "scsfm-source-id:" SCSFM_SOURCE_ID;
int scsfm_conf_source_id(char* buf, size_t n) {
  const volatile char* id = g_source_tag + 16;
  if (!buf || n == 0) return -1;
  size_t i = 0;
  for (; i + 1 < n && id[i]; ++i) buf[i] = id[i];
  buf[i] = 0;
  return 0;
}

int scsfm_conf_pairs(int n, int radius, const double* c2w, const float* K, float* pair, void* stream) {
  if (n <= 0 || radius < 1 || radius > SCSFM_CONF_MAX_RADIUS || n > INT_MAX / (2 * radius * kRec) || !aligned(c2w, 8) ||
      !aligned(K, 4) || !aligned(pair, 4))
    return SCSFM_CONF_ERR_ARG;
  const int lanes = n * 2 * radius;
  (void)hipGetLastError();
  hipLaunchKernelGGL(pairs_kernel, dim3((unsigned)((lanes + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, n, radius, c2w, K, pair);
  return (int)hipGetLastError();
}

int scsfm_conf_weights(int n, int radius, int H, int W, const float* depth, int is_disp, const float* pair,
                       float max_depth, int min_views, float floor, int reduce, float* weight, void* stream) {
  if (n <= 0 || H <= 0 || W <= 0 || radius < 1 || radius > SCSFM_CONF_MAX_RADIUS || min_views < 1 ||
      (reduce != SCSFM_CONF_MEAN && reduce != SCSFM_CONF_MAX) || !aligned(depth, 4) || !aligned(pair, 4) ||
      !aligned(weight, 4))
    return SCSFM_CONF_ERR_ARG;
  if ((long long)H * W > INT_MAX || (long long)n * H * W > INT_MAX || n > INT_MAX / (2 * radius * kRec))
    return SCSFM_CONF_ERR_ARG;
  if (!positive(max_depth) || !(floor >= 0.0f && floor <= 1.0f)) return SCSFM_CONF_ERR_ARG;
  const Frames u = {n, radius, H, W, is_disp != 0, min_views, reduce, max_depth, floor};
  const int per_frame = (int)(((long long)H * W + kThreads * kPer - 1) / (kThreads * kPer));
  const dim3 grid((unsigned)((long long)n * per_frame)), block(kThreads);  // (<= n H W)
  const bool vec = W % 4 == 0 && aligned(depth, 16) && aligned(weight, 16);
  (void)hipGetLastError();
  if (vec)
    hipLaunchKernelGGL((weights_kernel<true>), grid, block, 0, (hipStream_t)stream, u, per_frame, depth, pair, weight);
  else
    hipLaunchKernelGGL((weights_kernel<false>), grid, block, 0, (hipStream_t)stream, u, per_frame, depth, pair, weight);
  return (int)hipGetLastError();
}

int scsfm_conf_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, float trunc, float near_z,
                         float max_depth, float max_weight, int F, int H, int W, const float* cam, const float* depth,
                         const float* weight, int is_disp, const float* image, float* volume, void* stream) {
  const long long nvox = voxels(nx, ny, nz);
  if (!nvox || F <= 0 || H <= 0 || W <= 0 || !aligned(cam, 4) || !aligned(depth, 4) || !aligned(weight, 4) ||
      !aligned(volume, 4) || ((uintptr_t)image & 3) != 0)
    return SCSFM_CONF_ERR_ARG;
  if ((long long)H * W > INT_MAX || (long long)F * 3 * H * W > INT_MAX) return SCSFM_CONF_ERR_ARG;
  if (!std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(oz) || !positive(voxel) || !positive(trunc) ||
      !(near_z >= 0.0f) || !std::isfinite(near_z) || !positive(max_depth) || !(max_weight >= 1.0f) ||
      !std::isfinite(max_weight))
    return SCSFM_CONF_ERR_ARG;
  const Grid v = {nx, ny, nz, ox, oy, oz, voxel};
  const int tiles = ((nx + kTX - 1) / kTX) * ((ny + kTY - 1) / kTY) * ((nz + kTZ - 1) / kTZ);  // (<= nvox)
  const bool vec = nx % 4 == 0 && ((uintptr_t)volume & 15) == 0;
  (void)hipGetLastError();
  for (int f0 = 0; f0 < F; f0 += kMaxFrames) {
    const Fusion u = {trunc, near_z, max_depth, max_weight, F - f0 < kMaxFrames ? F - f0 : kMaxFrames, H, W, is_disp != 0};
    const dim3 grid((unsigned)tiles), block(kThreads);
    if (vec && image)
      hipLaunchKernelGGL((integrate_kernel<true, true>), grid, block, 0, (hipStream_t)stream, v, u, f0, cam, depth, weight,
                         image, volume);
    else if (vec)
      hipLaunchKernelGGL((integrate_kernel<true, false>), grid, block, 0, (hipStream_t)stream, v, u, f0, cam, depth,
                         weight, image, volume);
    else if (image)
      hipLaunchKernelGGL((integrate_kernel<false, true>), grid, block, 0, (hipStream_t)stream, v, u, f0, cam, depth,
                         weight, image, volume);
    else
      hipLaunchKernelGGL((integrate_kernel<false, false>), grid, block, 0, (hipStream_t)stream, v, u, f0, cam, depth,
                         weight, image, volume);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  return 0;
}

}  // extern "C"
