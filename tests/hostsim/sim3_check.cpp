// A stand-alone check of the 7-DoF tracking library's host-simulator build under the host's sanitizers: no Python, no GPU.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off
//       -Wno-unknown-pragmas -I tests/hostsim -I include -o sim3_check tests/hostsim/sim3_check.cpp
//       -x c++ sc-sfmlearner-release_amd/csrc_cast/scsfm_cast.hip
//       sc-sfmlearner-release_amd/csrc_sim3/scsfm_sim3.hip                 (one command line)
//   ./sim3_check
//
// tests/hostsim/track_check.cpp's scene: a sphere in the corner of three walls (40 x 18 x 29 voxels) is cast by the
// ray-cast library from three reference poses (the model maps) and from three true poses (the frames' depths), at 12 x 20
// and at 37 x 61 pixels (three workgroups of 1024 pixels, the last one partial).  The frames' depths are divided by 1.05
// and by 0.93 and tracked from guesses off by a voxel and a degree, at a scale of 1; the second frame's guess looks away
// (no pair: status 1) and, in a second run, its model maps are all NaN, its reference record carries 1e30 and the third
// frame starts from a scale of NaN (status 2).  Then the scaled depth is formed at pointers on and off a 16-byte boundary.
// Every buffer is a heap allocation of exactly its size, so a read or write past one is the sanitizer's finding.  Exit
// status 0: no finding, the tracked frames end nearer the truth than they began with the scale they were spoiled by, the
// degenerate frames' states keep their bits, and a second run gives the same bits.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "scsfm_cast.h"
#include "scsfm_sim3.h"

namespace {

int fails = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    ++fails;
  }
}

constexpr int NX = 40, NY = 18, NZ = 29;
constexpr float OX = -1.85f, OY = -0.9f, OZ = 0.45f, VOXEL = 0.1f;

std::vector<float> scene() {
  const size_t n = (size_t)NX * NY * NZ;
  std::vector<float> planes(5 * n, 0.0f);
  for (int z = 0; z < NZ; ++z)
    for (int y = 0; y < NY; ++y)
      for (int x = 0; x < NX; ++x) {
        const double px = OX + (x + 0.5) * VOXEL, py = OY + (y + 0.5) * VOXEL, pz = OZ + (z + 0.5) * VOXEL;
        double d = std::sqrt((px - 0.15) * (px - 0.15) + (py - 0.02) * (py - 0.02) + (pz - 1.9) * (pz - 1.9)) - 0.5;
        d = std::fmin(d, (-0.15 * px - pz) / std::sqrt(1.0225) + 2.9);
        d = std::fmin(d, (-py - 0.1 * pz) / std::sqrt(1.01) + 0.75);
        d = std::fmin(d, (-px - 0.1 * py) / std::sqrt(1.01) + 1.2);
        const size_t i = ((size_t)z * NY + y) * NX + x;
        planes[i] = (float)std::fmax(-1.0, std::fmin(1.0, d / 0.3));
        planes[n + i] = 1.0f;
      }
  return planes;
}

// camera to world, 12 doubles: yaw about y, then pitch about x
void pose(double* p, double yaw, double pitch, double x, double y, double z) {
  const double cy = std::cos(yaw), sy = std::sin(yaw), cp = std::cos(pitch), sp = std::sin(pitch);
  const double R[9] = {cy, sy * sp, sy * cp, 0, cp, -sp, -sy, cy * sp, cy * cp};
  const double t[3] = {x, y, z};
  for (int i = 0; i < 3; ++i) p[4 * i] = R[3 * i], p[4 * i + 1] = R[3 * i + 1], p[4 * i + 2] = R[3 * i + 2], p[4 * i + 3] = t[i];
}

struct Maps {
  std::vector<float> view, depth, normal;
};

Maps cast(const std::vector<float>& planes, const std::vector<double>& c2w, const float* K, int H, int W) {
  const int V = (int)c2w.size() / 12;
  Maps m;
  m.view.assign((size_t)V * 16, -1.0f);
  m.depth.assign((size_t)V * H * W, -1.0f);
  m.normal.assign((size_t)V * 3 * H * W, -1.0f);
  expect(scsfm_cast_views(V, c2w.data(), K, m.view.data(), nullptr) == 0, "scsfm_cast_views");
  expect(scsfm_cast_cast(NX, NY, NZ, OX, OY, OZ, VOXEL, planes.data(), 1.0f, 0.0f, VOXEL, 40, V, H, W, m.view.data(),
                         nullptr, m.depth.data(), m.normal.data(), nullptr, nullptr, nullptr) == 0, "scsfm_cast_cast");
  return m;
}

struct Result {
  std::vector<double> state, c2w, scale, report;
  std::vector<float> est, sigma_f;
  bool operator==(const Result& o) const {
    return !std::memcmp(state.data(), o.state.data(), state.size() * 8) &&
           !std::memcmp(c2w.data(), o.c2w.data(), c2w.size() * 8) &&
           !std::memcmp(scale.data(), o.scale.data(), scale.size() * 8) &&
           !std::memcmp(report.data(), o.report.data(), report.size() * 8) &&
           !std::memcmp(est.data(), o.est.data(), est.size() * 4) &&
           !std::memcmp(sigma_f.data(), o.sigma_f.data(), sigma_f.size() * 4);
  }
};

Result track(const std::vector<float>& depth, const std::vector<double>& guess, const std::vector<double>& scale0,
             const float* K, const Maps& model, int H, int W, int iters, std::vector<double>* state0) {
  const int V = (int)guess.size() / 12;
  Result r;
  r.state.assign((size_t)V * 8, -1.0);
  r.est.assign((size_t)V * 16, -1.0f);
  r.sigma_f.assign((size_t)V, -1.0f);
  r.c2w.assign((size_t)V * 12, -1.0);
  r.scale.assign((size_t)V, -1.0);
  r.report.assign((size_t)V * iters * 6, -1.0);
  const size_t nb = scsfm_sim3_ws_bytes(V, H, W);
  expect(nb == (size_t)V * ((H * W + 1023) / 1024) * 37 * 8, "scsfm_sim3_ws_bytes");
  std::vector<double> ws(nb / 8, -1.0);
  expect(scsfm_sim3_init(V, guess.data(), scale0.data(), K, r.state.data(), r.est.data(), r.sigma_f.data(), nullptr) == 0,
         "scsfm_sim3_init");
  if (state0) *state0 = r.state;
  expect(scsfm_sim3_iterate(V, H, W, depth.data(), 0, 0.05f, 4.0f, model.view.data(), model.depth.data(),
                            model.normal.data(), 0.3f, 24, 2e-3, iters, r.state.data(), r.est.data(), r.sigma_f.data(),
                            ws.data(), r.report.data(), nullptr) == 0, "scsfm_sim3_iterate");
  expect(scsfm_sim3_poses(V, r.state.data(), r.c2w.data(), r.scale.data(), nullptr) == 0, "scsfm_sim3_poses");
  return r;
}

double centre_error(const double* a, const double* b) {
  double s = 0;
  for (int i = 0; i < 3; ++i) s += (a[4 * i + 3] - b[4 * i + 3]) * (a[4 * i + 3] - b[4 * i + 3]);
  return std::sqrt(s);
}

void run(const char* name, const std::vector<float>& planes, int H, int W, float f, float cx, float cy, bool spoil) {
  const float K[9] = {f, 0, cx, 0, f, cy, 0, 0, 1};
  const int iters = 6;
  std::vector<double> truth(36), ref(36), guess(36), scale0(3, 1.0);
  const float factor[3] = {1.05f, 1.0f, 0.93f};
  pose(&truth[0], 0.35, -0.20, -0.30, -0.10, 0.50), pose(&truth[12], 0.30, -0.15, -0.20, -0.05, 0.45);
  pose(&truth[24], 0.42, -0.22, -0.35, -0.12, 0.55);
  pose(&ref[0], 0.33, -0.18, -0.25, -0.08, 0.48), pose(&ref[12], 0.36, -0.19, -0.28, -0.10, 0.52);
  pose(&ref[24], 0.38, -0.20, -0.30, -0.08, 0.50);
  pose(&guess[0], 0.362, -0.212, -0.24, -0.15, 0.56), pose(&guess[12], 0.30 + 3.14159265358979, 0.0, -0.20, -0.05, 0.45);
  pose(&guess[24], 0.43, -0.206, -0.28, -0.08, 0.50);
  Maps frames = cast(planes, truth, K, H, W);
  const size_t hw = (size_t)H * W;
  for (int v = 0; v < 3; ++v)
    for (size_t i = 0; i < hw; ++i) frames.depth[v * hw + i] /= factor[v];
  Maps model = cast(planes, ref, K, H, W);
  if (spoil) {
    for (size_t i = 0; i < hw; ++i) model.depth[hw + i] = std::numeric_limits<float>::quiet_NaN();
    for (size_t i = 0; i < 3 * hw; ++i) model.normal[3 * hw + i] = std::numeric_limits<float>::quiet_NaN();
    model.view[16 + 9] = 1e30f;
    pose(&guess[12], 0.31, -0.16, -0.22, -0.04, 0.47);   // (looks at the scene: the pairs fail on the maps)
    scale0[2] = std::numeric_limits<double>::quiet_NaN();
  }
  std::vector<double> state0;
  const Result a = track(frames.depth, guess, scale0, K, model, H, W, iters, &state0);
  const Result b = track(frames.depth, guess, scale0, K, model, H, W, iters, nullptr);
  expect(a == b, "a second run gave other bits");
  std::printf("%-16s", name);
  for (int v = 0; v < 3; ++v) {
    const double* rep = &a.report[(size_t)v * iters * 6];
    const double* last = rep + 6 * (iters - 1);
    const double before = centre_error(&guess[12 * v], &truth[12 * v]), after = centre_error(&a.c2w[12 * v], &truth[12 * v]);
    std::printf("  frame %d: pairs %g -> %g, status %g -> %g, centre error %.4f -> %.4f, scale %.5f;", v, rep[0], last[0],
                rep[2], last[2], before, after, a.scale[v]);
    if (v == 1 || (spoil && v == 2)) {
      const double status = v == 1 ? 1.0 : 2.0;
      expect(rep[2] == status && last[2] == status && rep[0] == 0.0, "a degenerate frame found pairs or another status");
      expect(!std::memcmp(&a.state[8 * v], &state0[8 * v], 64), "a degenerate frame's state changed");
    } else {
      expect(rep[2] == 0.0 && last[2] == 0.0 && rep[0] >= 0.5 * H * W, "a tracked frame has too few pairs or did not solve");
      expect(after < 0.25 * before, "a tracked frame did not end nearer the truth");
      expect(std::fabs(a.scale[v] - factor[v]) < 0.005, "a tracked frame did not find its scale");
      expect(a.sigma_f[v] == (float)a.scale[v] && rep[5] == 1.0 && last[4] > 0.01, "the fp32 scale or the report");
    }
  }
  std::printf("\n");
  // the scaled depth, on and off a 16-byte boundary, against the product
  for (int off = 0; off < 3; ++off) {
    std::vector<float> src(3 * hw + 4, 0.0f), out(3 * hw + 4, -7.0f);
    std::memcpy(src.data() + off, frames.depth.data(), 3 * hw * 4);
    expect(scsfm_sim3_scale(3, H, W, src.data() + off, 0, a.sigma_f.data(), out.data() + off, nullptr) == 0,
           "scsfm_sim3_scale");
    bool same = true;
    for (size_t i = 0; i < 3 * hw; ++i) {
      const float want = a.sigma_f[i / hw] * frames.depth[i];
      same = same && !std::memcmp(&want, &out[off + i], 4);
    }
    for (int i = 0; i < off; ++i) same = same && out[i] == -7.0f;
    for (size_t i = off + 3 * hw; i < out.size(); ++i) same = same && out[i] == -7.0f;
    expect(same, "the scaled depth is not the product, or was written outside its range");
  }
}

}  // namespace

int main() {
  const std::vector<float> planes = scene();
  run("12 x 20", planes, 12, 20, 12.0f, 9.5f, 5.5f, false);
  run("37 x 61", planes, 37, 61, 37.0f, 29.5f, 17.5f, false);
  run("37 x 61 spoiled", planes, 37, 61, 37.0f, 29.5f, 17.5f, true);
  // rejected arguments touch no pointer
  expect(scsfm_sim3_ws_bytes(0, 12, 20) == 0 && scsfm_sim3_ws_bytes(1, 65536, 65536) == 0, "ws_bytes of bad sizes");
  expect(scsfm_sim3_init(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -1, "init with V = 0");
  expect(scsfm_sim3_iterate(3, 12, 20, nullptr, 0, 0.0f, 4.0f, nullptr, nullptr, nullptr, 0.3f, 24, 2e-3, 4, nullptr,
                            nullptr, nullptr, nullptr, nullptr, nullptr) == -1, "iterate with NULL pointers");
  expect(scsfm_sim3_scale(3, 12, 20, nullptr, 0, nullptr, nullptr, nullptr) == -1, "scale with NULL pointers");
  std::printf(fails ? "sim3_check: %d FAILED\n" : "sim3_check: ok\n", fails);
  return fails ? 1 : 0;
}
