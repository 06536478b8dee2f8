// A stand-alone check of the confidence library's host-simulator build under the host's sanitizers: no Python, no GPU.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off
//       -Wno-unknown-pragmas -I tests/hostsim -I include -include tests/hostsim/fuse_shim.h -o conf_check
//       tests/hostsim/conf_check.cpp -x c++ sc-sfmlearner-release_amd/csrc_conf/scsfm_conf.hip      (one command line)
//   ./conf_check
//
// The smallest cases of tests/_conf_cases.py's kinds: three cameras that step sideways over a sloping surface, at 12 x 20
// pixels (the 16-byte path) and 37 x 61 (the scalar path, three workgroups with the last one partial), radius 1 and, with
// two frames, radius 4; own depths and taps of 0 and NaN; flat frames a whole pixel apart, whose weights must be exactly
// 1 or 0; then the weighted integration of those frames into 37 x 19 x 22 (scalar) and 40 x 16 x 12 (16-byte path) voxels,
// with and without an image, with weights that include 0, -1, NaN and 1.5, as one call of three frames and as three calls
// of one.  Every buffer is a heap allocation of exactly its size, so a read or write past one is the sanitizer's
// finding.  Exit status 0: no finding, every weight in [0, 1], the two ways of integrating leave the same bits, and a
// second run gives the same bits.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "scsfm_conf.h"

namespace {

int fails = 0;
const float kNaN = std::numeric_limits<float>::quiet_NaN();

void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    ++fails;
  }
}

// camera to world, 12 doubles: identity rotation at (x, y, z)
std::vector<double> poses(int n, double step) {
  std::vector<double> p((size_t)n * 12, 0.0);
  for (int k = 0; k < n; ++k) {
    p[12 * k] = p[12 * k + 5] = p[12 * k + 10] = 1.0;
    p[12 * k + 3] = step * k, p[12 * k + 7] = 0.01 * k, p[12 * k + 11] = 0.0;
  }
  return p;
}

// the depth of the plane z = 2 + 0.1 x from a camera at (cx, cy, 0) looking along z
std::vector<float> frames(const std::vector<double>& c2w, int H, int W, float f, float u0, float v0, bool flat) {
  const int n = (int)c2w.size() / 12;
  std::vector<float> d((size_t)n * H * W);
  for (int k = 0; k < n; ++k)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const double rx = (x - u0) / f;
        d[((size_t)k * H + y) * W + x] = flat ? 2.0f : (float)((2.0 + 0.1 * c2w[12 * k + 3]) / (1.0 - 0.1 * rx));
      }
  return d;
}

std::vector<float> weights(const std::vector<double>& c2w, const std::vector<float>& depth, int radius, int H, int W,
                           float f, float u0, float v0, int is_disp, int min_views, float floor, int reduce) {
  const int n = (int)c2w.size() / 12;
  const float K[9] = {f, 0, u0, 0, f, v0, 0, 0, 1};
  std::vector<float> pair((size_t)n * 2 * radius * 16, -1.0f), w((size_t)n * H * W, -1.0f);
  expect(scsfm_conf_pairs(n, radius, c2w.data(), K, pair.data(), nullptr) == 0, "scsfm_conf_pairs");
  for (int i = 0; i < n; ++i)
    for (int s = 0; s < 2 * radius; ++s) {
      const int j = i + (s < radius ? s - radius : s - radius + 1);
      const float* r = &pair[((size_t)i * 2 * radius + s) * 16];
      bool zero = true;
      for (int e = 0; e < 16; ++e) zero = zero && r[e] == 0.0f && !std::signbit(r[e]);
      expect((j < 0 || j >= n) ? zero : (r[12] == f && r[15] == v0 && r[0] == 1.0f), "a pair record");
    }
  std::vector<float> again = w;
  expect(scsfm_conf_weights(n, radius, H, W, depth.data(), is_disp, pair.data(), 4.0f, min_views, floor, reduce, w.data(),
                            nullptr) == 0, "scsfm_conf_weights");
  expect(scsfm_conf_weights(n, radius, H, W, depth.data(), is_disp, pair.data(), 4.0f, min_views, floor, reduce,
                            again.data(), nullptr) == 0, "scsfm_conf_weights again");
  expect(!std::memcmp(w.data(), again.data(), w.size() * 4), "a second run of the weights gave other bits");
  for (float c : w) expect(c >= 0.0f && c <= 1.0f, "a weight outside [0, 1]");
  return w;
}

void run_weights(const char* name, int H, int W, float f, float u0, float v0) {
  const std::vector<double> c3 = poses(3, 0.09), c2 = poses(2, 0.09), c1 = poses(1, 0.0);
  std::vector<float> d3 = frames(c3, H, W, f, u0, v0, false);
  d3[(size_t)1 * H * W + 2 * W + 3] = 0.0f, d3[(size_t)1 * H * W + 2 * W + 4] = kNaN, d3[(size_t)2 * H * W + 5 * W + 7] = 0.0f;
  d3[(size_t)0 * H * W + 8 * W + 12] = kNaN, d3[(size_t)1 * H * W + 3 * W + 3] = 7.5f;
  const std::vector<float> w = weights(c3, d3, 1, H, W, f, u0, v0, 0, 1, 0.0f, SCSFM_CONF_MEAN);
  expect(w[(size_t)1 * H * W + 2 * W + 3] == 0.0f && w[(size_t)1 * H * W + 2 * W + 4] == 0.0f &&
         w[(size_t)1 * H * W + 3 * W + 3] == 0.0f, "a pixel without a depth of its own has a weight");
  int some = 0;
  for (float c : w) some += c > 0.9f;
  expect(some > H * W, "too few pixels agree with their neighbours");
  const std::vector<float> best = weights(c3, d3, 1, H, W, f, u0, v0, 0, 1, 0.0f, SCSFM_CONF_MAX);
  bool above = true;
  for (size_t i = 0; i < w.size(); ++i) above = above && best[i] >= w[i];
  expect(above, "the best neighbour is below the mean");
  const std::vector<float> two = weights(c3, d3, 1, H, W, f, u0, v0, 0, 2, 0.999f, SCSFM_CONF_MEAN);
  bool ends = true;
  for (int i = 0; i < H * W; ++i) ends = ends && two[i] == 0.0f && two[(size_t)2 * H * W + i] == 0.0f;
  expect(ends, "min_views 2: an end frame has a weight");
  std::vector<float> disp = frames(c2, H, W, f, u0, v0, false);
  for (float& v : disp) v = 1.0f / v;
  disp[5] = 0.0f, disp[(size_t)H * W + 9] = kNaN;
  int far = 0;
  for (float c : weights(c2, disp, 4, H, W, f, u0, v0, 1, 1, 0.0f, SCSFM_CONF_MEAN)) far += c > 0.9f;
  expect(far > H * W / 2, "two frames at radius 4");
  for (float c : weights(c1, frames(c1, H, W, f, u0, v0, false), 1, H, W, f, u0, v0, 0, 1, 0.0f, SCSFM_CONF_MEAN))
    expect(c == 0.0f, "one frame alone has a weight");
  // flat frames a whole pixel apart (f is a power of two, the depth is 2): exactly 1 where a neighbour is met
  const std::vector<double> whole = poses(3, 2.0 / f);
  int ones = 0;
  for (float c : weights(whole, frames(whole, H, W, f, u0, v0, true), 1, H, W, f, u0, v0, 0, 1, 0.0f, SCSFM_CONF_MEAN)) {
    expect(c == 0.0f || c == 1.0f, "flat frames a pixel apart: a weight that is neither 0 nor 1");
    ones += c == 1.0f;
  }
  expect(ones > 2 * (H - 2) * (W - 2), "flat frames a pixel apart: too few ones");
  std::printf("%-8s %d of %d pixels above 0.9 at radius 1, %d of %d at radius 4, %d exact ones\n", name, some, 3 * H * W, far,
              2 * H * W, ones);
}

void run_integrate(const char* name, int nx, int ny, int nz, float ox, float oy, float oz, bool colour) {
  const int F = 3, H = 12, W = 20;
  const std::vector<double> c2w = poses(F, 0.09);
  const std::vector<float> depth = frames(c2w, H, W, 16.0f, 9.5f, 5.5f, false);
  std::vector<float> cam((size_t)F * 16, 0.0f), image, w((size_t)F * H * W);
  for (int k = 0; k < F; ++k) {   // world to camera of an identity rotation: (I, -centre)
    float* c = &cam[16 * k];
    c[0] = c[4] = c[8] = 1.0f;
    c[9] = (float)-c2w[12 * k + 3], c[10] = (float)-c2w[12 * k + 7], c[11] = 0.0f;
    c[12] = c[13] = 16.0f, c[14] = 9.5f, c[15] = 5.5f;
  }
  for (size_t i = 0; i < w.size(); ++i) w[i] = 0.05f + 0.95f * (float)((i * 37) % 101) / 101.0f;
  w[3] = 0.0f, w[4] = -1.0f, w[5] = kNaN, w[6] = 1.5f, w[7] = 1.0f;
  if (colour) {
    image.resize((size_t)F * 3 * H * W);
    for (size_t i = 0; i < image.size(); ++i) image[i] = (float)((i * 13) % 29) / 14.0f - 1.0f;
  }
  const size_t nvox = (size_t)nx * ny * nz;
  std::vector<float> a(5 * nvox, 0.0f), b(5 * nvox, 0.0f), c(5 * nvox, 0.0f);
  const float* img = colour ? image.data() : nullptr;
  for (std::vector<float>* v : {&a, &c})
    expect(scsfm_conf_integrate(nx, ny, nz, ox, oy, oz, 0.1f, 0.3f, 0.05f, 4.0f, 2.5f, F, H, W, cam.data(), depth.data(),
                                w.data(), 0, img, v->data(), nullptr) == 0, "scsfm_conf_integrate");
  for (int k = 0; k < F; ++k)
    expect(scsfm_conf_integrate(nx, ny, nz, ox, oy, oz, 0.1f, 0.3f, 0.05f, 4.0f, 2.5f, 1, H, W, &cam[16 * k],
                                &depth[(size_t)k * H * W], &w[(size_t)k * H * W], 0, colour ? &image[(size_t)k * 3 * H * W] : nullptr,
                                b.data(), nullptr) == 0, "scsfm_conf_integrate, one frame");
  expect(!std::memcmp(a.data(), b.data(), a.size() * 4), "three frames in one call and three calls of one differ");
  expect(!std::memcmp(a.data(), c.data(), a.size() * 4), "a second run of the integration gave other bits");
  size_t seen = 0, capped = 0;
  bool sane = true;
  for (size_t i = 0; i < nvox; ++i) {
    const float wt = a[nvox + i];
    seen += wt > 0.0f, capped += wt == 2.5f;
    sane = sane && wt >= 0.0f && wt <= 2.5f && a[i] >= -1.0f && a[i] <= 1.0f;
    if (!colour) sane = sane && a[2 * nvox + i] == 0.0f && a[3 * nvox + i] == 0.0f && a[4 * nvox + i] == 0.0f;
  }
  expect(sane && seen > nvox / 20, "the integrated volume");
  std::printf("%-22s %zu of %zu voxels seen, %zu at the weight's cap\n", name, seen, nvox, capped);
}

}  // namespace

int main() {
  run_weights("12 x 20", 12, 20, 16.0f, 9.5f, 5.5f);
  run_weights("37 x 61", 37, 61, 32.0f, 29.5f, 17.5f);
  run_integrate("37 x 19 x 22", 37, 19, 22, -1.85f, -0.9f, 0.45f, false);
  run_integrate("37 x 19 x 22, colour", 37, 19, 22, -1.85f, -0.9f, 0.45f, true);
  run_integrate("40 x 16 x 12", 40, 16, 12, -2.0f, -0.8f, 1.45f, false);
  run_integrate("40 x 16 x 12, colour", 40, 16, 12, -2.0f, -0.8f, 1.45f, true);
  // rejected arguments touch no pointer
  expect(scsfm_conf_pairs(0, 1, nullptr, nullptr, nullptr, nullptr) == -1, "pairs with n = 0");
  expect(scsfm_conf_pairs(3, 5, nullptr, nullptr, nullptr, nullptr) == -1, "pairs with radius 5");
  expect(scsfm_conf_weights(3, 1, 12, 20, nullptr, 0, nullptr, 4.0f, 1, 0.0f, 0, nullptr, nullptr) == -1,
         "weights with NULL pointers");
  expect(scsfm_conf_weights(3, 1, 12, 20, nullptr, 0, nullptr, 4.0f, 1, kNaN, 0, nullptr, nullptr) == -1, "weights with a NaN floor");
  expect(scsfm_conf_integrate(37, 19, 22, 0, 0, 0, 0.1f, 0.3f, 0.0f, 4.0f, 64.0f, 3, 12, 20, nullptr, nullptr, nullptr, 0,
                              nullptr, nullptr, nullptr) == -1, "integrate with NULL pointers");
  std::printf(fails ? "conf_check: %d FAILED\n" : "conf_check: ok\n", fails);
  return fails ? 1 : 0;
}
