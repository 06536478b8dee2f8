// A stand-alone check of the rolling library's host-simulator build under the host's sanitizers: no Python, no GPU.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off
//       -Wno-unknown-pragmas -I tests/hostsim -I include -include tests/hostsim/fuse_shim.h -o roll_check
//       tests/hostsim/roll_check.cpp -x c++ sc-sfmlearner-release_amd/csrc_roll/scsfm_roll.hip      (one command line)
//   ./roll_check
//
// The kinds of tests/_roll_cases.py at their smallest.  The shift: a 37 x 18 x 29 volume (no size a multiple of 4, a plane
// of 19314 floats) of distinct bit patterns moved by every shift of the list -- each axis alone, two diagonal ones, n - 1,
// n and beyond -- with dst at all four alignments to 16 bytes, and 4 x 1 x 1, 1 x 1 x 1 and 40 x 6 x 5 volumes; every
// element of dst is compared with a loop over the voxels.  The leaving extraction: a volume whose tsdf changes sign along
// a slanted plane, with the keep boxes of four shifts, an empty box, the whole volume (xyz and rgb NULL), a box one voxel
// thick and one whose faces cut a chunk; the points are compared with a loop over the edges, in order, at capacity ==
// total and at a smaller one.  Every buffer is a heap allocation of exactly its size, so a read or write past one is the
// sanitizer's finding.  Exit status 0: no finding and every comparison held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scsfm_roll.h"

namespace {

int fails = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    ++fails;
  }
}

std::vector<uint32_t> patterns(size_t n) {
  std::vector<uint32_t> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = (uint32_t)(i * 2654435761ull + 12345ull);
  if (n > 8) v[0] = 0x7FC00001u, v[1] = 0x00000001u, v[2] = 0xFF800000u, v[n - 1] = 0x807FFFFFu;  // NaN, denormals, -inf
  return v;
}

void run_shift(int nx, int ny, int nz, int sx, int sy, int sz) {
  const size_t nvox = (size_t)nx * ny * nz, total = 5 * nvox;
  const std::vector<uint32_t> src = patterns(total);
  std::vector<uint32_t> want(total, 0u);
  for (int p = 0; p < 5; ++p)
    for (int z = 0; z < nz; ++z)
      for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
          const long long ax = (long long)x + sx, ay = (long long)y + sy, az = (long long)z + sz;
          if (ax >= 0 && ax < nx && ay >= 0 && ay < ny && az >= 0 && az < nz)
            want[p * nvox + ((size_t)z * ny + y) * nx + x] = src[p * nvox + ((size_t)az * ny + ay) * nx + ax];
        }
  for (int lead = 0; lead < 4; ++lead) {
    // (dst starts `lead` floats into the allocation and ends at its end: all four alignments, whatever the allocator's)
    std::vector<uint32_t> buf(total + lead, 0x7FC00000u);
    const std::vector<uint32_t> before = src;
    expect(scsfm_roll_shift(nx, ny, nz, sx, sy, sz, (const float*)src.data(), (float*)(buf.data() + lead), nullptr) == 0,
           "scsfm_roll_shift");
    expect(!std::memcmp(buf.data() + lead, want.data(), total * 4), "the shifted planes differ");
    for (int j = 0; j < lead; ++j) expect(buf[j] == 0x7FC00000u, "the shift wrote in front of dst");
    expect(before == src, "the shift changed its source");
  }
}

struct Points {
  std::vector<float> xyz;
  std::vector<unsigned char> rgb;
};

float centre(float o, int i, float s) {
  float c = (float)i + 0.5f;
  c = c * s;
  return o + c;
}

bool inside(const int* k, int x, int y, int z) {
  return x >= k[0] && x < k[1] && y >= k[2] && y < k[3] && z >= k[4] && z < k[5];
}

// the header's extraction with the keep box, edge by edge
Points reference(int nx, int ny, int nz, const float* o, float voxel, const int* keep, const std::vector<float>& v,
                 float min_weight) {
  const size_t nvox = (size_t)nx * ny * nz;
  Points out;
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        const size_t a = ((size_t)z * ny + y) * nx + x;
        const int d[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        for (int k = 0; k < 3; ++k) {
          const int bx = x + d[k][0], by = y + d[k][1], bz = z + d[k][2];
          if (bx >= nx || by >= ny || bz >= nz) continue;
          const size_t b = ((size_t)bz * ny + by) * nx + bx;
          if (!(v[nvox + a] >= min_weight && v[nvox + b] >= min_weight && ((v[a] < 0.0f) != (v[b] < 0.0f)))) continue;
          if (inside(keep, x, y, z) && inside(keep, bx, by, bz)) continue;
          float frac = v[a] - v[b];
          frac = v[a] / frac;
          float c[3] = {centre(o[0], x, voxel), centre(o[1], y, voxel), centre(o[2], z, voxel)};
          float along = frac * voxel;
          c[k] = c[k] + along;
          for (int j = 0; j < 3; ++j) out.xyz.push_back(c[j]);
          for (int ch = 0; ch < 3; ++ch) {
            const float ca = v[(2 + ch) * nvox + a], cb = v[(2 + ch) * nvox + b];
            float col = cb - ca;
            col = frac * col;
            col = ca + col;
            col = col >= 0.0f ? col : 0.0f;
            col = col <= 1.0f ? col : 1.0f;
            col = col * 255.0f;
            col = col + 0.5f;
            out.rgb.push_back((unsigned char)(int)col);
          }
        }
      }
  return out;
}

void run_leaving(const char* name, int nx, int ny, int nz, const int* keep, float min_weight) {
  const size_t nvox = (size_t)nx * ny * nz;
  const float o[3] = {-1.85f, -0.9f, 0.45f}, voxel = 0.1f;
  std::vector<float> v(5 * nvox);
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        const size_t i = ((size_t)z * ny + y) * nx + x;
        v[i] = 0.11f * (float)z - 0.03f * (float)x + 0.05f * (float)y - 1.37f + 0.4f * std::sin(0.9f * (float)(x + 2 * y));
        v[nvox + i] = (float)((x * 7 + y * 3 + z) % 4);      // weights 0 .. 3
        for (int ch = 0; ch < 3; ++ch) v[(2 + ch) * nvox + i] = -0.1f + 1.2f * (float)((i * (ch + 3)) % 17) / 16.0f;
      }
  const Points want = reference(nx, ny, nz, o, voxel, keep, v, min_weight);
  const int total = (int)want.xyz.size() / 3;
  const size_t ws_bytes = scsfm_roll_ws_bytes(nx, ny, nz);
  expect(ws_bytes == 4 * (4 + 2 * ((nvox + 1023) / 1024)), "scsfm_roll_ws_bytes");
  int* ws = (int*)std::aligned_alloc(16, (ws_bytes + 15) / 16 * 16);  // (the library asks for 16-byte alignment)
  for (size_t i = 0; i < ws_bytes / 4; ++i) ws[i] = -7;
  expect(scsfm_roll_count(nx, ny, nz, keep[0], keep[1], keep[2], keep[3], keep[4], keep[5], v.data(), min_weight, ws,
                          ws_bytes, nullptr) == 0, "scsfm_roll_count");
  expect(ws[0] == total && ws[1] == -7 && ws[3] == -7, "the count");
  for (int cap : {total, total > 40 ? total - 37 : total / 2, 0}) {
    std::vector<float> xyz((size_t)3 * cap, -1.0f);
    std::vector<unsigned char> rgb((size_t)3 * cap, 0xAB);
    expect(scsfm_roll_extract(nx, ny, nz, o[0], o[1], o[2], voxel, keep[0], keep[1], keep[2], keep[3], keep[4], keep[5],
                              v.data(), min_weight, ws, ws_bytes, cap, cap ? xyz.data() : nullptr,
                              cap ? rgb.data() : nullptr, nullptr) == 0, "scsfm_roll_extract");
    if (!cap) continue;  // (nothing to compare: the vectors are empty)
    expect(!std::memcmp(xyz.data(), want.xyz.data(), xyz.size() * 4), "the points or their order differ");
    expect(!std::memcmp(rgb.data(), want.rgb.data(), rgb.size()), "the colours differ");
  }
  std::free(ws);
  std::printf("%-14s min_weight %g: %d points leave\n", name, min_weight, total);
}

}  // namespace

int main() {
  const int n[3] = {37, 18, 29};
  run_shift(37, 18, 29, 0, 0, 0);
  for (int axis = 0; axis < 3; ++axis)
    for (int k : {1, -1, 3, -5, 8, -8, n[axis] - 1, n[axis], -(n[axis] + 3)})
      run_shift(37, 18, 29, axis == 0 ? k : 0, axis == 1 ? k : 0, axis == 2 ? k : 0);
  run_shift(37, 18, 29, 8, -8, 16);
  run_shift(37, 18, 29, -3, 5, -7);
  run_shift(37, 18, 29, 2147483647, 0, 0);
  run_shift(37, 18, 29, 0, -2147483647 - 1, 0);
  for (int k : {0, 1, -1, 3, 4, -7}) run_shift(4, 1, 1, k, 0, 0);
  run_shift(4, 1, 1, 0, 1, 0);
  for (int k : {0, 1, -1}) run_shift(1, 1, 1, k, 0, 0);
  run_shift(40, 6, 5, 4, 0, 0);   // rows of whole groups, moved by a whole group
  run_shift(40, 6, 5, -3, 1, -1);
  std::printf("shift: 37 x 18 x 29, 4 x 1 x 1, 1 x 1 x 1 and 40 x 6 x 5 at four alignments of dst\n");
  const int boxes[][6] = {{0, 0, 0, 0, 0, 0},    {9, 9, 0, 18, 0, 29},  {0, 37, 0, 18, 0, 29}, {8, 37, 0, 18, 0, 29},
                          {0, 37, 0, 10, 0, 29}, {0, 37, 0, 18, 8, 29}, {0, 34, 5, 18, 0, 22}, {17, 18, 0, 18, 0, 29},
                          {0, 37, 0, 18, 11, 12}, {5, 30, 3, 14, 2, 20}};
  const char* names[] = {"empty", "empty on x", "whole", "shift 8 0 0", "shift 0 -8 0", "shift 0 0 8", "shift -3 5 -7",
                         "one thick, x", "one thick, z", "cuts a chunk"};
  for (float min_weight : {1.0f, 2.0f})
    for (int b = 0; b < 10; ++b) run_leaving(names[b], 37, 18, 29, boxes[b], min_weight);
  // rejected arguments touch no pointer
  float one = 0.0f;
  expect(scsfm_roll_shift(0, 1, 1, 0, 0, 0, &one, &one + 1, nullptr) == -1, "shift with nx = 0");
  expect(scsfm_roll_shift(1, 1, 1, 0, 0, 0, &one, &one, nullptr) == -1, "shift with dst == src");
  expect(scsfm_roll_shift(1, 1, 1, 0, 0, 0, nullptr, &one, nullptr) == -1, "shift with a NULL src");
  expect(scsfm_roll_shift(1024, 1024, 513, 0, 0, 0, &one, &one + 1, nullptr) == -1, "shift with more than 2^29 voxels");
  expect(scsfm_roll_ws_bytes(0, 1, 1) == 0 && scsfm_roll_ws_bytes(1024, 1024, 513) == 0, "ws_bytes of rejected sizes");
  expect(scsfm_roll_count(37, 18, 29, 0, 0, 0, 0, 0, 0, nullptr, 1.0f, nullptr, 0, nullptr) == -1, "count with NULL pointers");
  expect(scsfm_roll_extract(37, 18, 29, 0, 0, 0, 0.1f, 0, 0, 0, 0, 0, 0, nullptr, 1.0f, nullptr, 0, 5, nullptr, nullptr,
                            nullptr) == -1, "extract with NULL pointers");
  std::printf(fails ? "roll_check: %d FAILED\n" : "roll_check: ok\n", fails);
  return fails ? 1 : 0;
}
