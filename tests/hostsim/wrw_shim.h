// hostsim -- what csrc_wrw/scsfm_conv_wrw.hip uses beyond tests/hostsim/hip/hip_runtime.h: the fp32 matrix instruction
// v_mfma_f32_16x16x4_f32 and its accumulator type.  Injected with -include by tests/_hostsim_wrw.py alone, so the other
// simulator libraries build exactly as before.  TEST INFRASTRUCTURE ONLY.
//
// The instruction is a wave-cooperative D = A * B + C with A 16 x 4 (lane l holds A[l & 15][l >> 4]), B 4 x 16 (lane l
// holds B[l >> 4][l & 15]) and C/D 16 x 16 (lane l holds column l & 15, rows 4 * (l >> 4) + i in register i).  Its
// result is, bit for bit, the k-ordered fp32 fmaf chain D = fma(a_k3, b_k3, fma(a_k2, b_k2, fma(a_k1, b_k1,
// fma(a_k0, b_k0, C)))): that chain is what runs here.  The 64 fibres of a wave publish their operands, meet at the wave
// barrier, gather, and meet again before the exchange buffer is reused.  Needs full 64-lane waves with every lane
// taking part, as the hardware does.
#pragma once
#include <hip/hip_runtime.h>

#define SCSFM_WRW_F32X4 1
typedef float f32x4 __attribute__((vector_size(16)));

static inline f32x4 __builtin_amdgcn_mfma_f32_16x16x4f32(float a, float b, f32x4 c, int, int, int) {
  hostsim::State& s = hostsim::S();
  const int w = s.cur / 64, lane = s.cur % 64;
  uint32_t ua, ub;
  memcpy(&ua, &a, 4);
  memcpy(&ub, &b, 4);
  s.xbuf[w * 64 + lane] = (uint64_t)ua | ((uint64_t)ub << 32);
  hostsim::wave_barrier();
  const int col = lane & 15, row0 = (lane >> 4) * 4;
  for (int k = 0; k < 4; ++k) {
    const uint32_t vb = (uint32_t)(s.xbuf[w * 64 + 16 * k + col] >> 32);
    float bk;
    memcpy(&bk, &vb, 4);
    for (int i = 0; i < 4; ++i) {
      const uint32_t va = (uint32_t)s.xbuf[w * 64 + 16 * k + row0 + i];
      float ak;
      memcpy(&ak, &va, 4);
      c[i] = fmaf(ak, bk, c[i]);
    }
  }
  hostsim::wave_barrier();
  return c;
}
