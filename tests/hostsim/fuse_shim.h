// hostsim -- what csrc_fuse/scsfm_fuse.hip uses beyond tests/hostsim/hip/hip_runtime.h: the wave's ballot and the
// population count.  Injected with -include by tests/_hostsim_fuse.py alone, so the other simulator libraries build
// exactly as before.  TEST INFRASTRUCTURE ONLY.
//
// The 64 fibres of a wave publish their predicate, meet at the wave barrier, gather the bits of the lanes the wave has,
// and meet again before the exchange buffer is reused.  Every lane of the wave that is still running must take part, as
// on the hardware a lane that has left contributes 0.
#pragma once
#include <hip/hip_runtime.h>

static inline unsigned long long __ballot(int predicate) {
  hostsim::State& s = hostsim::S();
  const int w = s.cur / 64, lane = s.cur % 64;
  s.xbuf[w * 64 + lane] = predicate ? 1 : 0;
  hostsim::wave_barrier();
  int nl = s.nthreads - w * 64;
  if (nl > 64) nl = 64;
  unsigned long long bits = 0;
  for (int l = 0; l < nl; ++l) {
    if (s.xbuf[w * 64 + l] && !s.fibers[w * 64 + l].done) bits |= 1ull << l;
  }
  hostsim::wave_barrier();
  return bits;
}
static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
