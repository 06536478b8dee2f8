// hostsim -- what csrc_nets/scsfm_decoder.hip uses of the HIP device library beyond tests/hostsim/hip/hip_runtime.h: the
// integer min / max that hipcc declares for device code.  Injected with -include by tests/_hostsim_nets.py alone, so the
// other simulator libraries build exactly as before.  TEST INFRASTRUCTURE ONLY.
#pragma once
static inline int min(int a, int b) { return b < a ? b : a; }
static inline int max(int a, int b) { return a < b ? b : a; }
