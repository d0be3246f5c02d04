// tests/native/sim_forced_shim.h -- TEST ONLY: what csrc/ta_forced.hip uses beyond tests/native/hipshim.  The kernel
// hands LDS from lane to lane of one wave with a compiler-level fence and wave barrier (no instruction on the GPU, where a
// wave's LDS operations run in program order); among coroutines that hand-over has to be a rendezvous.
#pragma once
#include <hip/hip_runtime.h>

inline void __builtin_amdgcn_fence(int, const char*) {}
inline void __builtin_amdgcn_wave_barrier() { sim_meet(); }
