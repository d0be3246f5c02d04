// tests/native/sim_forced.cpp -- host build of the forced-alignment kernel (TEST ONLY).
//
// Compiles text_alignment_amd/csrc/ta_forced.hip ITSELF -- not a restatement -- against tests/native/hipshim (a wave is 64
// coroutines that meet at every wave-wide operation) and sim_forced_shim.h.  The library this makes exports the same
// ta_forced_workspace_bytes / ta_forced_align, taking host pointers where the real ones take device pointers, so the
// emission scores, the lane hand-over, the packing of the moves, the walk's blocks and every bounds check are run against
// tests/forced_ref.py without a GPU, and under a host sanitizer if one is wanted.
// Build: g++ -O2 -std=c++17 -shared -fPIC -I tests/native/hipshim (tests/test_forced_sim.py does it).
#include "sim_forced_shim.h"

#include <string>

sim_idx threadIdx, blockIdx;
sim_wave sim_w;

static std::string last_error;
int ta_fail(int code, const char* what) { last_error = what; return code; }
int ta_fail_hip(hipError_t, const char* where) { last_error = where; return -3; }
extern "C" const char* sim_forced_last_error() { return last_error.c_str(); }

#include "../../text_alignment_amd/csrc/ta_forced.hip"
