// tests/native/sim_errs.cpp -- host build of the held-out scoring kernel (TEST ONLY).
//
// Compiles text_alignment_amd/csrc/ta_errs.hip ITSELF -- not a restatement -- against tests/native/hipshim, where a
// wave is 64 coroutines that meet at every wave-wide operation.  The library this makes exports the same
// ta_errs_workspace_bytes / ta_edit_distance, taking host pointers where the real ones take device pointers, so the
// filter, the strip hand-over, the pointer layout, the walk and every bounds check are run against tests/errs_ref.py
// without a GPU, and under a host sanitizer if one is wanted.
// Build: g++ -O2 -std=c++17 -shared -fPIC -I tests/native/hipshim (tests/test_errs_sim.py does it).
#include <hip/hip_runtime.h>

#include <string>

sim_idx threadIdx, blockIdx;
sim_wave sim_w;

static std::string last_error;
int ta_fail(int code, const char* what) { last_error = what; return code; }
int ta_fail_hip(hipError_t, const char* where) { last_error = where; return -3; }
extern "C" const char* sim_errs_last_error() { return last_error.c_str(); }

#include "../../text_alignment_amd/csrc/ta_errs.hip"
