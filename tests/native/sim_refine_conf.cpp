// tests/native/sim_refine_conf.cpp -- host build of the confidence-spreading kernel (TEST ONLY).
//
// Compiles text_alignment_amd/csrc/ta_refine_conf.hip ITSELF -- not a restatement -- against tests/native/hipshim, where a
// wave is 64 coroutines that meet at every wave-wide operation and the workgroups of a launch run one after the other.
// The library this makes exports the same ta_confidence_pages, taking host pointers where the real one takes device
// pointers, so the checks, the fill, the spread, the reduction and every refusal are run against
// tests/refine_conf_ref.py without a GPU, and under a host sanitizer if one is wanted.
// The kernel uses nothing the shim lacks.
// Build: g++ -O2 -std=c++17 -shared -fPIC -I tests/native/hipshim (tests/test_refine_conf_sim.py does it).
#include <hip/hip_runtime.h>

#include <string>

sim_idx threadIdx, blockIdx;
sim_wave sim_w;

static std::string last_error;
int ta_fail(int code, const char* what) { last_error = what; return code; }
int ta_fail_hip(hipError_t, const char* where) { last_error = where; return -3; }
extern "C" const char* sim_refine_conf_last_error() { return last_error.c_str(); }

#include "../../text_alignment_amd/csrc/ta_refine_conf.hip"
