// tests/native/sim_forced_page.cpp -- host build of the page-scope forced-alignment kernel (TEST ONLY).
//
// Compiles text_alignment_amd/csrc/ta_forced_page.hip ITSELF -- not a restatement -- against tests/native/hipshim (a wave
// is 64 coroutines that meet at every wave-wide operation) and sim_forced_shim.h.  The library this makes exports the same
// ta_forced_page_workspace_bytes / ta_forced_page_variant / ta_forced_align_pages, taking host pointers where the real
// ones take device pointers, so the re-basing at the line boundaries, the first-frame step, the packing of the moves per
// line, the walk through the lines and every bounds check are run against tests/forced_page_ref.py without a GPU.
// Build: g++ -O2 -std=c++17 -shared -fPIC -I tests/native/hipshim (tests/test_forced_page_sim.py does it).
#include "sim_forced_shim.h"

#include <string>

sim_idx threadIdx, blockIdx;
sim_wave sim_w;

static std::string last_error;
int ta_fail(int code, const char* what) { last_error = what; return code; }
int ta_fail_hip(hipError_t, const char* where) { last_error = where; return -3; }
extern "C" const char* sim_forced_page_last_error() { return last_error.c_str(); }

#include "../../text_alignment_amd/csrc/ta_forced_page.hip"
