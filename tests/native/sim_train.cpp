// tests/native/sim_train.cpp -- host build of the training kernels (TEST ONLY).
//
// Compiles text_alignment_amd/csrc/ta_train.hip ITSELF -- not a restatement -- against tests/native/hipshim_wg, where a
// workgroup is the launch's block.x lanes (512 for the two LSTM kernels, 128 for the output layer, 256 for the CTC
// lattice) that meet at every barrier.  The library this makes exports the same ta_lstm_train_forward /
// ta_lstm_train_backward / ta_ctc_align / ta_ctc_workspace_bytes, taking host pointers where the real ones take device
// pointers, so the output layer's row tail, the lattice's strided state loops, the first and last steps of the
// recurrences, the clamps and the kernels' own refusals are run against tests/train_ref.py without a GPU
// (tests/test_train_sim.py).
// Build: g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I tests/native/hipshim_wg (no contraction: only the
// kernels' explicit fma() calls are fused, as on the device).
#include <hip/hip_runtime.h>

#include <string>

dim3 threadIdx, blockIdx, gridDim, blockDim;
sim_group sim_g;

static std::string last_error;
int ta_fail(int code, const char* what) { last_error = what; return code; }
int ta_fail_hip(hipError_t, const char* where) { last_error = where; return -3; }
extern "C" const char* sim_train_last_error() { return last_error.c_str(); }

#include "../../text_alignment_amd/csrc/ta_train.hip"
