// tests/native/sim_forced_post.cpp -- host build of the forced-alignment posterior kernel (TEST ONLY).
//
// Compiles text_alignment_amd/csrc/ta_forced_post.hip ITSELF -- not a restatement -- against tests/native/hipshim (a wave
// is 64 coroutines that meet at every wave-wide operation), sim_forced_shim.h and sim_forced_conf_shim.h (the two DPP
// controls of the moves from the left and from the right lane).  The library this makes exports the same
// ta_forced_posterior_workspace_bytes / ta_forced_posterior, taking host pointers where the real ones take device
// pointers, so both fills, the renormalisation, the kept rows, the query cursor, the combine and every bounds check are run
// against tests/forced_post_ref.py without a GPU.  The kernel's frexp / ldexp are <math.h>'s here, exact as the device's.
// With SIM_FORCED_POST_MAIN it is a stand-alone program (one small call, exit status 0 if every line came back
// TA_FORCED_OK) that a host sanitizer can be put on: g++ -fsanitize=address,undefined -DSIM_FORCED_POST_MAIN ...
// Build: g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I tests/native/hipshim (tests/test_forced_post_sim.py does it).
#include "sim_forced_conf_shim.h"

#include <math.h>

#include <string>

sim_idx threadIdx, blockIdx;
sim_wave sim_w;

static std::string last_error;
int ta_fail(int code, const char* what) { last_error = what; return code; }
int ta_fail_hip(hipError_t, const char* where) { last_error = where; return -3; }
extern "C" const char* sim_forced_last_error() { return last_error.c_str(); }

#include "../../text_alignment_amd/csrc/ta_forced_post.hip"

#ifdef SIM_FORCED_POST_MAIN
#include <cstdio>
int main() {
    const int no = 5, n = 3;
    const int32_t T[n] = {9, 40, 300}, L[n] = {3, 7, 140};
    std::vector<int64_t> row_off(n), lab_off(n), ws_off(n);
    int64_t rows = 0, nlab = 0, ws = 0;
    for (int b = 0; b < n; ++b) {
        row_off[b] = rows; lab_off[b] = nlab; ws_off[b] = ws;
        rows += T[b]; nlab += L[b]; ws += ta_forced_posterior_workspace_bytes(T[b], L[b]);
    }
    std::vector<float> probs(rows * no);
    uint32_t x = 12345;
    for (float& p : probs) { x = x * 1664525u + 1013904223u; p = (float)(x >> 8) / (float)(1u << 24); }
    std::vector<int32_t> labels(nlab), tq(nlab), own_x(nlab), rival_x(nlab), rival(nlab), z_x(n), status(n);
    for (int64_t i = 0; i < nlab; ++i) { x = x * 1664525u + 1013904223u; labels[i] = 1 + (int)((x >> 16) % (no - 1)); }
    for (int b = 0; b < n; ++b)                          // spread over the line, the first at 0 and the last at T - 1
        for (int i = 0; i < L[b]; ++i) tq[lab_off[b] + i] = L[b] == 1 ? 0 : (int)((int64_t)i * (T[b] - 1) / (L[b] - 1));
    std::vector<double> own_m(nlab), rival_m(nlab), z_m(n);
    std::vector<unsigned char> work(ws + 16);
    unsigned char* w = work.data() + ((16 - (reinterpret_cast<uintptr_t>(work.data()) & 15)) & 15);
    const int rc = ta_forced_posterior(probs.data(), row_off.data(), T, labels.data(), lab_off.data(), L, ws_off.data(),
                                       tq.data(), n, no, rows, nlab, T, L, w, ws, own_m.data(), own_x.data(), rival_m.data(),
                                       rival_x.data(), rival.data(), z_m.data(), z_x.data(), status.data(), nullptr);
    if (rc != 0 || status[0] != 0 || status[1] != 0 || status[2] != 0) {
        std::printf("rc %d, status %d %d %d\n", rc, status[0], status[1], status[2]);
        return 1;
    }
    std::printf("log2 P(text | line) %.3f %.3f %.3f\n", log2(z_m[0]) + z_x[0], log2(z_m[1]) + z_x[1], log2(z_m[2]) + z_x[2]);
    return 0;
}
#endif
