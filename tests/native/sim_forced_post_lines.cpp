// tests/native/sim_forced_post_lines.cpp -- host build of the posterior kernel for its entry whose line list lies "on the
// device" (TEST ONLY).
//
// Compiles text_alignment_amd/csrc/ta_forced_post.hip ITSELF -- not a restatement -- as sim_forced_post.cpp does (the same
// shims: tests/native/hipshim, sim_forced_shim.h, sim_forced_conf_shim.h; <math.h>'s frexp / ldexp) and holds the library
// to the entry points tests/test_forced_post_lines_sim.py drives: ta_forced_posterior_lines and
// ta_forced_posterior_lines_workspace_bytes, taking host pointers where the real ones take device pointers.  A source
// without them does not link.
// With SIM_FORCED_POST_LINES_MAIN it is a stand-alone program (one small chunk: four slots on six lines, the second
// skipped and the third refused through a peak that decreases; exit status 0 if the statuses are OK, SKIPPED, QUERY, OK
// and the two slots' rows were left alone) that a host sanitizer can be put on:
// g++ -fsanitize=address,undefined -DSIM_FORCED_POST_LINES_MAIN ...
// Build: g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I tests/native/hipshim (tests/test_forced_post_lines_sim.py
// does it).
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

// the entry points this build is for, by name
extern "C" void* sim_forced_post_lines_entry(int which) {
    return which ? reinterpret_cast<void*>(&ta_forced_posterior_lines)
                 : reinterpret_cast<void*>(&ta_forced_posterior_lines_workspace_bytes);
}

#ifdef SIM_FORCED_POST_LINES_MAIN
#include <cstdio>
int main() {
    const int no = 5, nall = 6, nslots = 4;
    const int32_t T_all[nall] = {1, 9, 40, 1, 300, 25}, Lcap[nall] = {0, 4, 7, 0, 149, 6};
    const int32_t acc_line[nslots] = {1, 2, 5, 4}, L[nslots] = {3, 7, 6, 140};
    const int32_t align_status[nslots] = {TA_FORCED_OK, TA_FORCED_BOUNDS, TA_FORCED_OK, TA_FORCED_OK};
    std::vector<int64_t> row_off(nall), lab_off(nslots);
    int64_t rows = 0, nlab = 0;
    for (int q = 0; q < nall; ++q) { row_off[q] = rows; rows += T_all[q]; }
    for (int k = 0; k < nslots; ++k) { lab_off[k] = nlab; nlab += L[k]; }
    std::vector<float> probs(rows * no);
    uint32_t x = 12345;
    for (float& p : probs) { x = x * 1664525u + 1013904223u; p = (float)(x >> 8) / (float)(1u << 24); }
    std::vector<int32_t> labels(nlab), frames(nlab * TA_FORCED_FIELDS, -77), status(nslots, -5);
    std::vector<int32_t> own_x(nlab, -5), rival_x(nlab, -5), rival(nlab, -5), z_x(nslots, -5);
    std::vector<double> own_m(nlab, -5.0), rival_m(nlab, -5.0), z_m(nslots, -5.0);
    for (int64_t i = 0; i < nlab; ++i) { x = x * 1664525u + 1013904223u; labels[i] = 1 + (int)((x >> 16) % (no - 1)); }
    for (int k = 0; k < nslots; ++k) {                   // peaks spread over the line; the skipped slot's rows stay -77
        if (align_status[k] != TA_FORCED_OK) continue;
        const int t = T_all[acc_line[k]];
        for (int i = 0; i < L[k]; ++i)
            frames[(lab_off[k] + i) * TA_FORCED_FIELDS + 2] = L[k] == 1 ? 0 : (int)((int64_t)i * (t - 1) / (L[k] - 1));
    }
    frames[(lab_off[2] + 3) * TA_FORCED_FIELDS + 2] = 0; // the third slot's peaks decrease: refused on the "device"
    const int64_t count[2] = {nslots, nlab};
    const int64_t ws = ta_forced_posterior_lines_workspace_bytes(nlab, 149);
    std::vector<unsigned char> work(ws + 16);
    unsigned char* w = work.data() + ((16 - (reinterpret_cast<uintptr_t>(work.data()) & 15)) & 15);
    const int rc = ta_forced_posterior_lines(probs.data(), row_off.data(), T_all, Lcap, acc_line, L, lab_off.data(),
                                             labels.data(), count, align_status, frames.data(), nall, nslots, no, rows, nlab,
                                             T_all, Lcap, w, ws, own_m.data(), own_x.data(), rival_m.data(), rival_x.data(),
                                             rival.data(), z_m.data(), z_x.data(), status.data(), nullptr);
    bool ok = rc == 0 && status[0] == TA_FORCED_OK && status[1] == TA_FORCED_SKIPPED && status[2] == TA_FORCED_QUERY &&
              status[3] == TA_FORCED_OK;
    for (int k = 1; k <= 2; ++k) {
        ok = ok && z_m[k] == -5.0 && z_x[k] == -5;
        for (int i = 0; i < L[k]; ++i) ok = ok && own_m[lab_off[k] + i] == -5.0 && rival[lab_off[k] + i] == -5;
    }
    if (!ok) {
        std::printf("rc %d, status %d %d %d %d\n", rc, status[0], status[1], status[2], status[3]);
        return 1;
    }
    std::printf("log2 P(text | line) %.3f %.3f\n", log2(z_m[0]) + z_x[0], log2(z_m[3]) + z_x[3]);
    return 0;
}
#endif
