// tests/native/sim_forced_page_post.cpp -- host build of the page-scope posterior kernel (TEST ONLY).
//
// Compiles text_alignment_amd/csrc/ta_forced_page_post.hip ITSELF -- not a restatement -- against tests/native/hipshim (a
// wave is 64 coroutines that meet at every wave-wide operation), sim_forced_shim.h and sim_forced_conf_shim.h (the two DPP
// controls of the moves from the left and from the right lane).  The library this makes exports the same
// ta_forced_page_posterior_workspace_bytes / ta_forced_page_posterior, taking host pointers where the real ones take
// device pointers, so both fills, the re-basing at the line boundaries in both directions, the renormalisation, the kept
// rows, the query cursor, the combine and every bounds check are run against tests/forced_page_post_ref.py without a GPU.
// The kernel's frexp / ldexp are <math.h>'s here, exact as the device's.
// With SIM_FORCED_PAGE_POST_MAIN it is a stand-alone program (one small call, exit status 0 if every page came back
// TA_FORCED_OK) that a host sanitizer can be put on: g++ -fsanitize=address,undefined -DSIM_FORCED_PAGE_POST_MAIN ...
// Build: g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -I tests/native/hipshim (tests/test_forced_page_post_sim.py
// does it).
#include "sim_forced_conf_shim.h"

#include <math.h>

#include <string>

sim_idx threadIdx, blockIdx;
sim_wave sim_w;

static std::string last_error;
int ta_fail(int code, const char* what) { last_error = what; return code; }
int ta_fail_hip(hipError_t, const char* where) { last_error = where; return -3; }
extern "C" const char* sim_forced_page_post_last_error() { return last_error.c_str(); }

#include "../../text_alignment_amd/csrc/ta_forced_page_post.hip"

#ifdef SIM_FORCED_PAGE_POST_MAIN
#include <cstdio>
#include <vector>
int main() {
    // three pages: K = 2 with windows that shift, K = 4 with a window that drops 60 characters at the break, K = 32 with
    // the whole text on both lines; character i of a page is queried where an even spread over the page's frames puts it
    const int no = 5, npages = 3, nlines = 7;
    const int32_t T[nlines] = {8, 8, 8, 100, 100, 400, 400}, lo[nlines] = {0, 2, 5, 0, 60, 0, 0},
                  hi[nlines] = {4, 7, 9, 100, 130, 520, 520};
    const int64_t line_first[npages + 1] = {0, 3, 5, 7}, lab_off[npages + 1] = {0, 9, 139, 659};
    const int32_t Kp[npages] = {2, 4, 32};
    std::vector<int64_t> row_off(nlines), ws_off(npages);
    int64_t rows = 0, ws = 0;
    for (int q = 0; q < nlines; ++q) { row_off[q] = rows; rows += T[q]; }
    for (int p = 0; p < npages; ++p) {
        ws_off[p] = ws;
        ws += ta_forced_page_posterior_workspace_bytes(lab_off[p + 1] - lab_off[p], Kp[p]);
    }
    const int64_t nlab = lab_off[npages];
    std::vector<float> probs(rows * no);
    uint32_t x = 12345;
    for (float& p : probs) { x = x * 1664525u + 1013904223u; p = (float)(x >> 8) / (float)(1u << 24); }
    std::vector<int32_t> labels(nlab), query(4 * nlab, -9), own_x(nlab), rival_x(nlab), rival(nlab), z_x(npages), status(npages);
    for (int64_t i = 0; i < nlab; ++i) { x = x * 1664525u + 1013904223u; labels[i] = 1 + (int)((x >> 16) % (no - 1)); }
    for (int p = 0; p < npages; ++p) {
        const int64_t n = lab_off[p + 1] - lab_off[p];
        int k = (int)line_first[p];
        for (int64_t i = 0; i < n; ++i) {                // the first line (from the one before) whose window holds i
            while (i >= hi[k]) ++k;
            const int w = hi[k] - lo[k];
            query[4 * (lab_off[p] + i)] = k - (int)line_first[p];
            query[4 * (lab_off[p] + i) + 3] = (int)((i - lo[k]) * (int64_t)(T[k] - 1) / (w > 1 ? w - 1 : 1));
        }
    }
    std::vector<double> own_m(nlab), rival_m(nlab), z_m(npages);
    std::vector<unsigned char> work(ws + 16);
    unsigned char* w = work.data() + ((16 - (reinterpret_cast<uintptr_t>(work.data()) & 15)) & 15);
    const int rc = ta_forced_page_posterior(probs.data(), row_off.data(), T, line_first, lo, hi, labels.data(), lab_off,
                                            ws_off.data(), query.data(), npages, nlines, no, rows, nlab, T, line_first, lo, hi,
                                            lab_off, w, ws, own_m.data(), own_x.data(), rival_m.data(), rival_x.data(),
                                            rival.data(), z_m.data(), z_x.data(), status.data(), nullptr);
    if (rc != 0 || status[0] != 0 || status[1] != 0 || status[2] != 0) {
        std::printf("rc %d (%s), status %d %d %d\n", rc, last_error.c_str(), status[0], status[1], status[2]);
        return 1;
    }
    std::printf("log2 P(text | page) %.3f %.3f %.3f\n", log2(z_m[0]) + z_x[0], log2(z_m[1]) + z_x[1], log2(z_m[2]) + z_x[2]);
    return 0;
}
#endif
