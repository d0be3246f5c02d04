// tests/native/sim_forced_page.cpp -- host build of the page-scope forced-alignment kernel (TEST ONLY).
//
// Compiles text_alignment_amd/csrc/ta_forced_page.hip ITSELF -- not a restatement -- against tests/native/hipshim (a wave
// is 64 coroutines that meet at every wave-wide operation) and sim_forced_shim.h.  The library this makes exports the same
// ta_forced_page_workspace_bytes / ta_forced_page_variant / ta_forced_align_pages, taking host pointers where the real
// ones take device pointers, so the re-basing at the line boundaries, the first-frame step, the packing of the moves per
// line, the walk through the lines and every bounds check are run against tests/forced_page_ref.py without a GPU.
// With SIM_FORCED_PAGE_MAIN it is a stand-alone program (one small call, exit status 0 if every page came back
// TA_FORCED_OK) that a host sanitizer can be put on: g++ -fsanitize=address,undefined -DSIM_FORCED_PAGE_MAIN ...
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

#ifdef SIM_FORCED_PAGE_MAIN
#include <cstdio>
#include <vector>
int main() {
    // three pages, as sim_forced_page_omit.cpp's but with frames enough for a strict path: K = 2 with windows that shift,
    // K = 4 with a window that drops 60 characters at the break, K = 32 with the whole text on both lines
    const int no = 5, npages = 3, nlines = 7;
    const int32_t T[nlines] = {8, 8, 8, 100, 100, 400, 400}, lo[nlines] = {0, 2, 5, 0, 60, 0, 0},
                  hi[nlines] = {4, 7, 9, 100, 130, 520, 520};
    const int64_t line_first[npages + 1] = {0, 3, 5, 7}, lab_off[npages + 1] = {0, 9, 139, 659};
    const int32_t Kp[npages] = {2, 4, 32};
    std::vector<int64_t> row_off(nlines), ws_off(nlines);
    int64_t rows = 0, ws = 0;
    for (int p = 0; p < npages; ++p)
        for (int64_t q = line_first[p]; q < line_first[p + 1]; ++q) {
            if (ta_forced_page_variant(hi[q] - lo[q]) > Kp[p]) return 2;
            row_off[q] = rows; ws_off[q] = ws;
            rows += T[q]; ws += ta_forced_page_workspace_bytes(1, T + q, Kp[p]);
        }
    const int64_t nlab = lab_off[npages];
    std::vector<float> probs(rows * no);
    uint32_t x = 12345;
    for (float& p : probs) { x = x * 1664525u + 1013904223u; p = (float)(x >> 8) / (float)(1u << 24); }
    std::vector<int32_t> labels(nlab), frames(4 * nlab), status(npages);
    for (int64_t i = 0; i < nlab; ++i) { x = x * 1664525u + 1013904223u; labels[i] = 1 + (int)((x >> 16) % (no - 1)); }
    std::vector<int64_t> score(npages);
    std::vector<unsigned char> work(ws + 16);
    unsigned char* w = work.data() + ((16 - (reinterpret_cast<uintptr_t>(work.data()) & 15)) & 15);
    const int rc = ta_forced_align_pages(probs.data(), row_off.data(), T, line_first, lo, hi, labels.data(), lab_off,
                                         ws_off.data(), npages, nlines, no, rows, nlab, T, line_first, lo, hi, lab_off, w, ws,
                                         frames.data(), score.data(), status.data(), nullptr);
    if (rc != 0 || status[0] != 0 || status[1] != 0 || status[2] != 0) {
        std::printf("rc %d (%s), status %d %d %d\n", rc, last_error.c_str(), status[0], status[1], status[2]);
        return 1;
    }
    std::printf("scores %lld %lld %lld\n", (long long)score[0], (long long)score[1], (long long)score[2]);
    return 0;
}
#endif
