// tests/native/sim_forced_page_omit_gated.cpp -- host build of the gated page-scope aligner with omission (TEST ONLY).
//
// Compiles text_alignment_amd/csrc/ta_forced_page_omit_gated.hip ITSELF (and with it forced_page_omit.h, the kernel) against
// tests/native/hipshim, sim_forced_shim.h and sim_forced_omit_shim.h, as sim_forced_page_omit.cpp does;
// tests/test_forced_page_omit_gated_sim.py drives ta_forced_align_pages_omit_gated and
// ta_forced_page_omit_gated_workspace_bytes of this library (host pointers where the real ones take device pointers)
// against tests/forced_page_omit_ref.py: the gate in front of every check, the cap that sizes the workspace, one launch per
// variant up to the widest cap's.
// With SIM_FORCED_PAGE_OMIT_GATED_MAIN it is a stand-alone program (exit status 0 if every page came back as expected) that
// a host sanitizer can be put on: g++ -fsanitize=address,undefined -DSIM_FORCED_PAGE_OMIT_GATED_MAIN ...
// Build: g++ -O2 -std=c++17 -shared -fPIC -I tests/native/hipshim (tests/simlib.py does it).
#include "sim_forced_shim.h"
#include "sim_forced_omit_shim.h"

#include <string>

sim_idx threadIdx, blockIdx;
sim_wave sim_w;

static std::string last_error;
int ta_fail(int code, const char* what) { last_error = what; return code; }
int ta_fail_hip(hipError_t, const char* where) { last_error = where; return -3; }
extern "C" const char* sim_forced_page_omit_gated_last_error() { return last_error.c_str(); }

#include "../../text_alignment_amd/csrc/ta_forced_page_omit_gated.hip"

#ifdef SIM_FORCED_PAGE_OMIT_GATED_MAIN
#include <cstdio>
#include <vector>
int main() {
    // sim_forced_page_omit.cpp's three pages (K = 2 with more characters than frames, K = 4, K = 32) and between them a gated
    // page without lines and without text; the caps are min(n, 1023), so every piece is sized for a wider variant than the
    // page's windows need
    const int no = 5, npages = 4, nlines = 7;
    const int32_t T[nlines] = {2, 2, 2, 9, 33, 8, 12}, lo[nlines] = {0, 5, 12, 0, 60, 0, 590},
                  hi[nlines] = {9, 16, 20, 100, 130, 600, 640};
    const int64_t line_first[npages + 1] = {0, 3, 3, 5, 7}, lab_off[npages + 1] = {0, 20, 20, 150, 790};
    const int32_t gate[npages] = {0, 4, 0, 0}, cap[npages] = {20, 0, 130, 640};
    std::vector<int64_t> row_off(nlines), ws_off(nlines);
    int64_t rows = 0, ws = 0;
    for (int p = 0; p < npages; ++p)
        for (int64_t q = line_first[p]; q < line_first[p + 1]; ++q) {
            row_off[q] = rows; ws_off[q] = ws;
            rows += T[q]; ws += ta_forced_page_omit_gated_workspace_bytes(1, T + q, cap[p]);
        }
    const int64_t nlab = lab_off[npages];
    std::vector<float> probs(rows * no);
    uint32_t x = 12345;
    for (float& p : probs) { x = x * 1664525u + 1013904223u; p = (float)(x >> 8) / (float)(1u << 24); }
    std::vector<int32_t> labels(nlab), frames(4 * nlab), status(npages, -7);
    for (int64_t i = 0; i < nlab; ++i) { x = x * 1664525u + 1013904223u; labels[i] = 1 + (int)((x >> 16) % (no - 1)); }
    std::vector<int64_t> score(npages);
    std::vector<unsigned char> work(ws + 16);
    unsigned char* w = work.data() + ((16 - (reinterpret_cast<uintptr_t>(work.data()) & 15)) & 15);
    for (int omit : {0, 3 << 16, 1 << 26}) {
        const int rc = ta_forced_align_pages_omit_gated(probs.data(), row_off.data(), T, line_first, lo, hi, labels.data(),
                                                        lab_off, ws_off.data(), gate, cap, npages, nlines, no, rows, nlab, T,
                                                        line_first, lab_off, cap, omit, w, ws, frames.data(), score.data(),
                                                        status.data(), nullptr);
        if (rc != 0 || status[0] != 0 || status[1] != TA_FORCED_SKIPPED || status[2] != 0 || status[3] != 0) {
            std::printf("omit %d: rc %d (%s), status %d %d %d %d\n", omit, rc, last_error.c_str(), status[0], status[1],
                        status[2], status[3]);
            return 1;
        }
        std::printf("omit %d: scores %lld %lld %lld\n", omit, (long long)score[0], (long long)score[2], (long long)score[3]);
    }
    return 0;
}
#endif
