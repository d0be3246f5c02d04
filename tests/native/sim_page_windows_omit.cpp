// tests/native/sim_page_windows_omit.cpp -- host build of the page-scope window kernel for the lattice with omission
// (TEST ONLY).
//
// Compiles text_alignment_amd/csrc/ta_page_windows_omit.hip ITSELF (and with it page_windows.h, the kernel) against
// tests/native/hipshim, sim_forced_shim.h and sim_forced_omit_shim.h, as sim_page_windows.cpp does for the strict entry;
// tests/test_page_windows_omit_sim.py drives ta_page_windows_omit of this library (host pointers where the real one takes
// device pointers) against forced.page_scope_eligibility(..., omit=True).
// With SIM_PAGE_WINDOWS_OMIT_MAIN it is a stand-alone program (exit status 0 if every answer is the expected one) that a
// host sanitizer can be put on: g++ -fsanitize=address,undefined -DSIM_PAGE_WINDOWS_OMIT_MAIN ...
// Build: g++ -O2 -std=c++17 -shared -fPIC -I tests/native/hipshim (tests/simlib.py does it).
#include "sim_forced_shim.h"
#include "sim_forced_omit_shim.h"

#include <string>

sim_idx threadIdx, blockIdx;
sim_wave sim_w;

static std::string last_error;
int ta_fail(int code, const char* what) { last_error = what; return code; }
int ta_fail_hip(hipError_t, const char* where) { last_error = where; return -3; }
extern "C" const char* sim_page_windows_omit_last_error() { return last_error.c_str(); }

#include "../../text_alignment_amd/csrc/ta_page_windows_omit.hip"

#ifdef SIM_PAGE_WINDOWS_OMIT_MAIN
#include <cstdio>
#include <vector>
int main() {
    // sim_page_windows.cpp's three pages with ONE frame per line: page 0 (12 characters on 3 frames) and page 1 have fewer
    // frames than the strict rule asks for and are eligible all the same; page 2 is not plain
    const int npages = 3, nl[npages] = {3, 130, 2}, n[npages] = {12, 130, 5};
    std::vector<int64_t> line_first{0}, t_off{0};
    for (int p = 0; p < npages; ++p) { line_first.push_back(line_first.back() + nl[p]); t_off.push_back(t_off.back() + n[p]); }
    const int nlines = (int)line_first.back();
    const int64_t t_len = t_off.back();
    std::vector<int32_t> table(nlines * TA_HARVEST_FIELDS, 0), T(nlines, 1), t_class(t_len, 3), h_status(npages, 0);
    auto row = [&](int q, int reason, int first, int L) {
        table[q * TA_HARVEST_FIELDS] = reason; table[q * TA_HARVEST_FIELDS + 1] = first; table[q * TA_HARVEST_FIELDS + 2] = L;
    };
    row(0, 0, 0, 4); row(1, TA_HARVEST_EMPTY, 0, 0); row(2, 0, 7, 5);
    for (int k = 0; k < 130; ++k) row(3 + k, 0, k, 1);
    row(133, 0, 0, 2); row(134, 0, 2, 3);
    const uint8_t plain[npages] = {1, 1, 0};
    std::vector<int32_t> lo(nlines, -7), hi(nlines, -7), reason(npages, -7);
    const int rc = ta_page_windows_omit(table.data(), h_status.data(), line_first.data(), t_off.data(), t_class.data(),
                                        T.data(), plain, npages, nlines, t_len, 1, lo.data(), hi.data(), reason.data(), nullptr);
    bool ok = rc == 0 && reason[0] == 0 && reason[1] == 0 && reason[2] == TA_PAGE_SCOPE_NOT_PLAIN;
    const int want_lo[3] = {0, 3, 5}, want_hi[3] = {5, 5, 12};
    for (int k = 0; k < 3; ++k) ok = ok && lo[k] == want_lo[k] && hi[k] == want_hi[k];
    for (int k = 0; k < 130; ++k) {
        const int l = k == 0 ? 0 : k - 1, h = k == 129 ? 130 : k + 2;
        ok = ok && lo[3 + k] == l && hi[3 + k] == h;
    }
    ok = ok && lo[133] == -7 && hi[134] == -7;
    std::printf("rc %d (%s), reasons %d %d %d: %s\n", rc, last_error.c_str(), reason[0], reason[1], reason[2], ok ? "ok" : "WRONG");
    return ok ? 0 : 1;
}
#endif
