// tests/native/sim_refine_post.cpp -- host build of the posterior-spreading kernel (TEST ONLY).
//
// Compiles text_alignment_amd/csrc/ta_refine_conf.hip ITSELF -- not a restatement -- against tests/native/hipshim, as
// sim_refine_conf.cpp does, and holds the library to the entry tests/test_posterior_pages_sim.py drives:
// ta_posterior_pages, taking host pointers where the real one takes device pointers.  A source without it does not link.
// The kernel's division and ldexp are the host's here (IEEE, round to nearest-even; no -ffast-math), so the checks, the
// fill, the spread, the reduction and every refusal are run against tests/refine_post_ref.py without a GPU.
// With SIM_REFINE_POST_MAIN it is a stand-alone program (two pages of one refined line each, the second line's slot
// refused by the posterior call; exit status 0 if the statuses are OK and STATUS, the first page holds its three
// quotients and the second page's words were left alone) that a host sanitizer can be put on:
// g++ -fsanitize=address,undefined -DSIM_REFINE_POST_MAIN ...
// Build: g++ -O2 -std=c++17 -shared -fPIC -I tests/native/hipshim (tests/test_posterior_pages_sim.py does it).
#include <hip/hip_runtime.h>

#include <string>

sim_idx threadIdx, blockIdx;
sim_wave sim_w;

static std::string last_error;
int ta_fail(int code, const char* what) { last_error = what; return code; }
int ta_fail_hip(hipError_t, const char* where) { last_error = where; return -3; }
extern "C" const char* sim_refine_conf_last_error() { return last_error.c_str(); }

#include "../../text_alignment_amd/csrc/ta_refine_conf.hip"

// the entry point this build is for, by name
extern "C" void* sim_refine_post_entry() { return reinterpret_cast<void*>(&ta_posterior_pages); }

#ifdef SIM_REFINE_POST_MAIN
#include <cstdio>
int main() {
    const int nprob = 2, nlines = 2, nslots = 2;
    const double own_m[5] = {0.5, 0.75, 0.0, 0.5, 0.5}, z_m[nslots] = {0.75, 0.5};
    const int32_t own_x[5] = {-3, -4, 0, -1, -1}, z_x[nslots] = {-3, -1};
    const int64_t lab_off[nslots] = {0, 3}, count[2] = {2, 5};
    const int32_t L[nslots] = {3, 2}, post_status[nslots] = {TA_FORCED_OK, TA_FORCED_QUERY};
    int32_t table[nlines * TA_HARVEST_FIELDS] = {0};
    table[1] = 1; table[2] = 3;                          // line 0 keeps characters 1 .. 3 of page 0
    table[TA_HARVEST_FIELDS + 1] = 0; table[TA_HARVEST_FIELDS + 2] = 2;
    const int64_t line_first[nprob + 1] = {0, 1, 2}, t_off[nprob + 1] = {0, 5, 8}, syl_off[nprob + 1] = {0, 2, 3};
    const int32_t refined[nlines] = {1, 1}, slot[nlines] = {0, 1};
    const int32_t syl_first[3] = {0, 1, 0}, syl_last[3] = {0, 4, 2};
    double char_post[8], syl_post[3];
    for (double& v : char_post) v = -5.0;
    for (double& v : syl_post) v = -5.0;
    int32_t status[nprob] = {-5, -5};
    const int rc = ta_posterior_pages(own_m, own_x, z_m, z_x, lab_off, L, count, post_status, nslots, 5, table, line_first,
                                      refined, slot, nlines, t_off, 8, syl_first, syl_last, syl_off, 3, nprob, char_post,
                                      syl_post, status, nullptr);
    bool ok = rc == 0 && status[0] == TA_CONF_PAGES_OK && status[1] == TA_CONF_PAGES_STATUS;
    ok = ok && char_post[0] != char_post[0] && char_post[1] == 0.5 / 0.75 && char_post[2] == 0.5 && char_post[3] == 0.0 &&
         char_post[4] != char_post[4] && syl_post[0] != syl_post[0] && syl_post[1] == 0.0;
    for (int i = 5; i < 8; ++i) ok = ok && char_post[i] == -5.0;
    ok = ok && syl_post[2] == -5.0;
    if (!ok) {
        std::printf("rc %d, status %d %d, %g %g %g\n", rc, status[0], status[1], char_post[1], char_post[2], char_post[3]);
        return 1;
    }
    std::printf("posteriors %.4f %.4f %.4f\n", char_post[1], char_post[2], char_post[3]);
    return 0;
}
#endif
