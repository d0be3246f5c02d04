// tests/native/sim_nw_lcs_runs.cpp -- the run schedule of nw_lcs_suffix_kernel's right-edge stores (TEST ONLY).
//
// lcs_next_run (text_alignment_amd/csrc/nw_band.h, the SAME header the kernel compiles) yields the stores as runs; here
// every run is expanded and compared with the schedule's definition, event by event: the walker of
// tests/native/sim_nw_funnel_lcs.cpp's replay (next_event), restated below as it stands there -- strips from the last,
// lanes from 63, one event per (strip, lane) with gh < ngroups, r >= 1 and cnt >= 0, at step r - 1 + cnt / 64.
// Built with -DSIM_MAIN it is a stand-alone program (for -fsanitize=address,undefined): the sweep of the Python test,
// exit status 0 iff every case holds.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../text_alignment_amd/csrc/nw_band.h"

using namespace ta;

namespace {

struct Event { int t, w, b, s, l; };

// the definition: the events in the order next_event hands them out
std::vector<Event> events_by_definition(int n, int m, const int* gh_of) {
    const int nstrips = PtrLayout<4>::nstrips(n), ngroups = PtrLayout<4>::ngroups(m);
    std::vector<Event> ev;
    int ev_s = nstrips - 1, ev_l = 64;
    while (true) {
        if (--ev_l < 0) { ev_l = 63; --ev_s; }
        if (ev_s < 0) break;
        const int gh = gh_of[ev_s];
        const int r = n - 256 * ev_s - 4 * ev_l, cnt = m - 4 * gh + ev_l;
        if (gh >= ngroups) { ev_l = 0; continue; }
        if (r < 1 || cnt < 0) continue;
        ev.push_back(Event{r - 1 + (cnt >> 6), cnt >> 6, cnt & 63, ev_s, ev_l});
    }
    return ev;
}

std::vector<LcsRun> runs_of(int n, int m, const int* gh_of, int* calls) {
    const int ngroups = PtrLayout<4>::ngroups(m);
    std::vector<LcsRun> runs;
    LcsRunCursor c = lcs_run_begin(n);
    while (true) {
        const LcsRun r = lcs_next_run(n, m, ngroups, c, [&](int s) { ++*calls; return gh_of[s]; });
        if (r.count == 0) {
            if (r.t0 != INT32_MAX) runs.push_back(LcsRun{-1, -1, -1, -1, -1, -1});      // (the end must read as "never")
            break;
        }
        runs.push_back(r);
        if (runs.size() > 4096) break;
    }
    return runs;
}

// 0 if the runs, expanded, are the definition's events; a negative code and where[0..2] otherwise
int check(int n, int m, const int* gh_of, int* where) {
    const int nstrips = PtrLayout<4>::nstrips(n);
    const std::vector<Event> ev = events_by_definition(n, m, gh_of);
    int calls = 0;
    const std::vector<LcsRun> runs = runs_of(n, m, gh_of, &calls);
    size_t e = 0;
    std::vector<int> per_strip(nstrips, 0);
    bool sorted_gh = true;
    for (int s = 1; s < nstrips; ++s) sorted_gh &= gh_of[s - 1] <= gh_of[s];
    for (size_t k = 0; k < runs.size(); ++k) {
        const LcsRun& r = runs[k];
        where[0] = (int)k; where[1] = r.s; where[2] = r.l;
        if (r.count < 1 || r.count > 64) return -1;
        if (r.s < 0 || r.s >= nstrips || r.l < 0 || r.l > 63 || r.w < 0 || r.w > 63 || r.b < 0 || r.b > 63) return -2;
        if (r.count > r.b + 1 || r.count > r.l + 1) return -3;          // a run stays in its word and in its strip
        if (++per_strip[r.s] > 2) return -4;
        for (int q = 0; q < r.count; ++q, ++e) {
            if (e >= ev.size()) return -5;
            const Event& d = ev[e];
            if (d.t != r.t0 + 4 * q || d.w != r.w || d.b != r.b - q || d.s != r.s || d.l != r.l - q) return -6;
            // inside a run the definition's own steps are exactly 4 apart; across runs of non-decreasing gh they grow
            if (q > 0 && ev[e].t - ev[e - 1].t != 4) return -7;
            if (q == 0 && e > 0 && sorted_gh && ev[e].t <= ev[e - 1].t) return -8;
        }
    }
    where[0] = (int)e; where[1] = (int)ev.size(); where[2] = calls;
    if (e != ev.size()) return -9;
    if (calls > 2 * nstrips) return -10;                                // the generic code runs a few times per strip, not per event
    return 0;
}

struct Lcg {
    uint64_t x;
    unsigned next() { x = x * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(x >> 33); }
};

// gh per strip, non-decreasing; kind 0: all 0, 1: all past ngroups, 2: random over the whole range and a little past it,
// 3: a funnel-like ramp ending past ngroups, 4: multiples of 16 as the plan's are, 5: close to m / 4 (cnt around 0)
void make_gh(int kind, int nstrips, int ngroups, int m, Lcg& g, std::vector<int>& gh) {
    gh.assign(nstrips, 0);
    for (int s = 0; s < nstrips; ++s) {
        switch (kind) {
            case 0: gh[s] = 0; break;
            case 1: gh[s] = ngroups + (int)(g.next() % 3); break;
            case 2: gh[s] = (int)(g.next() % (unsigned)(ngroups + 3)); break;
            case 3: gh[s] = (int)((int64_t)(ngroups + 2) * (s + 1) / nstrips); break;
            case 4: gh[s] = 16 * (int)(g.next() % (unsigned)(ngroups / 16 + 2)); break;
            default: gh[s] = m / 4 - 8 + (int)(g.next() % 24); if (gh[s] < 0) gh[s] = 0; break;
        }
    }
    for (int s = 1; s < nstrips; ++s)
        if (gh[s] < gh[s - 1]) gh[s] = gh[s - 1];
}

}  // namespace

// the runs of one problem, expanded: out[5 k ..] = (step, lane, bit, strip, l) of the k-th store; the number of stores,
// or -1 if there are more than cap
extern "C" int sim_lcs_runs_expand(int n, int m, const int* gh_of, int* out, int cap) {
    int calls = 0, e = 0;
    for (const LcsRun& r : runs_of(n, m, gh_of, &calls))
        for (int q = 0; q < r.count; ++q, ++e) {
            if (e >= cap) return -1;
            const int v[5] = {r.t0 + 4 * q, r.w, r.b - q, r.s, r.l - q};
            for (int k = 0; k < 5; ++k) out[5 * e + k] = v[k];
        }
    return e;
}

// every n in n_lo .. n_hi against the listed m, each with every kind of gh; the number of cases checked, or a negative
// code with fail[0..5] = n, m, kind, and check's three words
extern "C" int sim_lcs_runs_sweep(int n_lo, int n_hi, const int* ms, int n_ms, unsigned seed, int* fail) {
    Lcg g{seed * 2654435761ull + 1};
    std::vector<int> gh;
    int cases = 0;
    for (int n = n_lo; n <= n_hi; ++n)
        for (int k = 0; k < n_ms; ++k)
            for (int kind = 0; kind < 6; ++kind) {
                const int m = ms[k];
                make_gh(kind, PtrLayout<4>::nstrips(n), PtrLayout<4>::ngroups(m), m, g, gh);
                const int rc = check(n, m, gh.data(), fail + 3);
                if (rc) { fail[0] = n; fail[1] = m; fail[2] = kind; return rc; }
                ++cases;
            }
    return cases;
}

#ifdef SIM_MAIN
#include <cstdio>
int main() {
    std::vector<int> ms = {2, 3, 5, 31, 1100};
    for (int k = 1; 64 * k <= 1088; ++k) { ms.push_back(64 * k - 1); ms.push_back(64 * k); ms.push_back(64 * k + 1); }
    int fail[6] = {0};
    const int rc = sim_lcs_runs_sweep(2, 1100, ms.data(), (int)ms.size(), 7, fail);
    if (rc < 0) printf("BAD: code %d at n %d m %d kind %d (%d %d %d)\n", rc, fail[0], fail[1], fail[2], fail[3], fail[4], fail[5]);
    else printf("%d cases ok\n", rc);
    return rc < 0 ? 1 : 0;
}
#endif
