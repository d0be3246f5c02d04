// tests/native/sim_forced_omit_conf.cpp -- host build of the confidence kernel on the lattice with omission (TEST ONLY).
//
// Compiles text_alignment_amd/csrc/ta_forced_omit_conf.hip ITSELF -- not a restatement -- against tests/native/hipshim (a
// wave is 64 coroutines that meet at every wave-wide operation), sim_forced_shim.h and sim_forced_omit_conf_shim.h (the DPP
// controls of both max-scans and of the moves from either neighbour, and the lane read that joins the suffix scan's rows).
// The library this makes exports the same ta_forced_omit_confidence_workspace_bytes / ta_forced_omit_confidence, taking
// host pointers where the real ones take device pointers, so both fills, the kept rows, the query cursor, the combine and
// every bounds check are run against tests/forced_omit_conf_ref.py without a GPU.
// With SIM_FORCED_OMIT_CONF_MAIN it is a stand-alone program (one small call, exit status 0 if every line came back
// TA_FORCED_OK) that a host sanitizer can be put on: g++ -fsanitize=address,undefined -DSIM_FORCED_OMIT_CONF_MAIN ...
// Build: g++ -O2 -std=c++17 -shared -fPIC -I tests/native/hipshim (tests/test_forced_omit_conf_sim.py does it).
#include "sim_forced_omit_conf_shim.h"

#include <string>

sim_idx threadIdx, blockIdx;
sim_wave sim_w;

static std::string last_error;
int ta_fail(int code, const char* what) { last_error = what; return code; }
int ta_fail_hip(hipError_t, const char* where) { last_error = where; return -3; }
extern "C" const char* sim_forced_last_error() { return last_error.c_str(); }

#include "../../text_alignment_amd/csrc/ta_forced_omit_conf.hip"

#ifdef SIM_FORCED_OMIT_CONF_MAIN
#include <cstdio>
int main() {
    // a line per variant K = 2, 2, 4, 8, 16 and 32; queries at both ends, repeated frames, several per character, the
    // first line with all its 2 L, the second with none at all
    const int no = 5, n = 6;
    const int32_t T[n] = {9, 40, 210, 300, 610, 1050}, L[n] = {3, 7, 100, 140, 300, 520};
    const int32_t nq[n] = {6, 0, 100, 7, 60, 200};
    std::vector<int64_t> row_off(n), lab_off(n), ws_off(n), q_off(n);
    int64_t rows = 0, nlab = 0, ws = 0, nqs = 0;
    for (int b = 0; b < n; ++b) {
        row_off[b] = rows; lab_off[b] = nlab; ws_off[b] = ws; q_off[b] = nqs;
        rows += T[b]; nlab += L[b]; nqs += nq[b];
        const int64_t piece = ta_forced_omit_confidence_workspace_bytes(T[b], L[b], nq[b]);
        if (piece < 0) return 2;
        ws += piece;
    }
    std::vector<float> probs(rows * no);
    uint32_t x = 12345;
    for (float& p : probs) { x = x * 1664525u + 1013904223u; p = (float)(x >> 8) / (float)(1u << 24); }
    std::vector<int32_t> labels(nlab), qc(nqs), qf(nqs), rival(nqs), status(n);
    for (int64_t i = 0; i < nlab; ++i) { x = x * 1664525u + 1013904223u; labels[i] = 1 + (int)((x >> 16) % (no - 1)); }
    for (int b = 0; b < n; ++b)
        for (int j = 0; j < nq[b]; ++j) {                // frames spread over the line, the first 0 and the last T - 1
            x = x * 1664525u + 1013904223u;
            qc[q_off[b] + j] = (int)((x >> 16) % (uint32_t)L[b]);
            const int pairs = (nq[b] - 1) / 2 > 1 ? (nq[b] - 1) / 2 : 1;           // two queries per frame
            qf[q_off[b] + j] = (int)((int64_t)(j / 2) * (T[b] - 1) / pairs);
        }
    std::vector<int64_t> conf(nqs);
    std::vector<unsigned char> work(ws + 16);
    unsigned char* w = work.data() + ((16 - (reinterpret_cast<uintptr_t>(work.data()) & 15)) & 15);
    const int rc = ta_forced_omit_confidence(probs.data(), row_off.data(), T, labels.data(), lab_off.data(), L, ws_off.data(),
                                             qc.data(), qf.data(), q_off.data(), nq, n, no, rows, nlab, nqs, T, L, nq,
                                             4 << 16, w, ws, conf.data(), rival.data(), status.data(), nullptr);
    int bad = rc != 0;
    for (int b = 0; b < n; ++b) bad |= status[b] != 0;
    if (bad) {
        std::printf("rc %d (%s), status", rc, last_error.c_str());
        for (int b = 0; b < n; ++b) std::printf(" %d", status[b]);
        std::printf("\n");
        return 1;
    }
    std::printf("confidence of the first queries %lld %lld %lld\n", (long long)conf[q_off[0]], (long long)conf[q_off[2]],
                (long long)conf[q_off[5]]);
    return 0;
}
#endif
