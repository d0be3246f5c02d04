// tests/native/main_forced_omit_lines.cpp -- stand-alone host program over the omission pipeline's aligner entry (TEST ONLY).
//
// sim_forced_omit.cpp (the host build of text_alignment_amd/csrc/ta_forced_omit.hip) with a main of its own that calls
// ta_forced_align_omit_lines the way forced.Refining does: a chunk of five lines, two of them holes, three packed slots
// in permuted order, one slot behind count, caps at and above L.  Exit status 0 if every filled slot came back
// TA_FORCED_OK with every first field a frame or TA_FORCED_OMITTED and the slot behind count was left alone.  It is the
// program a host sanitizer can be put on (nothing is loaded into Python):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I tests/native/hipshim tests/native/main_forced_omit_lines.cpp
#include "sim_forced_omit.cpp"

#include <cstdio>

int main() {
    const int no = 5, nlines_all = 5, nslots = 4;
    const int32_t T_all[nlines_all] = {300, 1, 9, 1, 40}, Lcap[nlines_all] = {149, 0, 3, 0, 12};
    const int32_t acc_line[nslots] = {4, 0, 2, 0x7ffffff0}, L[nslots] = {7, 140, 3, 5};
    const int64_t lab_off[nslots] = {2, 11, 153, int64_t(1) << 40}, count[2] = {3, 150};
    const int64_t label_cap = 160;
    std::vector<int64_t> row_off(nlines_all), ws_off(nlines_all);
    int64_t rows = 0, ws = 0;
    for (int q = 0; q < nlines_all; ++q) {
        row_off[q] = rows; ws_off[q] = ws;
        rows += T_all[q];
        if (Lcap[q] > 0) ws += ta_forced_omit_workspace_bytes(T_all[q], Lcap[q]);
    }
    std::vector<float> probs(rows * no);
    uint32_t x = 12345;
    for (float& p : probs) { x = x * 1664525u + 1013904223u; p = (float)(x >> 8) / (float)(1u << 24); }
    std::vector<int32_t> labels(label_cap);
    for (int64_t i = 0; i < label_cap; ++i) { x = x * 1664525u + 1013904223u; labels[i] = 1 + (int)((x >> 16) % (no - 1)); }
    std::vector<unsigned char> work(ws + 16);
    unsigned char* w = work.data() + ((16 - (reinterpret_cast<uintptr_t>(work.data()) & 15)) & 15);
    for (int omit : {0, 3 << 16, 1 << 26}) {
        std::vector<int32_t> frames(3 * label_cap, -77), status(nslots, -77);
        std::vector<int64_t> score(nslots, -77);
        const int rc = ta_forced_align_omit_lines(probs.data(), row_off.data(), T_all, ws_off.data(), Lcap, acc_line, L, lab_off,
                                                  labels.data(), count, nlines_all, nslots, no, rows, label_cap, T_all, Lcap, omit,
                                                  w, ws, frames.data(), score.data(), status.data(), nullptr);
        bool ok = rc == 0 && status[3] == -77 && score[3] == -77;
        for (int k = 0; k < 3 && ok; ++k) {
            ok = status[k] == TA_FORCED_OK;
            for (int i = 0; i < L[k] && ok; ++i) {
                const int32_t tf = frames[3 * (lab_off[k] + i)];
                ok = tf == TA_FORCED_OMITTED || (tf >= 0 && tf < T_all[acc_line[k]]);
            }
        }
        if (!ok) {
            std::printf("omit %d: rc %d (%s), status %d %d %d %d\n", omit, rc, sim_forced_last_error(), status[0], status[1],
                        status[2], status[3]);
            return 1;
        }
        std::printf("omit %d: scores %lld %lld %lld\n", omit, (long long)score[0], (long long)score[1], (long long)score[2]);
    }
    return 0;
}
