// tests/native/sim_span.cpp -- host-side lane simulator of the span-locating fill (TEST ONLY).
//
// Replays the data flow of text_alignment_amd/csrc/ta_nw_span.hip on the CPU -- 64 lanes, R rows per lane, skewed
// steps, the wave_shr hand-down of V / D (values WITH origins) between lanes, the single strip-to-strip hand-off row
// that every strip overwrites behind its own reads, the per-lane last-column maximum, the xor-tree wave reduction and
// the combination of the waves' results -- with the SAME nw_span.h the kernel compiles (carrier, cell, free column-0
// boundary, lane step, span_lane_best / span_pick).  Strips run one after the other, which is one of the orders the
// kernel's progress words allow.  Build: g++ -O2 -shared -fPIC (the test does it), or with -DSIM_SPAN_MAIN as a
// stand-alone program for a sanitizer run.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../text_alignment_amd/csrc/nw_span.h"

using namespace ta;

template <int R>
static void run(const int32_t* t, int n, const int32_t* o, int m, const int* p, int W, int32_t* out) {
    using L = PtrLayout<R>;
    if (n <= 0 || m <= 0) { out[0] = 0; out[1] = 0; out[2] = m > 0 ? -m : 0; return; }
    const CellConsts c = make_consts(p[0], p[1], p[2], p[3], p[4], p[5]);
    const SpanConsts k = span_consts(c, p[0], p[1]);
    const auto score = [&](int tt, int oo) -> SpanVal { return tt == oo ? k.cmat : k.cmis; };
    std::vector<SpanVal> hv(m + 2), hd(m + 2);                    // the hand-off row: V~, D of the row above the strip
    for (int j = 0; j <= m; ++j) { hv[j] = span_V_row0(c, j); hd[j] = span_D_row0(c, j); }
    std::vector<SpanBest> wbest(W, span_none());
    const int ngroups = L::ngroups(m);
    for (int s = 0; s < L::nstrips(n); ++s) {
        SpanVal D[kLanes][R], V[kLanes][R], H[kLanes][R], dsave[kLanes];
        int tcode[kLanes][R];
        for (int l = 0; l < kLanes; ++l)
            span_lane_boundary<R>(c, s * L::SR + l * R, D[l], V[l], H[l], dsave[l],
                                  [&](int r, int i) { tcode[l][r] = (i <= n) ? t[i - 1] : -1; });
        for (int g = 0; g < ngroups; ++g) {
            for (int q = 0; q < L::SPG; ++q) {
                const int kk = g * L::SPG + q;
                // cross-lane phase (full EXEC): lane 0 reads the hand-off row, lanes 1 .. 63 the lane above
                SpanVal vup[kLanes], dnext[kLanes];
                const int j0 = (kk + 1 <= m) ? kk + 1 : m;
                for (int l = 0; l < kLanes; ++l) {
                    vup[l] = l ? V[l - 1][R - 1] : hv[j0];
                    dnext[l] = l ? D[l - 1][R - 1] : hd[j0];
                }
                for (int l = 0; l < kLanes; ++l) {
                    const int j = kk - l + 1;
                    // (the kernel's steady groups also run lanes whose rows lie below row n: don't-care values that
                    // reach no valid row; they are run here too, so that the claim is part of what is checked)
                    if (j < 1 || j > m) continue;
                    span_lane_step<R>(score, k, D[l], V[l], H[l], dsave[l], vup[l], dnext[l], tcode[l], o[j - 1]);
                    if (l == kLanes - 1) { hv[j] = V[l][R - 1]; hd[j] = D[l][R - 1]; }
                }
            }
        }
        SpanBest lb[kLanes];
        for (int l = 0; l < kLanes; ++l) {
            const int row0 = s * L::SR + l * R;
            lb[l] = row0 < n ? span_lane_best<R>(c, row0, n, m, D[l]) : span_none();
        }
        for (int off = 32; off >= 1; off >>= 1) {                // __shfl_xor tree: every lane ends with the wave's best
            SpanBest nx[kLanes];
            for (int l = 0; l < kLanes; ++l) nx[l] = span_pick(lb[l], lb[l ^ off]);
            for (int l = 0; l < kLanes; ++l) lb[l] = nx[l];
        }
        for (int l = 1; l < kLanes; ++l)
            if (lb[l].score != lb[0].score || lb[l].i1 != lb[0].i1 || lb[l].origin != lb[0].origin) abort();
        wbest[s % W] = span_pick(wbest[s % W], lb[0]);
    }
    SpanBest b = span_row0(m);
    for (int w = 0; w < W; ++w) b = span_pick(b, wbest[w]);
    out[0] = b.origin; out[1] = b.i1; out[2] = b.score;
}

extern "C" int sim_span(const int32_t* t, int n, const int32_t* o, int m, const int* p, int R, int W, int32_t* out) {
    if (W < 1 || W > 8) return -1;
    if (R == 4) run<4>(t, n, o, m, p, W, out);
    else if (R == 2) run<2>(t, n, o, m, p, W, out);
    else if (R == 1) run<1>(t, n, o, m, p, W, out);
    else return -1;
    return 0;
}
// the carrier's pack / unpack, for the test of its exactness at the ends of both fields
extern "C" int sim_span_roundtrip(int score, int origin, int add, int32_t* out) {
    const SpanVal v = span_val(score, origin) + span_val(add, 0);
    out[0] = span_score(v); out[1] = span_origin(v);
    return 0;
}

#ifdef SIM_SPAN_MAIN
// stand-alone run for -fsanitize=address,undefined: random problems, both scoring kinds, every R and W
int main() {
    unsigned x = 12345;
    auto rnd = [&](int mod) { x = x * 1664525u + 1013904223u; return (int)((x >> 8) % (unsigned)mod); };
    const int systems[2][6] = {{8, -4, -7, -7, -3, 0}, {3, -2, 1, -1, 0, -2}};
    long long sum = 0;
    for (int it = 0; it < 60; ++it) {
        const int n = rnd(700), m = rnd(300);
        std::vector<int32_t> t(n + 1), o(m + 1);
        for (auto& v : t) v = rnd(4);
        for (auto& v : o) v = rnd(4);
        int32_t out[3];
        const int R = 1 << rnd(3);
        if (sim_span(t.data(), n, o.data(), m, systems[it & 1], R, 1 + rnd(8), out)) return 1;
        sum += out[0] + out[1] + out[2];
    }
    printf("sim_span ok %lld\n", sum);
    return 0;
}
#endif
