// tests/native/sim_span_chain.cpp -- host-side simulator of the CHAINED span search (TEST ONLY).
//
// Replays ta_nw_span_chain (text_alignment_amd/csrc/ta_nw_span.hip) on the CPU with the SAME nw_span.h the kernels compile:
// per page the fill of tests/native/sim_span.cpp -- 64 lanes, R rows per lane, skewed steps, the hand-off row -- with the
// chained boundary (span_lane_boundary_chain, the row-0 values with the carry) and the store of every row's last-column
// value and origin (span_store_last / span_trivial_last); then the carry kernel's tiles (span_carry_load, an inclusive
// maximum scan over the lanes of a wave, the waves' totals, the running value, span_carry_store) and the walk back
// (span_walk_lane per lane, span_walk_pick in the order of the kernel's xor tree and of its waves, span_walk_result).
// Build: g++ -O2 -shared -fPIC (the test does it), or with -DSIM_SPAN_CHAIN_MAIN as a stand-alone program for a
// sanitizer run.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../text_alignment_amd/csrc/nw_span.h"

using namespace ta;

constexpr int kMaxThreads = 512;
static int kThreads = 256;                                       // the carry's and the walk's workgroup: 64 W lanes (the
                                                                 // kernels launch W = 4; no result may depend on it)

template <int R>
static void fill(const int32_t* t, int n, const int32_t* o, int m, const int* p, const int32_t* G, int32_t* F, int32_t* O) {
    using L = PtrLayout<R>;
    if (n <= 0 || m <= 0) {
        for (int i = 0; i <= (m <= 0 ? n : 0); ++i) span_trivial_last(i, m > 0 ? m : 0, G ? G[i + kSpanChainPad] : 0, F, O);
        return;
    }
    const CellConsts c = make_consts(p[0], p[1], p[2], p[3], p[4], p[5]);
    const SpanConsts k = span_consts(c, p[0], p[1]);
    const auto score = [&](int tt, int oo) -> SpanVal { return tt == oo ? k.cmat : k.cmis; };
    const int g0 = G ? G[kSpanChainPad] : 0;
    std::vector<SpanVal> hv(m + 2), hd(m + 2);
    for (int j = 0; j <= m; ++j) { hv[j] = span_V_row0(c, j, g0); hd[j] = span_D_row0(c, j, g0); }
    span_trivial_last(0, m, g0, F, O);
    const int ngroups = L::ngroups(m);
    for (int s = 0; s < L::nstrips(n); ++s) {
        SpanVal D[kLanes][R], V[kLanes][R], H[kLanes][R], dsave[kLanes];
        int tcode[kLanes][R];
        for (int l = 0; l < kLanes; ++l)
            span_lane_boundary_chain<R>(c, s * L::SR + l * R, D[l], V[l], H[l], dsave[l],
                                        [&](int i) { return (G && i <= n) ? G[i + kSpanChainPad] : 0; },
                                        [&](int r, int i) { tcode[l][r] = (i <= n) ? t[i - 1] : -1; });
        for (int g = 0; g < ngroups; ++g) {
            for (int q = 0; q < L::SPG; ++q) {
                const int kk = g * L::SPG + q;
                SpanVal vup[kLanes], dnext[kLanes];
                const int j0 = (kk + 1 <= m) ? kk + 1 : m;
                for (int l = 0; l < kLanes; ++l) {
                    vup[l] = l ? V[l - 1][R - 1] : hv[j0];
                    dnext[l] = l ? D[l - 1][R - 1] : hd[j0];
                }
                for (int l = 0; l < kLanes; ++l) {
                    const int j = kk - l + 1;
                    if (j < 1 || j > m) continue;
                    span_lane_step<R>(score, k, D[l], V[l], H[l], dsave[l], vup[l], dnext[l], tcode[l], o[j - 1]);
                    if (l == kLanes - 1) { hv[j] = V[l][R - 1]; hd[j] = D[l][R - 1]; }
                }
            }
        }
        for (int l = 0; l < kLanes; ++l) {
            const int row0 = s * L::SR + l * R;
            if (row0 < n) span_store_last<R>(c, row0, n, m, D[l], F, O);
        }
    }
}

static void carry(const int32_t* F, int32_t* G, int n, int floor) {
    int top = kSpanNone;
    for (int i = 0; i <= n; ++i) top = span_imax(top, F[i + kSpanChainPad]);
    int running = kSpanNone;
    for (int base = 0; base <= n; base += kThreads * kSpanCarryPer) {
        int v[kMaxThreads][kSpanCarryPer], incl[kMaxThreads], wave_max[kMaxThreads / 64];
        for (int tid = 0; tid < kThreads; ++tid) {
            const int mine = span_carry_load(F, base + tid * kSpanCarryPer, n, v[tid]);
            incl[tid] = (tid & 63) ? span_imax(incl[tid - 1], mine) : mine;       // the wave's inclusive scan
            if ((tid & 63) == 63) wave_max[tid >> 6] = incl[tid];
        }
        int tile = kSpanNone;
        for (int tid = 0; tid < kThreads; ++tid) {
            int before = (tid & 63) ? incl[tid - 1] : kSpanNone;
            for (int w = 0; w < (tid >> 6); ++w) before = span_imax(before, wave_max[w]);
            span_carry_store(G, base + tid * kSpanCarryPer, n, v[tid], span_imax(before, running), top, floor);
        }
        for (int w = 0; w < kThreads / 64; ++w) tile = span_imax(tile, wave_max[w]);
        running = span_imax(running, tile);
    }
}

static void walk_page(const int32_t* F, const int32_t* O, const int32_t* Gprev, int limit, int32_t* out3) {
    SpanWalk w[kMaxThreads];
    for (int tid = 0; tid < kThreads; ++tid) w[tid] = span_walk_lane(F, limit, tid, kThreads);
    for (int off = 32; off >= 1; off >>= 1) {                     // the xor tree inside each wave
        SpanWalk nx[kMaxThreads];
        for (int tid = 0; tid < kThreads; ++tid) nx[tid] = span_walk_pick(w[tid], w[tid ^ off]);
        for (int tid = 0; tid < kThreads; ++tid) w[tid] = nx[tid];
    }
    SpanWalk b = span_walk_none();
    for (int x = 0; x < kThreads / 64; ++x) b = span_walk_pick(b, w[x * 64]);
    span_walk_result(b, O, Gprev, out3);
}

// t[n]; the pages' codes o[o_off[p] .. o_off[p+1]); out[npages][3], total[1].  R = rows per lane of the fill, W = waves
// of the carry's and the walk's workgroup (the fill keeps no per-wave state in a chain: its strips run in order).
extern "C" int sim_span_chain(const int32_t* t, int n, const int32_t* o, const int64_t* o_off, int npages, const int* p,
                              int floor, int R, int W, int32_t* out, int64_t* total) {
    if (npages < 0 || n < 0 || floor <= 0 || (R != 1 && R != 2 && R != 4) || W < 1 || W > 8) return -1;
    kThreads = 64 * W;
    const int64_t stride = span_chain_stride(n);
    std::vector<int32_t> F((size_t)npages * stride + 4, -7777), O(F), G(F);
    const CellConsts c = make_consts(p[0], p[1], p[2], p[3], p[4], p[5]);
    if (!span_consts_fit(span_consts(c, p[0], p[1]))) return -2;
    for (int pg = 0; pg < npages; ++pg) {
        const int m = (int)(o_off[pg + 1] - o_off[pg]);
        const int32_t* Gp = pg ? G.data() + (pg - 1) * stride : nullptr;
        int32_t *Fp = F.data() + pg * stride, *Op = O.data() + pg * stride;
        if (R == 4) fill<4>(t, n, o + o_off[pg], m, p, Gp, Fp, Op);
        else if (R == 2) fill<2>(t, n, o + o_off[pg], m, p, Gp, Fp, Op);
        else fill<1>(t, n, o + o_off[pg], m, p, Gp, Fp, Op);
        if (pg + 1 < npages) carry(Fp, G.data() + pg * stride, n, floor);
    }
    int limit = n;
    int64_t sum = 0;
    for (int pg = npages - 1; pg >= 0; --pg) {
        walk_page(F.data() + pg * stride, O.data() + pg * stride, pg ? G.data() + (pg - 1) * stride : nullptr, limit,
                  out + 3 * pg);
        sum += out[3 * pg + 2];
        limit = out[3 * pg];
    }
    *total = sum;
    return 0;
}

#ifdef SIM_SPAN_CHAIN_MAIN
// stand-alone run for -fsanitize=address,undefined: random chains, both scoring kinds, every R
int main() {
    unsigned x = 4321;
    auto rnd = [&](int mod) { x = x * 1664525u + 1013904223u; return (int)((x >> 8) % (unsigned)mod); };
    const int systems[2][6] = {{8, -4, -7, -7, -3, 0}, {3, -2, 1, -1, 0, -2}};
    long long sum = 0;
    for (int it = 0; it < 40; ++it) {
        const int n = rnd(1400), npages = 1 + rnd(4);
        std::vector<int32_t> t(n + 1), o;
        std::vector<int64_t> off(1, 0);
        for (auto& v : t) v = rnd(4);
        for (int pg = 0; pg < npages; ++pg) {
            const int m = rnd(3) ? rnd(200) : 0;
            for (int j = 0; j < m; ++j) o.push_back(rnd(4));
            off.push_back((int64_t)o.size());
        }
        o.push_back(0);
        std::vector<int32_t> out(3 * npages);
        int64_t total;
        if (sim_span_chain(t.data(), n, o.data(), off.data(), npages, systems[it & 1], it % 3 ? 4000 : 5, 1 << rnd(3),
                           1 + rnd(8), out.data(), &total)) return 1;
        sum += total;
    }
    printf("sim_span_chain ok %lld\n", sum);
    return 0;
}
#endif
