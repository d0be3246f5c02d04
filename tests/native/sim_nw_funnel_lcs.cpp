// tests/native/sim_nw_funnel_lcs.cpp -- host-side replay of the LCS-bounded funnel (TEST ONLY).
//
// 1. nw_lcs_suffix_kernel's data flow (text_alignment_amd/csrc/ta_nw2.hip), lane by lane: one 64-bit word per lane, rows
//    skewed across the lanes, carry / count / symbol handed to the next lane one step later, the stores scheduled as the
//    kernel schedules them, the boundary's share of the exit word gathered as the kernel gathers it.  Every stored value
//    is compared with a plain dynamic-programming table of L(i, j) = LCS(T[i+1..n], O[j+1..m]).
// 2. Phase 1 as nw_score_kernel<.., BAND = 4> runs it under the narrower ranges, with the three edge gatherings taking
//    funnel_suf_lcs and the counts of the table from 1.  The exit word must EQUAL a scan of every cell of the region and
//    the boundary for neighbours outside it, each border cell under the count the kernel's design gives it (below) but
//    taken from the plain table: that proves the list of edge cells complete and the table's addressing right.
// Phase 2 is not replayed here: it is the static funnel's, whose replay (sim_nw_funnel.cpp) covers any ranges that
// pass funnel_ok.  Uses the SAME nw_band.h / nw_cell.h as the kernel.
// Built with -DSIM_MAIN it is a stand-alone program (for -fsanitize=address,undefined): a few shapes and systems,
// exit status 0 iff every check holds.
#include "sim_nw.cpp"

#include "../../text_alignment_amd/csrc/nw_band.h"

namespace {

struct LcsTable {                       // L[i][j], 0 <= i <= n, 0 <= j <= m
    int n, m;
    std::vector<int> v;
    int at(int i, int j) const { return v[(size_t)i * (m + 1) + j]; }
};
LcsTable lcs_dp(const int32_t* t, int n, const int32_t* o, int m, int alphabet) {
    LcsTable L{n, m, std::vector<int>((size_t)(n + 1) * (m + 1), 0)};
    for (int i = n - 1; i >= 0; --i)
        for (int j = m - 1; j >= 0; --j) {
            const bool eq = t[i] == o[j] && (unsigned)t[i] < (unsigned)alphabet;   // T[i+1] against O[j+1]
            int best = std::max(L.at(i + 1, j), L.at(i, j + 1));
            if (eq) best = std::max(best, L.at(i + 1, j + 1) + 1);
            L.v[(size_t)i * (m + 1) + j] = best;
        }
    return L;
}

// the kernel, step by step; table[lcs_stride(n)] as it leaves it, *ex_out the boundary's share of the exit word
int lcs_kernel_replay(const int32_t* t, int n, const int32_t* o, int m, const int* prm, int band_w, int alphabet,
                      int32_t* table, int* ex_out) {
    const FunnelSys fsys = funnel_sys(prm);
    const FunnelLcs lsys = funnel_lcs_sys(prm);
    const int nstrips = PtrLayout<4>::nstrips(n), ngroups = PtrLayout<4>::ngroups(m);
    std::vector<uint64_t> mask((size_t)(alphabet + 1) * 64, 0);
    std::vector<BandRange> rg(nstrips);
    int32_t* const out = table;
    int32_t* const rows = table + lcs_row_off(n);
    for (int lane = 0; lane < 64; ++lane)
        for (int b = 0; b < 64; ++b) {
            const int c = 64 * lane + b;
            const int sym = c < m ? o[m - 1 - c] : -1;
            if ((unsigned)sym < (unsigned)alphabet) mask[(size_t)sym * 64 + lane] |= 1ull << b;
        }
    for (int s = 0; s < nstrips; ++s) rg[s] = funnel_raw<kFunnelLcsScalePm>(n, m, fsys, band_w, s);
    for (int k = 0; k < 64 * nstrips; ++k) out[k] = 0;
    auto is_out = [&](int i, int j) {
        if (i < 1 || i > n || j < 1 || j > m) return false;
        const BandRange& r = rg[(i - 1) / 256];
        return j < funnel_jlo(r, i) || j > funnel_jhi(r, i, m);
    };
    auto exit0 = [&](int db, int i2, int j2, int l) { return db + fsys.ap + funnel_suf_lcs<int>(n - i2, m - j2, l, fsys, lsys); };
    int ev_s = nstrips - 1, ev_l = 64, ev_t = -1, ev_w = 0, ev_b = 0;
    auto next_event = [&]() {
        while (true) {
            if (--ev_l < 0) { ev_l = 63; --ev_s; }
            if (ev_s < 0) { ev_t = -1; return; }
            const int gh = rg[ev_s].gh;
            const int r = n - 256 * ev_s - 4 * ev_l, cnt = m - 4 * gh + ev_l;
            if (gh >= ngroups) { ev_l = 0; continue; }
            if (r < 1 || cnt < 0) continue;
            ev_w = cnt >> 6; ev_b = cnt & 63; ev_t = r - 1 + ev_w;
            return;
        }
    };
    next_event();
    const int pad = alphabet;
    uint64_t V[64];
    int cy[64], pc[64], sym[64], ex[64];
    for (int l = 0; l < 64; ++l) { V[l] = ~0ull; cy[l] = 0; pc[l] = 0; sym[l] = pad; ex[l] = -(1 << 30); }
    const int nchunks = (n + 63 + 63) / 64;
    int last_t = -1;
    for (int ch = 0; ch < nchunks; ++ch) {
        const int base = ch * 64;
        int feed[64];
        for (int lane = 0; lane < 64; ++lane) {
            const int tk = n - 1 - base - lane;
            feed[lane] = pad;
            if (tk >= 0) { const int c = t[tk]; feed[lane] = (unsigned)c < (unsigned)alphabet ? c : pad; }
        }
        const int i_row = (int)((unsigned)((n - base - 1) >> 8) << 8);
        const int row_t0 = n - i_row - 1;
        for (int q = 0; q < 64; ++q) {
            const int tt = base + q;
            int cin[64], pin[64], nsym[64];
            for (int l = 0; l < 64; ++l) {          // the DPP shift: lane 0 keeps `old`
                cin[l] = l ? cy[l - 1] : 0;
                pin[l] = l ? pc[l - 1] : 0;
                nsym[l] = l ? sym[l - 1] : feed[q];
            }
            for (int l = 0; l < 64; ++l) {
                sym[l] = nsym[l];
                const uint64_t M = mask[(size_t)sym[l] * 64 + l];
                const uint64_t U = V[l] & M;
                const uint64_t s1 = V[l] + U;
                const uint64_t s2 = s1 + (uint64_t)(unsigned)cin[l];
                cy[l] = (int)(s1 < V[l]) | (int)(s2 < s1);
                V[l] = s2 | (V[l] & ~M);
                pc[l] = pin[l] + __builtin_popcountll(~V[l]);
            }
            if (tt == ev_t) {
                if (tt <= last_t) return -50;      // one event per step, in step order
                last_t = tt;
                out[64 * ev_s + ev_l] = pin[ev_w] + __builtin_popcountll(~V[ev_w] & ((1ull << ev_b) - 1));
                next_event();
            }
            for (int k = 0; k < 2; ++k) {
                const int d = tt - (row_t0 - 256 * k);
                const int i = i_row + 256 * k;
                if (d >= 0 && d < 64 && i < n && i >= 0) {
                    int32_t* const row = rows + 192 * (i >> 8);
                    reinterpret_cast<uint64_t*>(row)[d] = ~V[d];
                    row[128 + d] = pin[d];
                }
            }
        }
        const int ltot = pc[63];
        for (int lane = 0; lane < 64; ++lane) {
            const int r = base + 1 - lane, i = n - r;
            if (r >= 0 && r <= n) {
                if (is_out(i, 1)) ex[lane] = std::max(ex[lane], exit0(-i, i, 1, ltot));
                if (is_out(i + 1, 1)) ex[lane] = std::max(ex[lane], exit0(-i, i + 1, 1, ltot));
            }
        }
    }
    if (ev_t != -1) return -51;                     // an event the steps never reached
    int best = -(1 << 30);
    for (int lane = 0; lane < 64; ++lane) {
        const int before = pc[lane] - __builtin_popcountll(~V[lane]);
        for (int b = 0; b < 64; ++b) {
            const int cnt = 64 * lane + b, j = m - cnt;
            if (j < 0) break;
            const int l = before + (b ? __builtin_popcountll(~V[lane] & ((1ull << b) - 1)) : 0);
            if (is_out(1, j)) ex[lane] = std::max(ex[lane], exit0(-j, 1, j, l));
            if (is_out(1, j + 1)) ex[lane] = std::max(ex[lane], exit0(-j, 1, j + 1, l));
        }
        best = std::max(best, ex[lane]);
    }
    *ex_out = best;
    return 0;
}

}  // namespace

// info[0] = 1 if the certificate passes; [1] = v0; [2] = U(band_w); [3] = the exit word as the kernels gather it;
// [4] = strips counted; [5] = the exit bound by the scan of all cells; [6] = the boundary's share (LCS kernel);
// [7] = the flag word (2: covered, 1 / 0: the static funnel's business -- nothing else is filled in);
// [8] = 1 if every word of the table equals the plain DP's; [9] = the same scan under the static Suf (for comparison).
// table_out[lcs_stride(n)]: the LCS kernel's table; ranges_out[2 nstrips].
extern "C" int sim_nw2_funnel_lcs(const int32_t* t, int n, const int32_t* o, int m, const int* p, int band_w,
                                  int alphabet, int* info, int32_t* table_out, int* ranges_out) {
    constexpr int R = 4;
    using L = PtrLayout<R>;
    constexpr int SPG = L::SPG;
    for (int k = 0; k < 10; ++k) info[k] = 0;
    if (n < 2 || m < 1 || band_w < 2) return -1;
    const CellConsts c = make_consts(p[0], p[1], p[2], p[3], p[4], p[5]);
    const int cmat_raw = p[0] - p[4] - p[5], cmis_raw = p[1] - p[4] - p[5];
    const int nstrips = L::nstrips(n), ngroups = L::ngroups(m);
    const bool carried = opens_nonpositive(c.gox, c.goy);
    if (!carried) return -2;
    const int yadj = c.goy, xadj = c.gox;
    const FunnelSys fs = funnel_sys(p);
    const FunnelLcs ls = funnel_lcs_sys(p);
    // nw_band_cert_init_lcs_kernel's decision
    const bool lcs = m <= kLcsMaxM && alphabet > 0 && alphabet <= kLcsMaxAlphabet && p[0] > p[1] &&
                     funnel_ok<kFunnelLcsScalePm>(n, m, fs, band_w);
    info[7] = lcs ? 2 : funnel_ok(n, m, fs, band_w) ? 1 : 0;
    if (!lcs) return 0;
    std::vector<BandRange> rg(nstrips);
    for (int s = 0; s < nstrips; ++s) {
        rg[s] = funnel_raw<kFunnelLcsScalePm>(n, m, fs, band_w, s);
        if (ranges_out) { ranges_out[2 * s] = rg[s].gl; ranges_out[2 * s + 1] = rg[s].gh; }
        if (s > 0 && (rg[s].gl < rg[s - 1].gl || rg[s].gh < rg[s - 1].gh)) return -41;
    }
    std::vector<int32_t> table((size_t)lcs_stride(n), -7);
    int ex_lcs = 0;
    const int rc = lcs_kernel_replay(t, n, o, m, p, band_w, alphabet, table.data(), &ex_lcs);
    if (rc) return rc;
    if (table_out) memcpy(table_out, table.data(), table.size() * sizeof(int32_t));
    const int32_t* const edge = table.data();
    const int32_t* const rows = table.data() + lcs_row_off(n);

    // the table against the plain DP
    const LcsTable Lx = lcs_dp(t, n, o, m, alphabet);
    bool table_ok = true;
    for (int s = 0; s < nstrips; ++s) {
        for (int j = 0; j <= m; ++j) table_ok &= lcs_row_at(rows + 192 * s, m, j) == Lx.at(256 * s, j);
        for (int l = 0; l < 64; ++l) {
            const int row0 = 256 * s + 4 * l, jr = 4 * rg[s].gh - l;
            int want = 0;
            if (rg[s].gh < ngroups && row0 < n && jr <= m) want = Lx.at(row0, jr);
            table_ok &= edge[64 * s + l] == want;
        }
    }
    info[8] = table_ok;

    const auto unhat = [&](int v, int i, int j) { return v + p[4] * i + p[5] * j; };
    const auto sufl = [&](int i, int j, int l) { return funnel_suf_lcs<int64_t>(n - i, m - j, l, fs, ls); };
    int64_t exit_k = ex_lcs;
    int count = 0, v0 = INT32_MIN;
    std::vector<int> Dall((size_t)(n + 1) * (m + 1), 0);
    std::vector<int> HV((size_t)(nstrips + 1) * (m + 2)), HD(HV.size());
    for (int j = 0; j <= m; ++j) { HV[j] = raw_of(bnd_V_row0(c, j)) + xadj; HD[j] = raw_of(bnd_D_row0(c, j)); }
    for (int s = 0; s < nstrips; ++s) {
        const int* hv = &HV[(size_t)s * (m + 2)];
        const int* hd = &HD[(size_t)s * (m + 2)];
        int* hv_out = &HV[(size_t)(s + 1) * (m + 2)];
        int* hd_out = &HD[(size_t)(s + 1) * (m + 2)];
        int D[kLanes][R], V[kLanes][R], H[kLanes][R], tcode[kLanes][R], dsave[kLanes];
        strip_setup<false>(c, s, t, n, yadj, D, V, H, tcode, dsave);
        const BandRange br = rg[s];
        const int i0 = s * L::SR + 1;
        if (br.gl % 16 || (br.gh % 16 && br.gh != ngroups) || br.gl >= br.gh || br.gh > ngroups) return -30;
        if (br.gl > 0) {
            for (int l = 0; l < kLanes; ++l) {
                for (int r = 0; r < R; ++r) D[l][r] = H[l][r] = V[l][r] = kBandSentinel;
                dsave[l] = kBandSentinel;
            }
            const int c_lo = rg[s - 1].gl == 0 ? 1 : rg[s - 1].gl * SPG - 60, c_hi = std::min(m, br.gl * SPG + 2);
            const int32_t* lrow = rows + 192 * s;
            for (int j = c_lo; j <= c_hi; ++j) {
                const int64_t db = unhat(hd[j], i0 - 1, j);
                const int l = lcs_row_at(lrow, m, j);
                exit_k = std::max(exit_k, db + fs.ap + sufl(i0, j, l));
                if (j + 1 <= c_hi) exit_k = std::max(exit_k, db + fs.ap + sufl(i0, j + 1, l));
            }
        }
        const int cert_lane = ((n - 1) % L::SR) / R, cert_r = (n - 1) % R;
        const auto cell = [&](int d_ul, int v_u, int h_l, int tt, int oo, int& d, int& v, int& h) {
            const int cs = (tt == oo) ? cmat_raw : cmis_raw;
            cell_update_carried(d_ul, v_u, h_l, cs, c.gox, c.goy, d, v, h);
        };
        for (int g = br.gl; g < br.gh; ++g)
            for (int q = 0; q < SPG; ++q) {
                const int k = g * SPG + q;
                int vup[kLanes], dnext[kLanes];
                const int j0 = (k + 1 <= m) ? k + 1 : 0;
                shift_down<R>(0, kLanes, V, D, hv[j0], hd[j0], vup, dnext);
                for (int l = 0; l < kLanes; ++l) {
                    const int j = k - l + 1;
                    if (j < 1 || j > m) continue;
                    const bool cert_here = s == nstrips - 1 && l == cert_lane && j == m;
                    const int cert_m = (cert_r == 0 ? dsave[l] : D[l][cert_r - 1]) + ((tcode[l][cert_r] == o[m - 1]) ? cmat_raw : cmis_raw);
                    const int cert_y = H[l][cert_r];
                    lane_step(cell, D[l], V[l], H[l], dsave[l], vup[l], dnext[l], tcode[l], o[j - 1]);
                    if (cert_here)
                        v0 = std::min(cert_m, std::min(cert_r == 0 ? vup[l] : V[l][cert_r - 1], cert_y)) + p[4] * n + p[5] * m;
                    if (l == kLanes - 1) { hv_out[j] = V[l][R - 1]; hd_out[j] = D[l][R - 1]; }
                    for (int r = 0; r < R; ++r)
                        if (i0 + l * R + r <= n) Dall[(size_t)(i0 + l * R + r) * (m + 1) + j] = unhat(D[l][r], i0 + l * R + r, j);
                }
            }
        if (br.gh < ngroups) {
            for (int l = 0; l < kLanes; ++l) {
                const int jr = br.gh * SPG - l, row0 = i0 - 1 + l * R;
                if (jr < 1) return -35;
                const int lc = jr <= m && row0 < n ? edge[64 * s + l] : kBandMaxLen;
                if (jr <= m)
                    for (int r = 0; r < R; ++r) {
                        const int i = row0 + 1 + r;
                        if (i > n) continue;
                        const int64_t db = unhat(D[l][r], i, jr);
                        if (jr + 1 <= m) exit_k = std::max(exit_k, db + fs.ap + sufl(i, jr + 1, lc));
                        const bool diag_in = l == kLanes - 1 && r == R - 1 && s + 1 < nstrips &&
                                             jr + 1 >= (rg[s + 1].gl == 0 ? 1 : rg[s + 1].gl * SPG + 3) && jr + 1 <= std::min(m, rg[s + 1].gh * SPG);
                        if (jr + 1 <= m && i + 1 <= n && !diag_in) exit_k = std::max(exit_k, db + fs.ap + sufl(i + 1, jr + 1, lc));
                        if (r == R - 1 && l < kLanes - 1 && i + 1 <= n) exit_k = std::max(exit_k, db + fs.ap + sufl(i + 1, jr, lc));
                    }
                if (jr + 1 <= m && row0 + 1 <= n)
                    exit_k = std::max(exit_k, (int64_t)unhat(dsave[l], row0, jr) + fs.ap + sufl(row0 + 1, jr + 1, lc));
            }
            if (s + 1 >= nstrips) return -31;
            const int c_hi = std::min(m, rg[s + 1].gh * SPG + 4);
            for (int col = br.gh * SPG - 62; col <= c_hi; ++col) hv_out[col] = hd_out[col] = kBandSentinel;
        }
        ++count;
    }

    // The scan.  Counts from the plain table, per border cell c = (i, j) as the kernels' design assigns them:
    //   column 0: the count of the whole suffix of the block's tallest row -- rows are taken in blocks r = n - i in
    //             (64 k - 63 .. 64 k + 1], under L(n - min(64 k + 1, n), 0);    row 0: L(0, j);
    //   the last column of a row of R (the right edge's cells): L(row0, j), row0 = 4 floor((i - 1) / 4) -- the row above
    //             the lane's four; every other cell: L(i, j) (the left edge's row 256 s; the right edge's dsave cell).
    int64_t exit_scan = -(1ll << 40), exit_static = -(1ll << 40);
    {
        const auto in_r = [&](int i, int j) {
            const BandRange& r = rg[(i - 1) / L::SR];
            return j >= funnel_jlo(r, i) && j <= funnel_jhi(r, i, m);
        };
        for (int i = 0; i <= n; ++i)
            for (int j = 0; j <= m; ++j) {
                const bool bnd = i == 0 || j == 0;
                if (!bnd && !in_r(i, j)) continue;
                const int64_t db = bnd ? -(i + j) : Dall[(size_t)i * (m + 1) + j];
                int l;
                if (i == 0) l = Lx.at(0, j);
                else if (j == 0) {
                    const int r = n - i, k = (r + 62) / 64;          // r in (64 k - 63 .. 64 k + 1]
                    l = Lx.at(n - std::min(64 * k + 1, n), 0);
                } else if (j == funnel_jhi(rg[(i - 1) / L::SR], i, m)) l = Lx.at(4 * ((i - 1) / 4), j);
                else l = Lx.at(i, j);
                const int ni[3] = {i, i + 1, i + 1}, nj[3] = {j + 1, j, j + 1};
                for (int q = 0; q < 3; ++q) {
                    if (ni[q] < 1 || ni[q] > n || nj[q] < 1 || nj[q] > m || in_r(ni[q], nj[q])) continue;
                    if (l < Lx.at(ni[q], nj[q])) return -60;         // the count must bound the neighbour's
                    exit_scan = std::max(exit_scan, db + fs.ap + sufl(ni[q], nj[q], l));
                    exit_static = std::max(exit_static, db + fs.ap + funnel_suf<int64_t>(n - ni[q], m - nj[q], fs));
                }
            }
    }
    const auto clamp30 = [](int64_t v) { return (int)std::max<int64_t>(-(1ll << 30), std::min<int64_t>(v, 1ll << 30)); };
    info[1] = v0; info[2] = clamp30(band_bound(n, m, p, band_w)); info[3] = clamp30(exit_k); info[4] = count;
    info[5] = clamp30(exit_scan); info[6] = ex_lcs; info[9] = clamp30(exit_static);
    info[0] = count == nstrips && v0 > info[2] && v0 > info[3];
    return 0;
}

#ifdef SIM_MAIN
#include <cstdio>
#include <random>
int main() {
    const int systems[2][6] = {{8, -4, -7, -7, -3, 0}, {10, -5, -7, -7, -2, -2}};
    const int shapes[5][2] = {{1024, 1100}, {1280, 1024}, {1537, 2049}, {1100, 1100}, {2300, 2200}};
    int bad = 0;
    for (int sh = 0; sh < 5; ++sh)
        for (int sy = 0; sy < 2; ++sy) {
            const int n = shapes[sh][0], m = shapes[sh][1];
            std::mt19937 rng(77 + sh);
            std::vector<int32_t> t(n), o;
            for (int i = 0; i < n; ++i) t[i] = rng() % 27;
            for (int i = 0; i < n && (int)o.size() < m; ++i) {           // a noisy copy
                const unsigned u = rng() % 100;
                if (u < 8) continue;
                o.push_back(u < 20 ? (int32_t)(rng() % 27) : t[i]);
                if (rng() % 100 < 6) o.push_back((int32_t)(rng() % 27));
            }
            while ((int)o.size() < m) o.push_back((int32_t)(rng() % 27));
            o.resize(m);
            int info[10];
            const int rc = sim_nw2_funnel_lcs(t.data(), n, o.data(), m, systems[sy], 600, 27, info, nullptr, nullptr);
            const bool ok = rc == 0 && (info[7] != 2 || (info[8] == 1 && info[3] == info[5] && info[4] == (n + 255) / 256));
            printf("%d x %d system %d: rc %d flag %d table %d exit %d scan %d static %d v0 %d certified %d %s\n", n, m, sy, rc,
                   info[7], info[8], info[3], info[5], info[9], info[1], info[0], ok ? "ok" : "BAD");
            bad += !ok;
        }
    return bad ? 1 : 0;
}
#endif
