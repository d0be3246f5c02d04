// tests/native/sim_nw_funnel.cpp -- host-side replay of the FUNNEL data flow of the two-phase aligner (TEST ONLY).
//
// Phase 1 as nw_score_kernel<.., BAND = 3> runs it (text_alignment_amd/csrc/ta_nw2.hip): strip s runs the groups
// funnel_groups() gives it inside a forced outer band, starts from the sentinel state where its first group is not 0,
// leaves the sentinel tails in its rows, and gathers the certificate's three words in the kernel's order: the left edge
// from the row above at the strip's start, the right edge from the lane state at its end, the count, and v0 on the way
// into cell (n, m).  The exit word must EQUAL a scan of every cell of the region for neighbours outside it (info[5]):
// that is what proves the kernel's list of edge cells complete.  Everything phase 1 did not write is marked, and phase
// 2 -- the replay of sim_nw_band.cpp, unchanged -- fails if it restarts from or re-fills with anything unwritten; so
// does a scan of everything phase 2 could read for ANY walk inside the region, which does not depend on where the
// tests' walks happen to go.
// Uses the SAME nw_band.h / nw_cell.h as the kernel.
#include "sim_nw.cpp"

#include "../../text_alignment_amd/csrc/nw_band.h"

static int run2_funnel(const int32_t* t, int n, const int32_t* o, int m, const int* p, int band_w, int GSPAN,
                     uint8_t* ops_out, int* ops_len, int* info) {
    constexpr int R = 4, KCG = 16;
    using L = PtrLayout<R>;
    constexpr int SPG = L::SPG;
    const CellConsts c = make_consts(p[0], p[1], p[2], p[3], p[4], p[5]);
    const int cmat_raw = p[0] - p[4] - p[5], cmis_raw = p[1] - p[4] - p[5];
    const int nstrips = L::nstrips(n), ngroups = L::ngroups(m);
    const int nck = ngroups / KCG + 1;
    struct State { int D[kLanes][R], H[kLanes][R], Vlast[kLanes], dsave[kLanes]; };
    std::vector<State> ck_((size_t)std::max(nstrips, 1) * nck);
    std::vector<char> ck_ok(ck_.size(), 0);               // what the banded phase 1 wrote: reading anything else is an error
    // bottom rows: row s is what strip s starts from (row 0 = the table's boundary row), strip s
    // leaves row s + 1; index [row][j], j = 0..m
    std::vector<int> HV((size_t)(std::max(nstrips, 1) + 1) * (m + 2)), HD(HV.size());
    // ... and, for the half-strip flow of nw_trace2h_kernel, the bottom rows of lanes 31 and 63 of every strip
    // (Ws2 with kSubRows = 2): sub row 0 = the table's boundary row, sub row 1 + 2 s + q = last row of lanes
    // 32 q .. 32 q + 31 of strip s; the row above half-strip hs is sub row hs
    std::vector<int> SV((size_t)(2 * std::max(nstrips, 1) + 1) * (m + 2)), SD(SV.size());
    std::vector<char> S_ok(SV.size(), 0);
    if (n < 2 || m < 1 || band_w < 0) return -1;

    // phase 1 keeps V~ + gox / H~ + goy (the carried cell of nw_cell.h) when no gap open is
    // positive, exactly as nw_score_kernel does; phase 2 undoes the offsets where it reads them
    const bool carried = opens_nonpositive(c.gox, c.goy);
    const int xadj = carried ? c.gox : 0, yadj = carried ? c.goy : 0;
    if (!carried) return -2;                              // the banded kernel leaves such a problem to the full one
    int v0 = INT32_MIN;
    // the strips' ranges: the funnel inside B(band_w), or the band's own where the funnel is declined
    const FunnelSys fs = funnel_sys(p);
    const bool funnel = funnel_ok(n, m, fs, band_w);
    std::vector<BandRange> rg(nstrips);
    for (int s = 0; s < nstrips; ++s) {
        rg[s] = funnel_groups(n, m, p, band_w, s);
        const BandRange want = funnel ? funnel_raw(n, m, fs, band_w, s) : band_groups(n, m, band_w, s);
        if (rg[s].gl != want.gl || rg[s].gh != want.gh) return -40;
        if (s > 0 && (rg[s].gl < rg[s - 1].gl || rg[s].gh < rg[s - 1].gh)) return -41;
    }
    const int64_t x0 = funnel_exit0(n, m, p, rg.data());
    int64_t exit_k = std::max<int64_t>(-(1ll << 30), std::min<int64_t>(x0, 1ll << 30));   // the exit word, as launched
    int count = 0;
    // every banded D of the region, un-hatted, for the scan
    std::vector<int> Dall((size_t)(n + 1) * (m + 1), 0);
    const auto unhat = [&](int v, int i, int j) { return v + p[4] * i + p[5] * j; };
    const auto suf = [&](int i, int j) { return funnel_suf<int64_t>(n - i, m - j, fs); };

    // ---------------- phase 1: raw fill ----------------
    {
        for (int j = 0; j <= m; ++j) { HV[j] = raw_of(bnd_V_row0(c, j)) + xadj; HD[j] = raw_of(bnd_D_row0(c, j)); SV[j] = HV[j]; SD[j] = HD[j]; S_ok[j] = 1; }
        for (int s = 0; s < nstrips; ++s) {
            const int* hv = &HV[(size_t)s * (m + 2)];
            const int* hd = &HD[(size_t)s * (m + 2)];
            int* hv_out = &HV[(size_t)(s + 1) * (m + 2)];
            int* hd_out = &HD[(size_t)(s + 1) * (m + 2)];
            const char* top_ok = &S_ok[(size_t)(2 * s) * (m + 2)];
            int D[kLanes][R], V[kLanes][R], H[kLanes][R], tcode[kLanes][R], dsave[kLanes];
            strip_setup<false>(c, s, t, n, yadj, D, V, H, tcode, dsave);
            const BandRange br = rg[s];
            const int i0 = s * L::SR + 1;                     // the strip's first row
            if (br.gl % KCG || (br.gh % KCG && br.gh != ngroups) || br.gl >= br.gh || br.gh > ngroups) return -30;
            if (br.gl > 0)
                for (int l = 0; l < kLanes; ++l) {
                    for (int r = 0; r < R; ++r) D[l][r] = H[l][r] = V[l][r] = kBandSentinel;
                    dsave[l] = kBandSentinel;
                }
            if (br.gl > 0) {
                // lane 32's first step takes lane 31's state, the sentinel: phase 2 restarts the lower half-strip's
                // first chunk from lane 31's row, one column before the lane's first
                const size_t b = (size_t)(2 * s + 1) * (m + 2);
                const int col = br.gl * SPG - 31;
                if (col < 1 || S_ok[b + col]) return -33;
                SV[b + col] = SD[b + col] = kBandSentinel; S_ok[b + col] = 1;
                // the left edge: the row above, from the first column of R in it to column 4 gl + 2
                const int c_lo = rg[s - 1].gl == 0 ? 1 : rg[s - 1].gl * SPG - 60, c_hi = std::min(m, br.gl * SPG + 2);
                for (int j = c_lo; j <= c_hi; ++j) {
                    if (!top_ok[j]) return -34;
                    const int64_t db = unhat(hd[j], i0 - 1, j);
                    exit_k = std::max(exit_k, db + fs.ap + suf(i0, j));
                    if (j + 1 <= m && j + 1 <= br.gl * SPG + 2) exit_k = std::max(exit_k, db + fs.ap + suf(i0, j + 1));
                }
            }
            const int cert_lane = ((n - 1) % L::SR) / R, cert_r = (n - 1) % R;
            const auto cell = [&](int d_ul, int v_u, int h_l, int tt, int oo, int& d, int& v, int& h) {
                const int cs = (tt == oo) ? cmat_raw : cmis_raw;
                if (carried) cell_update_carried(d_ul, v_u, h_l, cs, c.gox, c.goy, d, v, h);
                else cell_update_raw(d_ul, v_u, h_l, cs, c.gox, c.goy, d, v, h);
            };
            for (int g = br.gl; g < br.gh; ++g) {
                if (g > 0 && g % KCG == 0) {
                    State& st = ck_[(size_t)s * nck + g / KCG];
                    ck_ok[(size_t)s * nck + g / KCG] = 1;
                    for (int l = 0; l < kLanes; ++l) {
                        for (int r = 0; r < R; ++r) { st.D[l][r] = D[l][r]; st.H[l][r] = H[l][r]; }
                        st.Vlast[l] = V[l][R - 1]; st.dsave[l] = dsave[l];
                    }
                }
                for (int q = 0; q < SPG; ++q) {
                    const int k = g * SPG + q;
                    int vup[kLanes], dnext[kLanes];
                    const int j0 = (k + 1 <= m) ? k + 1 : 0;
                    if (j0 > 0 && !top_ok[j0]) return -20;    // the row above, where the strip above never wrote it
                    shift_down<R>(0, kLanes, V, D, hv[j0], hd[j0], vup, dnext);
                    for (int l = 0; l < kLanes; ++l) {
                        const int j = k - l + 1;
                        if (j < 1 || j > m) continue;
                        // the certificate: the smallest of M, X, Y of cell (n, m) -- the inputs of its max3 -- un-hatted
                        const bool cert_here = s == nstrips - 1 && l == cert_lane && j == m;
                        const int cert_m = (cert_r == 0 ? dsave[l] : D[l][cert_r - 1]) + ((tcode[l][cert_r] == o[m - 1]) ? cmat_raw : cmis_raw);
                        const int cert_y = H[l][cert_r];
                        lane_step(cell, D[l], V[l], H[l], dsave[l], vup[l], dnext[l], tcode[l], o[j - 1]);
                        if (cert_here)
                            v0 = std::min(cert_m, std::min(cert_r == 0 ? vup[l] : V[l][cert_r - 1], cert_y)) + p[4] * n + p[5] * m;
                        if (l == kLanes - 1) { hv_out[j] = V[l][R - 1]; hd_out[j] = D[l][R - 1]; }
                        for (int r = 0; r < R; ++r)
                            if (i0 + l * R + r <= n) Dall[(size_t)(i0 + l * R + r) * (m + 1) + j] = unhat(D[l][r], i0 + l * R + r, j);
                        if ((l & 31) == 31) {
                            const size_t b = (size_t)(1 + 2 * s + l / 32) * (m + 2);
                            SV[b + j] = V[l][R - 1]; SD[b + j] = D[l][R - 1]; S_ok[b + j] = 1;
                        }
                    }
                }
            }
            if (br.gh < ngroups) {
                // the right edge, from the lane state after the strip's last step
                for (int l = 0; l < kLanes; ++l) {
                    const int jr = br.gh * SPG - l, row0 = i0 - 1 + l * R;
                    if (jr < 1) return -35;
                    if (jr <= m)
                        for (int r = 0; r < R; ++r) {
                            const int i = row0 + 1 + r;
                            if (i > n) continue;
                            const int64_t db = unhat(D[l][r], i, jr);
                            if (jr + 1 <= m) exit_k = std::max(exit_k, db + fs.ap + suf(i, jr + 1));
                            if (jr + 1 <= m && i + 1 <= n) exit_k = std::max(exit_k, db + fs.ap + suf(i + 1, jr + 1));
                            if (r == R - 1 && l < kLanes - 1 && i + 1 <= n) exit_k = std::max(exit_k, db + fs.ap + suf(i + 1, jr));
                        }
                    if (jr + 1 <= m && row0 + 1 <= n)
                        exit_k = std::max(exit_k, (int64_t)unhat(dsave[l], row0, jr) + fs.ap + suf(row0 + 1, jr + 1));
                }
                // the sentinel tails: of lane 31's row (the lower half-strip's last chunk re-fills one group past gh) ...
                {
                    const size_t b = (size_t)(2 * s + 1) * (m + 2);
                    for (int col = br.gh * SPG - 30; col <= std::min(m, br.gh * SPG - 28); ++col) {
                        if (S_ok[b + col]) return -36;
                        SV[b + col] = SD[b + col] = kBandSentinel; S_ok[b + col] = 1;
                    }
                }
                // ... and of the strip's last row
                if (s + 1 >= nstrips) return -31;
                const size_t b = (size_t)(2 * s + 2) * (m + 2);
                const int c_hi = std::min(m, rg[s + 1].gh * SPG + 4);
                for (int col = br.gh * SPG - 62; col <= c_hi; ++col) {
                    if (S_ok[b + col]) return -32;            // the tail must not overwrite what lane 63 stored
                    SV[b + col] = SD[b + col] = kBandSentinel; hv_out[col] = hd_out[col] = kBandSentinel; S_ok[b + col] = 1;
                }
            }
            ++count;
        }
    }

    // What phase 2 may read for a walk inside R, whether or not one of the tests' walks goes there: for every strip, as a
    // whole (the row above it) and for its lower half (lane 31's row), and every chunk that holds a step of R -- a cell
    // at step k belongs to chunk floor((k - 2) / 64) (tb_job_at) and its re-fill runs at most two groups past the cell's
    // (tb_predict), never past the chunk's halo group -- the chunk's state checkpoint and the columns of the row above
    // that the re-fill's steps take must have been written.
    for (int s = 0; s < nstrips; ++s) {
        const int k_lo = rg[s].gl == 0 ? 0 : rg[s].gl * SPG + 2, k_hi = rg[s].gh == ngroups ? L::nsteps(m) - 1 : rg[s].gh * SPG - 1;
        for (int ck = k_lo >= 2 ? (k_lo - 2) / (KCG * SPG) : 0; ck <= std::max(k_hi - 2, 0) / (KCG * SPG); ++ck) {
            if (ck > 0 && !ck_ok[(size_t)s * nck + ck]) return -37;
            const int k_last = std::min(k_hi, (ck + 1) * KCG * SPG + 1);
            const int g_top = std::min(k_last / SPG + 2, ck * KCG + KCG);
            for (int lb = 0; lb <= 32; lb += 32) {
                if (s == 0 && lb == 0) continue;                  // the table's boundary row: analytic
                const char* ok = &S_ok[(size_t)(2 * s + lb / 32) * (m + 2)];
                for (int kk = ck * KCG * SPG; kk <= g_top * SPG + SPG - 1; ++kk) {
                    const int j0 = kk - lb + 1;
                    if (j0 >= 1 && j0 <= m && !ok[j0]) return -38;
                }
            }
        }
    }

    // the scan: every cell of R or of the boundary, every neighbour of it that is an interior cell outside R
    int64_t exit_scan = -(1ll << 40);
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
                const int ni[3] = {i, i + 1, i + 1}, nj[3] = {j + 1, j, j + 1};
                for (int q = 0; q < 3; ++q) {
                    if (ni[q] < 1 || ni[q] > n || nj[q] < 1 || nj[q] > m || in_r(ni[q], nj[q])) continue;
                    exit_scan = std::max(exit_scan, db + fs.ap + suf(ni[q], nj[q]));
                }
            }
    }
    const auto clamp30 = [](int64_t v) { return (int)std::max<int64_t>(-(1ll << 30), std::min<int64_t>(v, 1ll << 30)); };
    const int64_t U = band_bound(n, m, p, band_w);
    info[1] = v0; info[2] = clamp30(U); info[3] = clamp30(exit_k); info[4] = count; info[5] = clamp30(exit_scan);
    info[6] = clamp30(x0); info[7] = funnel;
    info[0] = count == nstrips && v0 > info[2] && v0 > info[3];
    if (!info[0]) { *ops_len = 0; return 0; }             // not certified: the full kernel's business (sim_nw2)
    // ---------------- phase 2: chunked tagged re-fill + walk (nw_trace2_kernel's data flow) ----------------
    // A chunk = the KCG groups between two state checkpoints.  The chunk the walk is in is re-filled
    // with the tagged cell from its checkpoint (in carried form when phase 1 used it); its first two
    // steps carry no valid tags, so when the walk gets there the chunk before is re-filled one group
    // further (g_top = the first group of the chunk just left).  Of a chunk's pointer bytes only the lanes
    // l_lo .. l_lo + WL - 1 are kept, l_lo = max(0, entry lane - WL + 1) (WL = GSPAN if 0 < GSPAN < 64, else all
    // 64: nw_trace2_kernel's kWinLanes): a walk that needs a lane above l_lo stops, and the SAME chunk is
    // re-filled up to the group the walk stands in with the window at its lane.  Bytes outside the window
    // stay 0xEE here, so a walk that read one would fail with -7.
    // GSPAN >= 1000: the data flow of nw_trace2w_kernel (several waves per problem, each re-filling the chunk it
    // expects into a buffer of its own): whole chunks are kept (WL = 64; the entry lane of a chunk re-filled ahead of
    // the walk is not known), a chunk entered through its halo is re-filled to the first group of the chunk just left
    // with two steps of it -- what the one-wave flow does as well, so an expected chunk that turns out right IS the
    // chunk the walk needs -- and a position in a chunk's first two steps goes to the chunk before at once (tb_job_at)
    // instead of through a walk of zero steps.
    // GSPAN >= 2000: the half-strip flow of nw_trace2h_kernel on top of that: a strip restarts in two halves of 32 lanes
    // (from the same state checkpoints and from lane 31's bottom row), a step that leaves a HALF-strip upwards is
    // pending, and a half-strip's whole chunk is kept.
    const bool halves = GSPAN >= 2000;
    if (halves) GSPAN -= 1000;
    const bool skip_halo = GSPAN >= 1000;
    if (skip_halo) GSPAN -= 1000;
    const int LWs = halves ? 32 : kLanes;                   // lanes of the unit phase 2 restarts
    const int xadj6 = xadj * 64, yadj6 = yadj * 64;
    std::vector<uint8_t> rev;
    int x = n, y = m, st = 0;
    bool first = true;
    // pend: 0, or 3 + (state the strip was left in): the next state is the winner tag of D (3, left
    // in state M) or of XG / V~ (4, left in state X) of the cell (x, y) the walk now stands on.
    int pend = 0;
    bool probe = false;                               // start state of a walk that begins in a strip's first row
    if ((n - 1) % (LWs * R) == 0 && n > 1) {          // textSeqCompare.py:102 reads PM(n, m) = tag of D(n-1, m-1)
        if (m == 1) { st = 0; first = false; }        // D(n-1, 0): boundary column, M
        else { x = n - 1; y = m - 1; pend = 3; probe = true; }
    }
    int guard = 0;
    while (x > 0 && y > 0) {
        const int s = (x - 1) / L::SR;
        const int hs = (x - 1) / (LWs * R);                  // (half-)strip index; lanes lb .. lb + LWs - 1 of strip s
        const int lb = halves ? (hs & 1) * LWs : 0;
        int l = ((x - 1) % L::SR) / R, r = (x - 1) % R, k = (y - 1) + l;
        int ck = (k / SPG) / KCG;
        int g_top = k / SPG;
        if (skip_halo && ck > 0 && k < ck * KCG * SPG + 2) ck -= 1;      // tb_job_at
        // a chunk re-filled AHEAD of the walk for a strip entry (tb_predict) goes two groups further than the diagonal's
        // entry group, whole groups: a window re-filled further than the walk's entry point serves it as well
        if (skip_halo) g_top = std::min(g_top + 2, ck * KCG + KCG);     // (nw_trace2w_kernel and, on half-strips, nw_trace2hw_kernel)
        bool in_strip = true;
        while (in_strip) {
            if (++guard > 8 * (n + m) + 64) return -9;
            const int g0 = ck * KCG, k0 = g0 * SPG;
            const int kvalid = ck > 0 ? k0 + 2 : 0;
            // the row above the strip for columns k0 .. min(m, (g_top+1)*SPG), x-input in the re-fill's
            // form; tags only where they are known analytically (the table's boundary row)
            const int jhi = std::min(m, (g_top + 1) * SPG);
            std::vector<int> hvt(m + 2, 0), hdt(m + 2, 0);
            std::vector<char> hok(m + 2, 0);
            for (int j = std::max(0, k0 - lb); j <= jhi; ++j) {
                hok[j] = 1;
                if (hs == 0) { hvt[j] = bnd_V_row0(c, j) + xadj6; hdt[j] = bnd_D_row0(c, j); continue; }
                if (halves) {
                    const size_t b = (size_t)hs * (m + 2);
                    hvt[j] = enc_of(SV[b + j]); hdt[j] = enc_of(SD[b + j]); hok[j] = S_ok[b + j];
                    if (j == 0) { hvt[j] = 0; hdt[j] = bnd_D_col0(c, hs * LWs * R); hok[j] = 1; }   // column 0 of the row above (kernel: analytic)
                    continue;
                }
                const size_t b = (size_t)(2 * s) * (m + 2);
                hvt[j] = enc_of(SV[b + j]); hdt[j] = enc_of(SD[b + j]); hok[j] = S_ok[b + j];
            }
            // lane state at the start of group g0
            int D[kLanes][R], V[kLanes][R], H[kLanes][R], tcode[kLanes][R], dsave[kLanes];
            strip_setup<true>(c, s, t, n, yadj6, D, V, H, tcode, dsave);
            if (g0 > 0) {
                // lanes that have not started by step k0 (lane >= k0: only with checkpoint periods
                // shorter than 64 steps) keep the TAGGED boundary values: the scores are the same
                // and their column-0 tags are pointers of the column-1 cells
                if (!ck_ok[(size_t)s * nck + g0 / KCG]) return -21;    // a checkpoint phase 1 never wrote
                const State& cs0 = ck_[(size_t)s * nck + g0 / KCG];
                for (int ll = 0; ll < std::min(kLanes, k0); ++ll) {
                    for (int rr = 0; rr < R; ++rr) { D[ll][rr] = enc_of(cs0.D[ll][rr]); H[ll][rr] = enc_of(cs0.H[ll][rr]); }
                    V[ll][R - 1] = enc_of(cs0.Vlast[ll]); dsave[ll] = enc_of(cs0.dsave[ll]);
                }
            }
            // tagged fill of groups g0..g_top into the chunk buffer; the tagged outputs of the strip's
            // bottom row are kept per step for a pending state
            const int WL = halves ? LWs : (GSPAN > 0 && GSPAN < 64) ? GSPAN : 64;
            const int l_lo = halves ? lb : std::max(0, l - (WL - 1));
            std::vector<uint8_t> wbuf((size_t)(g_top - g0 + 1) * 1024, 0xEE);
            std::vector<int> capV((size_t)(g_top - g0 + 1) * SPG, 0), capD(capV.size(), 0);
            std::vector<char> capOk(capV.size(), 0);
            const auto cell = [&](int d_ul, int v_u, int h_l, int tt, int oo, int& d, int& v, int& h) {
                const int cs = (tt == oo) ? c.cmatch : c.cmismatch;
                return carried ? cell_update_carried_tagged(d_ul, v_u, h_l, cs, c.gox6, c.goy6, d, v, h)
                               : cell_update(d_ul, v_u, h_l, cs, c.gox6, c.goy6, d, v, h);
            };
            for (int g = g0; g <= g_top; ++g) {
                uint8_t acc[kLanes][16];
                memset(acc, 0xEE, sizeof(acc));
                // of the group the walk enters the chunk in only the steps up to the entry point are re-filled (two
                // of four when it stands in the group's first half, as the kernel does): the rest stays poisoned
                const int nq = (g == g_top && k / SPG == g_top && (k % SPG) + 1 <= 2) ? 2 : SPG;
                for (int q = 0; q < nq; ++q) {
                    const int kk = g * SPG + q;
                    int vup[kLanes], dnext[kLanes];
                    const int j0 = std::min(std::max(kk - lb + 1, 0), m);
                    if (kk - lb + 1 >= 1 && kk - lb + 1 <= m && !hok[j0]) return -22;   // the row above the unit (for a real column), where phase 1 never wrote it
                    shift_down<R>(lb, lb + LWs, V, D, hvt[j0], hdt[j0], vup, dnext);
                    for (int ll = lb; ll < lb + LWs; ++ll) {
                        const int j = kk - ll + 1;
                        if (j < 1 || j > m) continue;
                        unsigned b[R];
                        lane_step(cell, D[ll], V[ll], H[ll], dsave[ll], vup[ll], dnext[ll], tcode[ll], o[j - 1], b);
                        for (int rr = 0; rr < R; ++rr) acc[ll][q * R + rr] = (uint8_t)(b[rr] & 0x3F);
                        if (ll == lb + LWs - 1) {             // the (half-)strip's bottom row, tagged
                            capV[kk - k0] = V[ll][R - 1]; capD[kk - k0] = D[ll][R - 1]; capOk[kk - k0] = 1;
                        }
                    }
                }
                for (int ll = l_lo; ll < std::min(kLanes, l_lo + WL); ++ll) memcpy(&wbuf[((size_t)(g - g0) * 64 + ll) * 16], acc[ll], 16);
            }
            auto byte_at = [&](int ll, int rr, int kk) -> unsigned {
                return wbuf[((size_t)(kk / SPG - g0) * 64 + ll) * 16 + (kk % SPG) * R + rr];
            };
            if (pend) {                                   // the cell the walk stands on: bottom row of this strip
                if (l != lb + LWs - 1 || r != R - 1) return -10;
                if (k < k0 || k / SPG > g_top || !capOk[k - k0]) return -11;
                const int tagged = (pend == 3) ? capD[k - k0] : capV[k - k0];
                st = 2 - (tagged & 3);
                pend = 0;
                if (probe) {                              // that was the start state: back to (n, m)
                    probe = false; first = false;
                    x = n; y = m;
                    break;
                }
            }
            if (first && k >= kvalid) { st = ptr_pm(byte_at(l, r, k)); first = false; }   // start state, textSeqCompare.py:102
            int steps = 0;
            while (x > 0 && y > 0 && l >= l_lo && k >= kvalid) {
                if (k / SPG > g_top) return -6;               // would read past what this chunk re-filled
                const unsigned b = byte_at(l, r, k);
                if (b == 0xEE) return -7;
                const int up = (st != 2), left = (st != 1);
                rev.push_back((uint8_t)st);
                const bool leaves_up = up && l == lb && r == 0 && hs > 0;   // PM / PX of the (half-)strip's first row
                if (leaves_up) pend = 3 + st;
                else st = 2 - (int)((b >> (2 * st)) & 3u);
                const int wrap = up & (r == 0);
                r = (r - up) & (R - 1);
                x -= up; y -= left; k -= left + wrap; l -= wrap;
                ++steps;
            }
            if (x <= 0 || y <= 0 || l < lb) in_strip = false;
            else if (k >= kvalid) {
                if (steps == 0) return -12;                   // no progress: the entry lane is always in its window
                if (skip_halo) return -13;                    // whole chunks are kept: the walk cannot run off a window
                g_top = k / SPG;                              // ran off the window's top lane: same chunk, window at l
            } else {
                if (skip_halo && steps == 0) return -14;     // tb_job_at never starts a walk in a chunk's halo
                g_top = g0;
                ck -= 1;
                if (ck < 0) return -5;
            }
        }
    }
    while (y > 0) { rev.push_back(2); --y; }
    while (x > 0) { rev.push_back(1); --x; }
    const int len = (int)rev.size();
    for (int a = 0; a < len; ++a) ops_out[a] = rev[len - 1 - a];
    *ops_len = len;
    return 0;
}


// info[0] = 1 if the certificate passed (the alignment is then in ops_out); info[1] = v0, the smallest of the banded M,
// X, Y of (n, m); info[2] = U(band_w); info[3] = the exit word as the kernel gathers it; info[4] = strips counted;
// info[5] = the exit bound by the scan of all cells; info[6] = its host part; info[7] = 1 if the funnel's ranges ran;
// ranges_out[2 nstrips] = (gl, gh) per strip
extern "C" int sim_nw2_funnel(const int32_t* t, int n, const int32_t* o, int m, const int* params, int band_w, int GSPAN,
                            uint8_t* ops_out, int* ops_len, int* info, int* ranges_out) {
    if (ranges_out)
        for (int s = 0; s < PtrLayout<4>::nstrips(n); ++s) {
            const BandRange r = funnel_groups(n, m, params, band_w, s);
            ranges_out[2 * s] = r.gl; ranges_out[2 * s + 1] = r.gh;
        }
    return run2_funnel(t, n, o, m, params, band_w, GSPAN, ops_out, ops_len, info);
}
