// nw_band.h -- the band of the two-phase aligner's fill (ta_nw2.hip): which groups of a strip it runs, the sentinel
// that stands for everything outside, and the bound its certificate compares with.  Shared by the HIP kernel and the
// host-side replay of the banded data flow (tests/native/sim_nw_band.cpp).
#pragma once
#include <stdint.h>

#include "nw_cell.h"

namespace ta {

// Banded phase 1.  Band B(w) = the cells with lo <= j - i <= hi, lo = min(0, m - n) - w,
// hi = max(0, m - n) + w.
//
// Bound.  A path from (0, 0) to (n, m) that visits a cell with j - i > hi takes at least v = max(0, n - m) + w + 1
// vertical steps, so at most n - v diagonal ones (j - i < lo: the same with horizontal steps and m).  A diagonal step
// scores at most a = max(match, mismatch), a vertical one at most cv = max(gex + max(gox, 0), -1), a horizontal one at
// most ch = max(gey + max(goy, 0), -1) (-1: the boundary's G, textSeqCompare.py:53-60), so with #D diagonal steps the
// path scores at most #D a + (n - #D) cv + (m - #D) ch: linear in #D, hence largest at an end of its range.  U(w) is
// the larger of the two sides' values (band_bound below, host integers).
//
// Exactness.  The banded fill replaces every input from outside the band by a low sentinel; the recurrence is
// monotone in its inputs, so every banded value is <= the true one.  The walk starts at cell (n, m) in the state PM(n, m)
// names (tb_start), a tag phase 1 never forms, so let v0 be the SMALLEST of the banded M, X, Y of (n, m): M(n, m) > U
// makes that start state the reference's, and whichever state it is, its value exceeds U.  If v0 > U(w) strictly, every optimal path for that start, and every
// best prefix of every cell on one, stays inside B(w): on those cells banded and true values coincide; a predecessor
// that loses in truth also loses banded (banded <= true < max); ties are between cells that are themselves on optimal
// paths and therefore exact.  So every pointer the walk reads is the reference's, "first maximum wins" included.
// If v0 <= U(w) nothing is claimed: the problem's word stays 0 and today's full kernel fills it again.
//
// Strip s runs groups gl .. gh - 1 only: the groups that hold, for its 256 rows, the band's cells, plus what a chunk
// job of phase 2 for a walk inside the band reads -- the chunk's state checkpoint (tb_job_at: chunk floor((k - 2) /
// 64) of skewed step k), lane 31's row from 32 columns before the chunk's first step, both rows up to the chunk's
// halo group -- i.e. one whole checkpoint interval of margin on either side, in whole intervals.
constexpr int kBandSentinel = -(1 << 24);   // below every score (|score| < 2^23: ta_nw2_batch's score_bound); what grows
                                            // out of it stays within int32 in phase 2's encoded form (x 64) up to kBandMaxLen
constexpr int kBandMaxLen = 32768;
static_assert(((int64_t)kBandSentinel - 2ll * kBandMaxLen * 128 - (1 << 21)) * 64 > INT32_MIN, "sentinel-derived values, encoded");
struct BandRange { int gl, gh; };
TA_HD BandRange band_groups(int n, int m, int w, int s) {
    const int ngroups = PtrLayout<4>::ngroups(m);
    const int lo = (m < n ? m - n : 0) - w, hi = (m > n ? m - n : 0) + w;
    const int i0 = s * 256 + 1;                                   // the strip's first row
    const int jmin = i0 + lo > 1 ? i0 + lo : 1;
    const int jmax = i0 + 255 + hi < m ? i0 + 255 + hi : m;
    const int kmin = jmin - 1, kmax = jmax - 1 + 63;              // skewed steps of the band's cells in this strip
    int gl = kmin >= 2 ? ((kmin - 2) / 64) * 16 - 16 : 0;
    if (gl < 0) gl = 0;
    int gh = (kmax / 64) * 16 + 32;
    if (gh >= ngroups || gh <= gl) gh = ngroups;
    if (gl >= gh) gl = 0;
    return BandRange{gl, gh};
}

inline int64_t bmax(int64_t a, int64_t b) { return a > b ? a : b; }
inline int64_t bmin(int64_t a, int64_t b) { return a < b ? a : b; }
// U(w) for one problem: no path from (0, 0) to (n, m) that leaves B(w) scores more.
inline int64_t band_bound(int64_t n, int64_t m, const int32_t* prm, int64_t w) {
    const int64_t a = bmax(prm[0], prm[1]);
    const int64_t cv = bmax((int64_t)prm[4] + bmax(prm[2], 0), -1);
    const int64_t ch = bmax((int64_t)prm[5] + bmax(prm[3], 0), -1);
    const int64_t none = -(1ll << 40);                             // the side has no cell: nothing leaves through it
    auto side = [&](int64_t d_max) -> int64_t {                     // d_max: most diagonal steps of a path that leaves
        if (d_max < 0) return none;
        d_max = bmin(d_max, bmin(n, m));
        auto f = [&](int64_t d) { return d * a + (n - d) * cv + (m - d) * ch; };
        return bmax(f(0), f(d_max));
    };
    const int64_t above = side(n - (bmax(0, n - m) + w + 1));   // j - i > hi: vertical steps to come back
    const int64_t below = side(m - (bmax(0, m - n) + w + 1));   // j - i < lo: horizontal ones
    return bmax(above, below);
}

// ---- the funnel: a region that narrows towards (n, m), certified at its own border ----
//
// U(w) above ignores the data: it assumes that every diagonal step of a path that leaves the band is a match.  A path
// that leaves a filled region has a FIRST exit; its prefix up to there lies inside the region, where the banded fill
// has already computed an upper bound for it -- the banded value of the cell it leaves from.  Only the remainder needs
// a static bound, and the remainder shrinks with the rows left, so the region may narrow towards the last cell.
//
// Region R.  Strip s runs groups gl(s) .. gh(s) - 1 (funnel_groups below; any ranges that do not decrease with s
// serve).  Row i of the strip is strip lane l and holds the columns jlo(i) .. jhi(i):
//   jlo(i) = 1 if gl = 0, else 4 gl - l + 3      jhi(i) = m if gh = ngroups, else min(m, 4 gh - l).
// (The strip computes two more skewed steps on the left, k = 4 gl and 4 gl + 1.  They are left out of R: phase 2
// re-fills a walk's cell at step k from the state checkpoint of chunk floor((k - 2) / 64) (tb_job_at), and of the chunk
// before group gl the strip has none.  A smaller R only raises the bound.)  Everything else is the sentinel.
//
// Constants.  cvi = gex + max(gox, 0), chi = gey + max(goy, 0): the best interior vertical / horizontal step (without
// the boundary's -1); a = max(match, mismatch); a+ = max(a, cvi, chi): the best step of any kind.
//
// Static bound on the remainder.  From an interior cell (i, j), in any state, to (n, m): rn = n - i rows and rm = m - j
// columns are left; with #D diagonal steps the remainder scores at most #D a + (rn - #D) cvi + (rm - #D) chi, linear in
// #D in [0, min(rn, rm)], hence  Suf(i, j) = max(rn cvi + rm chi, d a + (rn - d) cvi + (rm - d) chi),  d = min(rn, rm).
//
// Exit bound.  X^ = the maximum of Db(c) + a+ + Suf(c') over every cell c in R or on the boundary row / column 0 and
// every neighbour c' of c among (i, j + 1), (i + 1, j), (i + 1, j + 1) that is an interior cell of the table outside R.
// Db(c) is the largest of the banded M, X, Y of c; on the boundary it is -i or -j.
//
// Soundness.  A complete path that visits a cell outside R has a first such cell c'; the cell c before it is in R or
// on the boundary, and so is the whole prefix up to c.  Banded values bound prefixes that stay inside the computed
// cells from above (the sentinel only ever replaces inputs such a prefix does not use), so the prefix scores at most
// Db(c), the step at most a+, the rest at most Suf(c').
//
// Exactness.  If v0 (the smallest of the banded M, X, Y of (n, m), as above) satisfies v0 > X^ strictly, the band's
// exactness argument carries over word for word with R in place of B(w).
//
// What the kernel owes (BAND = 3 in ta_nw2.hip; tests/native/sim_nw_funnel.cpp proves the list complete against a
// scan of all cells).  The cells of R with a neighbour outside are
//  1. the right edge of a strip with gh < ngroups: after the strip's last step lane l stands at column jr = 4 gh - l.
//     If jr <= m: its D[r] of the rows <= n, with Suf of the right and diagonal neighbours, and for r = 3, l < 63 of
//     the one below (the lane below stops one column earlier; below lane 63 the next strip goes on).  If jr + 1 <= m:
//     its dsave -- the lane above's last row at column jr -- with Suf(row0 + 1, jr + 1);
//  2. the left edge of a strip with gl > 0: the row above it (the bottom row of strip s - 1, in HBM), columns
//     jlo(that row) .. min(m, 4 gl + 2), with Suf of the neighbour below and, up to column 4 gl + 1, of the diagonal one;
//  3. the boundary row 0 and column 0, whose values are closed-form: funnel_exit0 below, on the host, per problem --
//     the initial value of the problem's exit word.
// Values in the kernel are hatted; + gex i + gey j un-hats them.
struct FunnelSys { int a, cvi, chi, ap; };
TA_HD FunnelSys funnel_sys(const int32_t* prm) {
    FunnelSys f;
    f.a = prm[0] > prm[1] ? prm[0] : prm[1];
    f.cvi = prm[4] + (prm[2] > 0 ? prm[2] : 0);
    f.chi = prm[5] + (prm[3] > 0 ? prm[3] : 0);
    f.ap = f.a > f.cvi ? f.a : f.cvi;
    if (f.chi > f.ap) f.ap = f.chi;
    return f;
}
template <typename T>
TA_HD T funnel_suf(T rn, T rm, const FunnelSys& f) {
    const T d = rn < rm ? rn : rm;
    const T none = rn * (T)f.cvi + rm * (T)f.chi;
    const T most = d * (T)f.a + (rn - d) * (T)f.cvi + (rm - d) * (T)f.chi;
    return none > most ? none : most;
}

// The funnel inside the band B(w_outer).  With rem = n - 256 s rows left at the strip's first row, the strip keeps
// wh = ceil(a rem / (2 (a - cvi - chi))) + w0 columns right and wl = ceil(a rem / (a - 2 cvi - 2 chi)) + w0 columns left
// of the diagonals through the table's corners: the theta = 1/2 forms of (1 - theta) a rem / (a - cvi - chi) and
// (1 - theta) a rem / (theta a - cvi - chi), theta being the share of a min(n, m) a good alignment is expected to score
// (the band's rule, ta_nw2.hip), and w0 = max(128, min(n, m) / 32) the floor.  The widths are a heuristic -- how far out
// Suf of an exit still leaves the certificate room -- and nothing rests on them: the certificate is taken on whatever
// region was filled.  The offsets are clipped to the outer band's, and the groups follow by band_groups' margin and
// rounding rule.  gl < 0: no funnel under this system (a <= 0 or a denominator <= 0).
//
// PM (per mille, a template argument so that the static funnel's code is what it was) shrinks the rem-proportional
// part of both widths: 1000 is the funnel above; the LCS-bounded certificate (below) runs kFunnelLcsScalePm.  w0, the clip to the outer band, margins and rounding are the same.
constexpr int kFunnelFullPm = 1000;
#ifndef TA_FUNNEL_LCS_SCALE_PM
#define TA_FUNNEL_LCS_SCALE_PM 250              // (a build of the replay for tools/funnel_lcs_estimate.py's sweep sets another)
#endif
constexpr int kFunnelLcsScalePm = TA_FUNNEL_LCS_SCALE_PM;
template <int PM = kFunnelFullPm>
TA_HD BandRange funnel_raw(int n, int m, const FunnelSys& f, int w_outer, int s) {
    const int64_t den_h = 2ll * ((int64_t)f.a - f.cvi - f.chi), den_l = (int64_t)f.a - 2ll * f.cvi - 2ll * f.chi;
    if (f.a <= 0 || den_h <= 0 || den_l <= 0) return BandRange{-1, -1};
    const int ngroups = PtrLayout<4>::ngroups(m);
    const int w0 = (n < m ? n : m) / 32 > 128 ? (n < m ? n : m) / 32 : 128;
    const int64_t full = (int64_t)f.a * (n - 256 * s);
    const int64_t num = PM == kFunnelFullPm ? full : (full * PM + 999) / 1000;
    const int64_t wh = (num + den_h - 1) / den_h + w0, wl = (num + den_l - 1) / den_l + w0;
    const int off_lo = m < n ? m - n : 0, off_hi = m > n ? m - n : 0;
    const int lo = wl < w_outer ? off_lo - (int)wl : off_lo - w_outer;
    const int hi = wh < w_outer ? off_hi + (int)wh : off_hi + w_outer;
    const int i0 = s * 256 + 1;                                   // from here on: band_groups
    const int jmin = i0 + lo > 1 ? i0 + lo : 1;
    const int jmax = i0 + 255 + hi < m ? i0 + 255 + hi : m;
    const int kmin = jmin - 1, kmax = jmax - 1 + 63;
    int gl = kmin >= 2 ? ((kmin - 2) / 64) * 16 - 16 : 0;
    if (gl < 0) gl = 0;
    int gh = (kmax / 64) * 16 + 32;
    if (gh >= ngroups || gh <= gl) gh = ngroups;
    if (gl >= gh) gl = 0;
    return BandRange{gl, gh};
}
// The funnel is declined -- the uniform band runs instead -- unless the ranges do not decrease with s and every strip
// that starts past group 0 finds the columns its left edge reads (up to 4 gl + 2) among those the strip above computed.
template <int PM = kFunnelFullPm>
TA_HD bool funnel_ok(int n, int m, const FunnelSys& f, int w_outer) {
    const int nstrips = PtrLayout<4>::nstrips(n), ngroups = PtrLayout<4>::ngroups(m);
    BandRange prev{0, 0};
    for (int s = 0; s < nstrips; ++s) {
        const BandRange r = funnel_raw<PM>(n, m, f, w_outer, s);
        if (r.gl < 0) return false;
        if (s > 0) {
            if (r.gl < prev.gl || r.gh < prev.gh) return false;
            if (r.gl > 0 && prev.gh < ngroups && 4 * r.gl + 2 > 4 * prev.gh - 63) return false;
        }
        prev = r;
    }
    return true;
}
TA_HD BandRange funnel_groups(int n, int m, const int32_t* prm, int w_outer, int s) {
    const FunnelSys f = funnel_sys(prm);
    return funnel_ok(n, m, f, w_outer) ? funnel_raw(n, m, f, w_outer, s) : band_groups(n, m, w_outer, s);
}
// funnel_groups of every strip at once, rg[nstrips], with funnel_ok asked once; true: the funnel's own ranges run
template <int PM = kFunnelFullPm>
inline bool funnel_ranges(int n, int m, const int32_t* prm, int w_outer, BandRange* rg) {
    const FunnelSys f = funnel_sys(prm);
    const bool own = funnel_ok<PM>(n, m, f, w_outer);
    const int nstrips = PtrLayout<4>::nstrips(n);
    for (int s = 0; s < nstrips; ++s) rg[s] = own ? funnel_raw<PM>(n, m, f, w_outer, s) : band_groups(n, m, w_outer, s);
    return own;
}

// columns of row i (1 <= i <= n) in R, given its strip's range
TA_HD int funnel_jlo(const BandRange& r, int i) { return r.gl == 0 ? 1 : 4 * r.gl - ((i - 1) % 256) / 4 + 3; }
TA_HD int funnel_jhi(const BandRange& r, int i, int m) {
    if (r.gh == PtrLayout<4>::ngroups(m)) return m;
    const int j = 4 * r.gh - ((i - 1) % 256) / 4;
    return j < m ? j : m;
}
// Part 3 of the exit bound: the exits from the boundary row and column, un-hatted.  rg[nstrips]: the strips' ranges.
inline int64_t funnel_exit0(int n, int m, const int32_t* prm, const BandRange* rg) {
    const FunnelSys f = funnel_sys(prm);
    int64_t best = -(1ll << 40);
    auto out = [&](int i, int j) {                                  // (i, j) is an interior cell outside R
        if (i < 1 || i > n || j < 1 || j > m) return false;
        const BandRange& r = rg[(i - 1) / 256];
        return j < funnel_jlo(r, i) || j > funnel_jhi(r, i, m);
    };
    auto take = [&](int64_t db, int i, int j) {
        if (out(i, j)) best = bmax(best, db + f.ap + funnel_suf<int64_t>(n - i, m - j, f));
    };
    for (int j = 0; j <= m; ++j) { take(-j, 1, j); take(-j, 1, j + 1); }
    for (int i = 1; i <= n; ++i) { take(-i, i, 1); take(-i, i + 1, 1); }
    return best;
}

// ---- the remainder bounded by the suffix LCS ----
//
// Suf assumes that every diagonal step of the remainder is a match.  The matches on any path from (i, j) to (n, m)
// are a common subsequence of T[i+1..n] and O[j+1..m] ("match": the token ids are equal, as the kernel's profile
// decides it), so there are at most L(i, j) = LCS(T[i+1..n], O[j+1..m]) of them.  Let l' = min(l, min(rn, rm)) for any
// l >= L(i, j).  With #D diagonal steps of which #M <= min(#D, l') are matches the remainder scores at most
//     #M match + (#D - #M) mismatch + (rn - #D) cvi + (rm - #D) chi.
// For match > mismatch this grows with #M, so #M = min(#D, l'); as a function of #D it is then linear on [0, l'] and on
// [l', d], d = min(rn, rm): the maximum is at #D in {0, l', d}.  Where mismatch >= match the count of matches buys
// nothing and the bound is Suf itself; in every case the smaller of the two is taken, so SufL <= Suf.
//
// Soundness of the exit bound with SufL.  Only the clause "the rest at most Suf(c')" changes: the rest scores at most
// SufL(c', l) for any l >= L(c').  L does not increase with i or j (a suffix of a suffix), so L of the border cell c --
// or of any cell that c' dominates in both coordinates -- serves for each of c's outside neighbours c'.
struct FunnelLcs { int mat, mis; };
TA_HD FunnelLcs funnel_lcs_sys(const int32_t* prm) { return FunnelLcs{prm[0], prm[1]}; }
template <typename T>
TA_HD T funnel_suf_lcs(T rn, T rm, T l, const FunnelSys& f, const FunnelLcs& q) {
    const T stat = funnel_suf<T>(rn, rm, f);
    if (q.mis >= q.mat) return stat;
    const T d = rn < rm ? rn : rm;
    const T lp = l < d ? (l < 0 ? 0 : l) : d;
    const T none = rn * (T)f.cvi + rm * (T)f.chi;
    const T all_match = lp * (T)q.mat + (rn - lp) * (T)f.cvi + (rm - lp) * (T)f.chi;
    const T most = lp * (T)q.mat + (d - lp) * (T)q.mis + (rn - d) * (T)f.cvi + (rm - d) * (T)f.chi;
    T best = none > all_match ? none : all_match;
    if (most > best) best = most;
    return best < stat ? best : stat;
}

// The LCS-bounded funnel: the rem-proportional widths at kFunnelLcsScalePm per mille of the static funnel's.  Nothing
// rests on the constant -- the certificate is taken on whatever region was filled; tools/funnel_lcs_estimate.py
// chose it (profiles/funnel_lcs_ab.txt: the smallest value at which every problem of the sweep certifies with at least
// half of the static funnel's smallest margin).
// nw_lcs_suffix_kernel keeps one 64-bit word of the row per lane: problems with more columns are declined (the static
// funnel runs for them), and so are alphabets past kLcsMaxAlphabet, the largest the 8-bit alphabet hint is trusted for
// (the two-level masks below would take 512 B for every eight symbols more: the LDS is not what limits it).
constexpr int kLcsMaxM = 4096;
constexpr int kLcsMaxAlphabet = 64;

// The kernel's match masks, two-level: a column matches symbol c exactly where its symbol has c's high part c >> 3 AND c's
// low part c & 7, so M(c) = A[c >> 3] & B[c & 7] with A of ceil(alphabet / 8) rows plus one all-zero pad row and B of 8
// rows -- 13 rows at alphabet 27 where one row per symbol took 28, 17 at kLcsMaxAlphabet.  A row is [lane] 64-bit words
// (512 B; the bank is the lane), A's rows first, then the pad row, then B's.  With the strips' ranges behind them a
// one-wave workgroup stays at or under 10 240 B = 160 KiB / 16, so that LDS allows 16 of them per CU.
// A code's two rows travel as ONE word: A's byte offset in the high half, B's in the low half.  The pad symbol and every
// code outside the alphabet take the pad row of A (and B's row 0): their M is 0.
constexpr int kLcsMaskRowBytes = 512;
TA_HD int lcs_mask_hi_rows(int alphabet) { return (alphabet + 7) >> 3; }           // A's rows, the pad row not counted
TA_HD int lcs_mask_rows(int alphabet) { return lcs_mask_hi_rows(alphabet) + 1 + 8; }
TA_HD uint32_t lcs_mask_offsets(int code, int alphabet) {
    const int nhi = lcs_mask_hi_rows(alphabet);
    const bool in = (unsigned)code < (unsigned)alphabet;
    const uint32_t hi = in ? (uint32_t)code >> 3 : (uint32_t)nhi, lo = (uint32_t)nhi + 1 + (in ? (uint32_t)code & 7 : 0);
    return (hi * kLcsMaskRowBytes) << 16 | lo * kLcsMaskRowBytes;
}
TA_HD uint32_t lcs_mask_pad(int alphabet) { return lcs_mask_offsets(-1, alphabet); }
// LDS of a workgroup: the rows, and (gl, gh) per strip of the batch's tallest problem
TA_HD size_t lcs_mask_lds_bytes(int alphabet, int max_n) {
    return (size_t)lcs_mask_rows(alphabet) * kLcsMaskRowBytes + 8 * (size_t)PtrLayout<4>::nstrips(max_n);
}
static_assert((kLcsMaxAlphabet + 7) / 8 + 1 + 8 == 17 && 17 * kLcsMaskRowBytes + 8 * ((kBandMaxLen + 255) / 256) <= 10240,
              "nw_lcs_suffix_kernel: 16 one-wave workgroups per CU at every alphabet and height it takes");

// The table nw_lcs_suffix_kernel leaves per problem (int32 words; stride from the batch's largest sizes):
//   edge[64 s + l]                 L(256 s + 4 l, 4 gh(s) - l): the right edge's count of strip s, lane l (0 where the
//                                  strip has no right edge, the lane no rows, or the column lies past m)
//   per strip s, at lcs_row_off(max_n) + 192 s:  the row i = 256 s as bits[64] (uint64, two words each; bit b of word
//   l set <=> L(i, m - 64 l - b - 1) = L(i, m - 64 l - b) + 1 -- the reversed strings' LCS row, complemented) and
//   pref[64], the matches in the words before l.
// L(i, j) of such a row = pref[w] + popcount(bits[w] & low mask), w = (m - j) / 64 (lcs_row_at below).
TA_HD int lcs_row_off(int max_n) { return (max_n + 1 + 63) & ~63; }
TA_HD int64_t lcs_stride(int max_n) { return (int64_t)lcs_row_off(max_n) + 192ll * PtrLayout<4>::nstrips(max_n); }
TA_HD int lcs_row_at(const int32_t* row, int m, int j) {
    const int c = m - j;                                             // columns of the reversed row that count
    if (c <= 0) return 0;
    const int w = c >> 6, b = c & 63;
    if (w >= 64) return row[128 + 63] + __builtin_popcountll(((const uint64_t*)row)[63]);
    const uint64_t bits = ((const uint64_t*)row)[w];
    return row[128 + w] + (b ? __builtin_popcountll(bits & ((1ull << b) - 1)) : 0);
}

// When nw_lcs_suffix_kernel stores the right edge's counts.  The rows run skewed, row r = n - i of the reversed strings
// passing lane w at step r - 1 + w, and edge[64 s + l] is the count of the first cnt = m - 4 gh(s) + l columns of row
// r = n - 256 s - 4 l: lane w = cnt / 64 stores it at step r - 1 + w from its bits below b = cnt % 64.  Strips from the
// last and lanes from 63 is the order of the steps.  One lane down, r grows by 4 and cnt falls by 1, so as long as cnt
// stays in one word the stores are exactly 4 steps apart at the same lane w, b falling by 1: a RUN
//     (t0, w, s, l, b, count):  its k-th store, k < count, is at step t0 + 4 k by lane w, bit b - k, into edge[64 s + l - k].
// A run ends where cnt crosses into the word below (the next run of the strip starts 3 steps later, at b = 63), at the
// strip's lane 0, or at cnt < 0 (the column lies past m); a strip starts below its lanes without rows (r < 1) and has no
// run at all at gh >= ngroups (no right edge).  At most two runs per strip.
struct LcsRun { int t0, w, s, l, b, count; };                        // count 0: none left (t0 = INT32_MAX)
struct LcsRunCursor { int s, l; };                                   // where the next run starts; l < 0: at the top of strip s - 1
TA_HD LcsRunCursor lcs_run_begin(int n) { return LcsRunCursor{PtrLayout<4>::nstrips(n), -1}; }
template <typename GhOf>                                             // gh_of(s): the strip's gh
TA_HD LcsRun lcs_next_run(int n, int m, int ngroups, LcsRunCursor& c, GhOf&& gh_of) {
    while (true) {
        if (c.l < 0) {
            if (--c.s < 0) return LcsRun{INT32_MAX, 0, 0, 0, 0, 0};
            const int top = (n - 256 * c.s - 1) >> 2;                // the last lane with r >= 1
            c.l = top < 63 ? top : 63;
        }
        const int gh = gh_of(c.s);
        const int lmin = 4 * gh > m ? 4 * gh - m : 0;                // the first lane with cnt >= 0
        if (gh >= ngroups || c.l < lmin) { c.l = -1; continue; }
        const int cnt = m - 4 * gh + c.l, b = cnt & 63, left = c.l - lmin + 1;
        const LcsRun r{n - 256 * c.s - 4 * c.l - 1 + (cnt >> 6), cnt >> 6, c.s, c.l, b, b + 1 < left ? b + 1 : left};
        c.l = r.count == left ? -1 : c.l - r.count;
        return r;
    }
}

}  // namespace ta
