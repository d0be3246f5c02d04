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

}  // namespace ta
