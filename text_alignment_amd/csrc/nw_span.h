// nw_span.h -- the pieces of the span-locating fill (ta_nw_span.hip) that do not need a GPU: the value that carries
// an ORIGIN with every score, its cell, the free column-0 boundary, a lane's step over its R rows, the last-column
// maximum and how the partial results combine.  Shared by the kernel and by the host-side lane simulator
// (tests/native/sim_span.cpp), like nw_cell.h; the definition of record is DESIGN.md section 4.6, its checker
// tests/span_ref.py.
//
// What is computed: the affine-gap table of nw_cell.h (same interior recurrence, same row-0 boundary, same hatted form
// D / V~ / H~) whose column 0 is FREE -- M(i,0) = Y(i,0) = 0, X(i,0) = -inf -- so that an alignment of the whole OCR
// string may start at any transcript position i0 = its ORIGIN.  Every value carries the origin of the candidate it
// took; candidates are ordered by score and, at equal score, by the LARGER origin.  No pointer is produced.
//
// Carrier.  One float64 per value: score * 2^28 + origin.  |score| < 2^23 (the bound NWBatch applies) and
// 0 <= origin < 2^28, so every value and every sum the cell forms is an integer below 2^52: exact.  The lexicographic
// maximum is ONE v_max_f64, a score offset ONE v_add_f64, and the match / mismatch constants differ in the high dword
// only (the low dword of k * 2^28, |k| < 2^21, is zero: parameters up to 2^19), so the select is one v_cndmask_b32.
// Priced against an int64 carrier with v_cmp_gt_i64 and the plain int cell: tools/ubench/span_carrier.hip, DESIGN.md
// section 4.6 (1.20 x the int cell; the int64 form 2.27 x).
#pragma once
#include <stdint.h>

#include "nw_cell.h"

namespace ta {

typedef double SpanVal;
constexpr int kSpanOriginBits = 28;
constexpr double kSpanUnit = 268435456.0;                  // 2^28: one score point
constexpr int kSpanMaxN = (1 << kSpanOriginBits) - 1;      // origins 0 .. n must fit the origin field
constexpr int kSpanNone = INT32_MIN / 2;                   // score of "no row seen yet"

TA_HD SpanVal span_val(int score, int origin) { return (double)score * kSpanUnit + (double)origin; }
TA_HD int span_score(SpanVal v) {                          // floor(v / 2^28): the division is exact
    const double q = v * (1.0 / kSpanUnit);
    const long long t = (long long)q;
    return (int)(((double)t > q) ? t - 1 : t);
}
TA_HD int span_origin(SpanVal v) { return (int)(v - (double)span_score(v) * kSpanUnit); }
TA_HD SpanVal span_max(SpanVal a, SpanVal b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fmax(a, b);                           // v_max_f64 (no NaN ever enters)
#else
    return a > b ? a : b;
#endif
}

// scoring constants as values (origin 0): the hatted substitution scores and the two gap opens
struct SpanConsts {
    SpanVal cmat, cmis, gox, goy;
};
TA_HD SpanConsts span_consts(const CellConsts& c, int match, int mismatch) {
    SpanConsts k;
    k.cmat = span_val(match - c.gex - c.gey, 0);
    k.cmis = span_val(mismatch - c.gex - c.gey, 0);
    k.gox = span_val(c.gox, 0);
    k.goy = span_val(c.goy, 0);
    return k;
}

// ---- boundaries ----
// Row 0 is the reference's (nw_cell.h: bnd_D_row0 / bnd_V_row0), origin 0.  Column 0 is free: bnd_D_col0 / bnd_H_col0
// with the un-hatted score 0 in place of -i, i.e. hatted -gex * i, origin i.  X(i,0) = -inf never wins (M and Y are
// finite), so it is resolved here as nw_cell.h does and no sentinel enters the kernel.
TA_HD SpanVal span_D_row0(const CellConsts& c, int j) { return span_val(raw_of(bnd_D_row0(c, j)), 0); }
TA_HD SpanVal span_V_row0(const CellConsts& c, int j) { return span_val(raw_of(bnd_V_row0(c, j)), 0); }
TA_HD SpanVal span_D_col0(const CellConsts& c, int i) { return span_val(-c.gex * i, i); }      // i = 0: D(0,0) = 0, origin 0
TA_HD SpanVal span_H_col0(const CellConsts& c, int i) {      // H~(i,0) = max(M^, Y^ - goy), both with origin i
    return span_val(-c.gex * i + (c.goy >= 0 ? 0 : -c.goy), i);
}

// ---- one interior cell: the three maxima of cell_update_raw (nw_cell.h) on values; covers every sign of the gap
// opens (3 v_add_f64 + 5 v_max_f64; the carried form would save one of the eight for non-positive opens only) ----
TA_HD void span_cell(SpanVal d_ul, SpanVal v_u, SpanVal h_l, SpanVal cs, SpanVal gox, SpanVal goy,
                     SpanVal& d, SpanVal& v, SpanVal& h) {
    const SpanVal mr = d_ul + cs;
    const SpanVal xg = v_u + gox;
    const SpanVal yg = h_l + goy;
    const SpanVal mx = span_max(mr, xg), my = span_max(mr, yg);
    d = span_max(mx, yg);
    v = span_max(my, v_u);
    h = span_max(mx, h_l);
}

// ---- a lane's state at the start of a strip and one skewed step of it: lane_boundary / lane_step of nw_cell.h on
// values (those are written for int registers; the data flow is the same, line for line) ----
template <int R, class Row = NoRow>
TA_HD void span_lane_boundary(const CellConsts& c, int row0, SpanVal (&D)[R], SpanVal (&V)[R], SpanVal (&H)[R],
                              SpanVal& dsave, Row&& row = Row()) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = row0 + r + 1;
        D[r] = span_D_col0(c, i);
        H[r] = span_H_col0(c, i);
        V[r] = 0.0;                                        // never read: a lane starts at column 1
        row(r, i);
    }
    dsave = span_D_col0(c, row0);
}
// cs(t, o) = the substitution score of the pair as a value
template <int R, class Score>
TA_HD void span_lane_step(Score&& cs, const SpanConsts& k, SpanVal (&D)[R], SpanVal (&V)[R], SpanVal (&H)[R],
                          SpanVal& dsave, SpanVal v_up, SpanVal d_next, const int (&tc)[R], int o) {
    SpanVal d_ul = dsave, v_u = v_up;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const SpanVal d_old = D[r];
        span_cell(d_ul, v_u, H[r], cs(tc[r], o), k.gox, k.goy, D[r], V[r], H[r]);
        d_ul = d_old;
        v_u = V[r];
    }
    dsave = d_next;
}

// ---- the last-column maximum ----
// best(i) = D(i, m) un-hatted.  A partial result is (score, i1, origin); `a` is better than `b` if its score is larger
// or, at equal score, its i1 SMALLER -- stated on i1 itself, so that no order of strips, lanes or waves can decide a
// tie (the origin belongs to the winner's i1 and takes no part).
struct SpanBest {
    int score, i1, origin;
};
TA_HD SpanBest span_none() { return SpanBest{kSpanNone, INT32_MAX, 0}; }
TA_HD bool span_better(const SpanBest& a, const SpanBest& b) {
    return a.score > b.score || (a.score == b.score && a.i1 < b.i1);
}
TA_HD SpanBest span_pick(const SpanBest& a, const SpanBest& b) { return span_better(b, a) ? b : a; }
TA_HD SpanBest span_row0(int m) { return SpanBest{-m, 0, 0}; }           // best(0) = M(0,m) = X(0,m) = -m
// a lane's rows after its last column: D[r] = D(row0 + r + 1, m)
template <int R>
TA_HD SpanBest span_lane_best(const CellConsts& c, int row0, int n, int m, const SpanVal (&D)[R]) {
    SpanBest b = span_none();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = row0 + r + 1;
        if (i > n) continue;
        const SpanBest mine{span_score(D[r]) + c.gex * i + c.gey * m, i, span_origin(D[r])};
        b = span_pick(b, mine);
    }
    return b;
}

}  // namespace ta
