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

// ---- the CHAINED search (ta_nw_span_chain; DESIGN.md section 4.6.1, checker tests/span_chain_ref.py) ----
// The pages of a book in reading order in one transcript: page p's fill is the one above with a CARRY G'(i) -- the
// renormalised prefix maximum of the previous page's last column, -floor <= G' <= 0 -- where column 0 and row 0 have
// the free 0.  The carry is a score offset on the boundary values, origins as above; the interior is untouched.
// Every row's last-column (F, origin) goes to HBM, row i at slot i + kSpanChainPad of its page's arrays, so that the
// R = 4 rows of a lane (row0 + 1 .., row0 a multiple of 4) lie at a multiple of 16 bytes.
constexpr int kSpanChainPad = 3;
TA_HD int64_t span_chain_stride(int max_n) { return ((int64_t)max_n + 1 + kSpanChainPad + 3) & ~(int64_t)3; }
struct alignas(16) SpanI4 {
    int32_t x, y, z, w;
};

TA_HD bool span_consts_fit(const SpanConsts& k) {           // the substitution constants' low dwords are zero
    uint64_t a, b;
    __builtin_memcpy(&a, &k.cmat, 8);
    __builtin_memcpy(&b, &k.cmis, 8);
    return (uint32_t)(a | b) == 0;
}
// a chain the kernels refuse as a whole: sizes beyond what the call was made for, parameters beyond the carrier
TA_HD bool span_chain_fits(const SpanConsts& k, int n, int m, int max_n, int max_m) {
    return n >= 0 && n <= max_n && m >= 0 && m <= max_m && span_consts_fit(k);
}

// row 0 with the carry: M(0,j) = X(0,j) = G'(0) - j
TA_HD SpanVal span_D_row0(const CellConsts& c, int j, int g0) { return span_D_row0(c, j) + span_val(g0, 0); }
TA_HD SpanVal span_V_row0(const CellConsts& c, int j, int g0) { return span_V_row0(c, j) + span_val(g0, 0); }
// column 0 with the carry: M(i,0) = Y(i,0) = G'(i), origin i; carry(i) = G'(i) for 0 <= i <= n, anything finite below
template <int R, class Carry, class Row = NoRow>
TA_HD void span_lane_boundary_chain(const CellConsts& c, int row0, SpanVal (&D)[R], SpanVal (&V)[R], SpanVal (&H)[R],
                                    SpanVal& dsave, Carry&& carry, Row&& row = Row()) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = row0 + r + 1;
        const SpanVal g = span_val(carry(i), 0);
        D[r] = span_D_col0(c, i) + g;
        H[r] = span_H_col0(c, i) + g;
        V[r] = 0.0;
        row(r, i);
    }
    dsave = span_D_col0(c, row0) + span_val(carry(row0), 0);
}
// a lane's rows after its last column -> F(i) = D(i, m) un-hatted and its origin, rows i <= n only; F and O point at
// slot 0 of the page's arrays.  A lane with R = 4 rows inside the table stores them as one 16-byte vector each.
template <int R>
TA_HD void span_store_last(const CellConsts& c, int row0, int n, int m, const SpanVal (&D)[R], int32_t* F, int32_t* O) {
    int32_t f[R], g[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = row0 + r + 1;
        f[r] = span_score(D[r]) + c.gex * i + c.gey * m;
        g[r] = span_origin(D[r]);
    }
    const int slot = row0 + 1 + kSpanChainPad;
    if constexpr (R == 4) {
        if (row0 + R <= n) {
            *reinterpret_cast<SpanI4*>(F + slot) = SpanI4{f[0], f[1], f[2], f[3]};
            *reinterpret_cast<SpanI4*>(O + slot) = SpanI4{g[0], g[1], g[2], g[3]};
            return;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (row0 + r + 1 <= n) { F[slot + r] = f[r]; O[slot + r] = g[r]; }
}
// the rows a fill has no table for: m = 0 gives F(i) = G'(i) with origin i; row 0 gives G'(0) - m with origin 0
TA_HD void span_trivial_last(int i, int m, int g, int32_t* F, int32_t* O) {
    F[i + kSpanChainPad] = g - m;
    O[i + kSpanChainPad] = i;
}

// ---- the carry: G'(i) = max(max_{j <= i} F(j) - top, -floor) ----
constexpr int kSpanCarryPer = 4;                            // consecutive rows per lane and tile of the prefix maximum
TA_HD int span_imax(int a, int b) { return a > b ? a : b; }
TA_HD int span_carry_value(int prefix_max, int top, int floor) { return span_imax(prefix_max - top, -floor); }
// a lane's kSpanCarryPer rows from row `first` on: their values (kSpanNone past row n) and the largest
TA_HD int span_carry_load(const int32_t* F, int first, int n, int (&v)[kSpanCarryPer]) {
    int mx = kSpanNone;
#pragma unroll
    for (int q = 0; q < kSpanCarryPer; ++q) {
        v[q] = (first + q <= n) ? F[first + q + kSpanChainPad] : kSpanNone;
        mx = span_imax(mx, v[q]);
    }
    return mx;
}
// ... and their carry values, `before` = the maximum of every row in front of the lane's
TA_HD void span_carry_store(int32_t* G, int first, int n, const int (&v)[kSpanCarryPer], int before, int top, int floor) {
    int run = before;
#pragma unroll
    for (int q = 0; q < kSpanCarryPer; ++q) {
        run = span_imax(run, v[q]);
        if (first + q <= n) G[first + q + kSpanChainPad] = span_carry_value(run, top, floor);
    }
}

// ---- the walk back: among the rows j <= limit the largest F, at equal F the SMALLEST j -- stated on the values, as
// span_better is, so that no order of lanes or waves decides a tie ----
struct SpanWalk {
    int f, j;
};
TA_HD SpanWalk span_walk_none() { return SpanWalk{kSpanNone, INT32_MAX}; }
TA_HD SpanWalk span_walk_pick(const SpanWalk& a, const SpanWalk& b) {
    return (b.f > a.f || (b.f == a.f && b.j < a.j)) ? b : a;
}
// one lane's share of a page: rows lane, lane + nlanes, ... up to limit
TA_HD SpanWalk span_walk_lane(const int32_t* F, int limit, int lane, int nlanes) {
    SpanWalk w = span_walk_none();
    for (int j = lane; j <= limit; j += nlanes) w = span_walk_pick(w, SpanWalk{F[j + kSpanChainPad], j});
    return w;
}
// the page's result from the winning row: (i0, i1, score), score = F(i1) - G'_{p-1}(i0); Gprev = NULL on page 0
TA_HD void span_walk_result(const SpanWalk& w, const int32_t* O, const int32_t* Gprev, int32_t* out3) {
    int i0 = O[w.j + kSpanChainPad];
    i0 = i0 < 0 ? 0 : (i0 > w.j ? w.j : i0);               // an origin never lies outside 0 .. i1: no index leaves the arrays
    out3[0] = i0;
    out3[1] = w.j;
    out3[2] = w.f - (Gprev ? Gprev[i0 + kSpanChainPad] : 0);
}

}  // namespace ta
