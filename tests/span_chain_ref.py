"""tests/span_chain_ref.py -- the checker of the CHAINED span search (TEST INFRASTRUCTURE ONLY).

The pages o_0 .. o_{P-1} of a book, in reading order, in ONE transcript t[0..n): page p's tables M, X, Y are those of
tests/span_ref.py (same interior recurrence, same origin rule: at equal score the larger origin) with a CARRY G'_{p-1}
where the single search has the free 0:

  column 0   M(i,0) = Y(i,0) = G'_{p-1}(i), origin i (i >= 1);  X(i,0) = -inf
  row 0      M(0,j) = X(0,j) = G'_{p-1}(0) - j, origin 0
  G'_{-1} = 0: page 0 is the single search's fill.

  F_p(i) = the largest of the three at (i, m_p), org_p(i) its origin;  top_p = max_i F_p(i)
  G'_p(i) = max( max_{j <= i} F_p(j) - top_p, -floor )

and the walk back from limit = n, p = P-1 .. 0:  i1_p = the smallest j <= limit with the largest F_p(j' <= limit),
i0_p = org_p(i1_p), score_p = F_p(i1_p) - G'_{p-1}(i0_p), limit = i0_p.  Integers only.

  chain_plain   plain Python on span_ref's (score, origin) pairs
  chain_numpy   int64 values score * 2^32 + origin along anti-diagonals, as span_ref.span_numpy

Both return (spans, total, bound): spans = [(i0, i1, score)] per page, total = the sum of the scores, bound = whether
the floor's clamp changed any carry value.
"""
import numpy as np

from span_ref import _NEG, _add, _params


def _fill_carry(t, o, params, G):
    """span_ref._fill's tables with the carry G[0 .. n] on column 0 and row 0"""
    match, mismatch, gox, goy, gex, gey = _params(params)
    n, m = len(t), len(o)
    M = [[_NEG] * (m + 1) for _ in range(n + 1)]
    X = [[_NEG] * (m + 1) for _ in range(n + 1)]
    Y = [[_NEG] * (m + 1) for _ in range(n + 1)]
    for j in range(m + 1):
        M[0][j] = X[0][j] = (G[0] - j, 0)
    for i in range(1, n + 1):
        M[i][0] = Y[i][0] = (G[i], i)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            s = match if t[i - 1] == o[j - 1] else mismatch
            M[i][j] = _add(max(M[i - 1][j - 1], X[i - 1][j - 1], Y[i - 1][j - 1]), s)
            X[i][j] = max(_add(M[i - 1][j], gox + gex), _add(X[i - 1][j], gex), _add(Y[i - 1][j], gox + gex))
            Y[i][j] = max(_add(M[i][j - 1], goy + gey), _add(X[i][j - 1], goy + gey), _add(Y[i][j - 1], gey))
    return M, X, Y


def last_column_plain(t, o, params, G):
    """(F, org): lists of n + 1 ints"""
    n, m = len(t), len(o)
    M, X, Y = _fill_carry(t, o, params, G)
    best = [max(M[i][m], X[i][m], Y[i][m]) for i in range(n + 1)]
    return [b[0] for b in best], [b[1] for b in best]


def last_column_numpy(t, o, params, G):
    """(F, org): int64 arrays of n + 1"""
    match, mismatch, gox, goy, gex, gey = _params(params)
    t = np.asarray(t, dtype=np.int64)
    o = np.asarray(o, dtype=np.int64)
    G = np.asarray(G, dtype=np.int64)
    n, m = len(t), len(o)
    SH = np.int64(1) << np.int64(32)
    NEG = -(np.int64(1) << np.int64(60))
    rows = np.arange(n + 1, dtype=np.int64)
    if m == 0:
        return G.copy(), rows
    best = np.full(n + 1, NEG, dtype=np.int64)
    best[0] = (G[0] - m) * SH
    if n > 0:
        def boundary(d):
            Md, Xd, Yd = (np.full(n + 1, NEG, dtype=np.int64) for _ in range(3))
            if d <= m:
                Md[0] = Xd[0] = (G[0] - d) * SH
            if 1 <= d <= n:
                Md[d] = Yd[d] = G[d] * SH + d
            return Md, Xd, Yd

        prev2, prev1 = boundary(0), boundary(1)
        for d in range(2, n + m + 1):
            Md, Xd, Yd = boundary(d)
            lo, hi = max(1, d - m), min(n, d - 1)
            if lo <= hi:
                i = np.arange(lo, hi + 1)
                s = np.where(t[i - 1] == o[d - i - 1], match, mismatch).astype(np.int64) * SH
                M2, X2, Y2 = prev2
                Md[i] = np.maximum(np.maximum(M2[i - 1], X2[i - 1]), Y2[i - 1]) + s
                M1, X1, Y1 = prev1
                Yd[i] = np.maximum(np.maximum(M1[i] + (goy + gey) * SH, X1[i] + (goy + gey) * SH), Y1[i] + gey * SH)
                Xd[i] = np.maximum(np.maximum(M1[i - 1] + (gox + gex) * SH, X1[i - 1] + gex * SH),
                                   Y1[i - 1] + (gox + gex) * SH)
            if 1 <= d - m <= n:
                ii = d - m
                best[ii] = max(Md[ii], Xd[ii], Yd[ii])
            prev2, prev1 = prev1, (Md, Xd, Yd)
    return best >> np.int64(32), best & np.int64(0xFFFFFFFF)


def carry(F, floor):
    """(G', bound): the renormalised prefix maximum of one page's last column, and whether the floor changed a value"""
    F = np.asarray(F, dtype=np.int64)
    rel = np.maximum.accumulate(F) - F.max()
    return np.maximum(rel, -int(floor)), bool((rel < -int(floor)).any())


def _chain(last_column, t, pages, params, floor):
    if floor <= 0:
        raise ValueError("floor must be positive")
    n = len(t)
    carries = [np.zeros(n + 1, dtype=np.int64)]
    cols, bound = [], False
    for o in pages:
        F, org = last_column(t, o, params, [int(v) for v in carries[-1]])
        cols.append((np.asarray(F, dtype=np.int64), np.asarray(org, dtype=np.int64)))
        g, b = carry(F, floor)
        carries.append(g)
        bound = bound or b
    spans, limit = [None] * len(pages), n
    for p in range(len(pages) - 1, -1, -1):
        F, org = cols[p]
        i1 = int(np.argmax(F[:limit + 1]))                 # the first maximum: the smallest row
        i0 = int(org[i1])
        spans[p] = (i0, i1, int(F[i1] - carries[p][i0]))
        limit = i0
    return spans, sum(s[2] for s in spans), bound


def chain_plain(t, pages, params, floor):
    return _chain(last_column_plain, list(t), [list(o) for o in pages], params, floor)


def chain_numpy(t, pages, params, floor):
    return _chain(last_column_numpy, t, pages, params, floor)
