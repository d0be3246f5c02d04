"""tests/span_ref.py -- the checker of the span-locating fill (TEST INFRASTRUCTURE ONLY).

Where in a longer transcript t[0..n) does the text o[0..m) of a page lie?  The definition of record, three times:

  span_origins   plain Python: the affine-gap tables M, X, Y of the reference (interior recurrence textSeqCompare.py:62-88,
                 row-0 boundary :57-60) with a FREE column 0 (M = Y = 0, X = -inf for i >= 1) in which every value carries
                 an origin -- 0 on row 0, i at (i, 0), inherited from the candidate taken; candidates are ordered by score
                 and, at equal score, by the larger origin.  best(i) = max of the three at (i, m); i1 = the smallest i with
                 the maximal score, i0 = the origin of best(i1).
  span_enumerate plain Python without origins: S(i0, i1) = the best score from (i0, 0) to (i1, m) when column 0 below i0 is
                 unreachable; the answer maximises S, then takes the smallest i1, then the largest i0.
  span_numpy     the first statement on int64 values score * 2^32 + origin along anti-diagonals (np.maximum is then the
                 lexicographic maximum), for shapes the plain forms are too slow for.

All return (i0, i1, score).  snap_to_words is the page-level rule that widens a span to whole words.
"""
import numpy as np

_NEG = (-(10 ** 18), -1)          # -inf with an origin that loses every tie


def _add(v, k):
    return v if v is _NEG else (v[0] + k, v[1])


def _params(params):
    match, mismatch, gox, goy, gex, gey = (int(v) for v in params)
    return match, mismatch, gox, goy, gex, gey


def _fill(t, o, params, i_start, free_below):
    """tables of (score, origin) from row i_start on; free_below: column 0 is free on every row (else only at i_start)"""
    match, mismatch, gox, goy, gex, gey = _params(params)
    n, m = len(t), len(o)
    M = [[_NEG] * (m + 1) for _ in range(n + 1)]
    X = [[_NEG] * (m + 1) for _ in range(n + 1)]
    Y = [[_NEG] * (m + 1) for _ in range(n + 1)]
    if i_start == 0:
        for j in range(m + 1):
            M[0][j] = X[0][j] = (-j, 0)
    else:
        M[i_start][0] = Y[i_start][0] = (0, i_start)
    if free_below:
        for i in range(max(i_start, 1), n + 1):
            M[i][0] = Y[i][0] = (0, i)
    first = i_start + 1 if i_start == 0 else i_start      # a start at (i0, 0), i0 >= 1, is an ordinary column-0 cell of its row
    for i in range(max(first, 1), n + 1):
        for j in range(1, m + 1):
            s = match if t[i - 1] == o[j - 1] else mismatch
            if i - 1 >= i_start:
                M[i][j] = _add(max(M[i - 1][j - 1], X[i - 1][j - 1], Y[i - 1][j - 1]), s)
                X[i][j] = max(_add(M[i - 1][j], gox + gex), _add(X[i - 1][j], gex), _add(Y[i - 1][j], gox + gex))
            Y[i][j] = max(_add(M[i][j - 1], goy + gey), _add(X[i][j - 1], goy + gey), _add(Y[i][j - 1], gey))
    return M, X, Y


def span_origins(t, o, params):
    n, m = len(t), len(o)
    M, X, Y = _fill(t, o, params, 0, True)
    best = [max(M[i][m], X[i][m], Y[i][m]) for i in range(n + 1)]
    top = max(b[0] for b in best)
    i1 = min(i for i in range(n + 1) if best[i][0] == top)
    return best[i1][1], i1, top


def span_enumerate(t, o, params):
    n, m = len(t), len(o)
    answer = None
    for i0 in range(n + 1):
        M, X, Y = _fill(t, o, params, i0, False)
        for i1 in range(i0, n + 1):
            sc = max(M[i1][m], X[i1][m], Y[i1][m])[0]
            if sc <= _NEG[0] // 2:
                continue
            key = (sc, -i1, i0)
            if answer is None or key > answer:
                answer = key
    return answer[2], -answer[1], answer[0]


def span_numpy(t, o, params):
    match, mismatch, gox, goy, gex, gey = _params(params)
    t = np.asarray(t, dtype=np.int64)
    o = np.asarray(o, dtype=np.int64)
    n, m = len(t), len(o)
    if m == 0:
        return 0, 0, 0
    if n == 0:
        return 0, 0, -m
    SH = np.int64(1) << np.int64(32)
    NEG = -(np.int64(1) << np.int64(60))

    def boundary(d):
        Md, Xd, Yd = (np.full(n + 1, NEG, dtype=np.int64) for _ in range(3))
        if d <= m:
            Md[0] = Xd[0] = -d * SH
        if 1 <= d <= n:
            Md[d] = Yd[d] = d               # score 0, origin d
        return Md, Xd, Yd

    best = np.full(n + 1, NEG, dtype=np.int64)
    best[0] = -m * SH
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
            Xd[i] = np.maximum(np.maximum(M1[i - 1] + (gox + gex) * SH, X1[i - 1] + gex * SH), Y1[i - 1] + (gox + gex) * SH)
        if 1 <= d - m <= n:
            ii = d - m
            best[ii] = max(Md[ii], Xd[ii], Yd[ii])
        prev2, prev1 = prev1, (Md, Xd, Yd)
    score = best >> np.int64(32)
    i1 = int(np.argmax(score))              # the first maximum: the smallest i1
    return int(best[i1] & np.int64(0xFFFFFFFF)), i1, int(score[i1])


def snap_to_words(tr, i0, i1):
    """(i0, i1) from the fill -> (a, b), indices into the transcript string as passed: outward to whole words; a span
    of nothing but spaces is empty"""
    while i0 < i1 and tr[i0] == ' ':
        i0 += 1
    while i1 > i0 and tr[i1 - 1] == ' ':
        i1 -= 1
    if i0 == i1:
        return i0, i0
    a = tr.rfind(' ', 0, i0) + 1
    b = tr.find(' ', i1)
    b = len(tr) if b < 0 else b
    return a, b
