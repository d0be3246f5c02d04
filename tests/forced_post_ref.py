"""Sum-product posteriors of a forced alignment and the text's likelihood per line, the specification of record (DESIGN.md
section 14.11) in plain Python / numpy: what csrc/ta_forced_post.hip must write, bit for bit.

The lattice, lab and the skip rule are tests/forced_ref.py's (S = 2 L + 1 <= T states; stay / advance / skip into an odd
s >= 3 with lab[s] != lab[s - 2]; start in 0, 1; end in S - 1, S - 2).  The emission is e(p) = float64(min(max(p, 2^-17),
1)) with forced_ref.q_of's two float32 comparisons in its order, so NaN, 0 and negatives give the floor.

Arithmetic: every value is a non-negative real with a 53-bit significand and an UNBOUNDED exponent; every + and * is
rounded once, to nearest-even, to 53 bits; no fused multiply-add.  So the result depends neither on when an
implementation renormalises nor on a device's denormal mode.
    forward   a_0[0] = e(P[0, 0]), a_0[1] = e(P[0, lab[1]]), 0 elsewhere.  t >= 1: y = a[s]; y = y + a[s - 1] if s >= 1;
              y = y + a[s - 2] if the skip is legal; a'[s] = y * e(P[t, lab[s]]).
    backward  b_{T-1}[s] = 1 for s in {S - 1, S - 2}, 0 elsewhere.  t = T - 1 .. 1: w[s] = b[s] * e(P[t, lab[s]]);
              b_{t-1}[s] = w[s], + w[s + 1] if s + 1 < S, + w[s + 2] if s + 2 < S, s odd and lab[s + 2] != lab[s].
    line      Z = a_{T-1}[S - 1] + a_{T-1}[S - 2].
    query     (character i, frame t): g[s] = a_t[s] * b_t[s]; own = g[2 i + 1]; rival = the largest g[s] over s != 2 i + 1,
              rival_state the smallest s that attains it.
Every output is a pair (significand in [0.5, 1) as frexp gives it, int exponent); zero is (0.0, 0).  The host forms
posterior = ldexp(own_m / z_m, own_x - z_x) and loglik_bits = log2(z_m) + z_x.

Two forms: `tables_exact` does the arithmetic in Python integers with the rounding spelled out (small lattices), `tables`
vectorised on (float64, int64) pairs: a product with e in [2^-17, 1] is a float64 multiply of normal numbers, a sum one
float64 add behind an exact ldexp of the smaller term -- a term more than SHIFT binades below the other is shifted by
SHIFT, since the add rounds it away either way.
"""
import math

import numpy as np

import forced_ref as R

QUERY = 4
# the clamp of a sum's alignment shift: far beyond the 53 bits an add keeps.  Significands here are normalised after every
# operation; csrc/ta_forced_post.hip renormalises once per chunk, so its significands spread over 150 binades and its clamp
# is 256 on purpose -- any clamp that exceeds the spread by 54 bits gives the same sums.
SHIFT = 128
ZERO_X = -(1 << 40)             # the exponent zero carries INSIDE the arithmetic, below every real one


def emission(P):
    """e(p) of float32 probabilities as float64, same shape"""
    P = np.asarray(P, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        a = np.where(P > R.FLOOR, P, R.FLOOR).astype(np.float32)
        a = np.where(a < np.float32(1), a, np.float32(1)).astype(np.float32)
    return a.astype(np.float64)


def _lattice(P, cs):
    P = np.asarray(P, dtype=np.float32)
    cs = [int(c) for c in cs]
    T, no = P.shape
    L = len(cs)
    S = 2 * L + 1
    if L < 1 or S > T or any(c < 1 or c >= no for c in cs):
        raise ValueError("forced alignment needs 1 <= L, 2 L + 1 <= T and labels in 1 .. no - 1")
    lab = R.states(cs)
    may_skip = np.zeros(S, dtype=bool)                # into s from s - 2
    may_skip[3::2] = lab[3::2] != lab[1:-2:2]
    return T, S, emission(P)[:, lab], may_skip


def _frames(frames, T):
    frames = np.arange(T) if frames is None else np.asarray(frames, dtype=np.int64).reshape(-1)
    if len(frames) and (frames.min() < 0 or frames.max() >= T):
        raise ValueError("frames inside 0 .. T - 1")
    return frames


# ---- the vectorised form ---------------------------------------------------------------------------------------------------

def _norm(y, x):
    m, e = np.frexp(y)
    return m, np.where(m == 0, ZERO_X, x + e)


def _add(m1, x1, m2, x2):
    x = np.maximum(x1, x2)
    y = np.ldexp(m1, np.maximum(x1 - x, -SHIFT)) + np.ldexp(m2, np.maximum(x2 - x, -SHIFT))
    return _norm(y, x)


def _shift(m, x, by):
    """entry s takes entry s - by (by > 0) or s + |by| (by < 0); zero where there is none"""
    zm, zx = np.zeros(abs(by)), np.full(abs(by), ZERO_X, dtype=np.int64)
    if by > 0:
        return np.concatenate((zm, m[:-by])), np.concatenate((zx, x[:-by]))
    return np.concatenate((m[-by:], zm)), np.concatenate((x[-by:], zx))


def tables(P, cs, frames=None):
    """(g_m (F, S) float64, g_x (F, S) int64, z_m, z_x) of one line: g at the frames asked for (all T by default)"""
    T, S, E, may_skip = _lattice(P, cs)
    frames = _frames(frames, T)
    keep = {}
    wanted = set(int(t) for t in frames)
    m, x = np.zeros(S), np.full(S, ZERO_X, dtype=np.int64)
    m[:2], x[:2] = _norm(E[0, :2], np.zeros(2, dtype=np.int64))
    for t in range(T):
        if t:
            ym, yx = _add(m, x, *_shift(m, x, 1))
            sm, sx = _shift(m, x, 2)
            ym, yx = _add(ym, yx, np.where(may_skip, sm, 0.0), np.where(may_skip, sx, ZERO_X))
            m, x = _norm(ym * E[t], yx)
        if t in wanted:
            keep[t] = (m, x)
    zm, zx = _add(m[S - 1:], x[S - 1:], m[S - 2:S - 1], x[S - 2:S - 1])
    skip_from = np.zeros(S, dtype=bool)               # from s to s + 2: the same edges, named by their start
    skip_from[:-2] = may_skip[2:]
    g = {}
    m, x = np.zeros(S), np.full(S, ZERO_X, dtype=np.int64)
    m[S - 2:], x[S - 2:] = 0.5, 1
    for t in range(T - 1, -1, -1):
        if t in wanted:
            am, ax = keep.pop(t)
            g[t] = _norm(am * m, ax + x)
        if t:
            wm, wx = _norm(m * E[t], x)
            ym, yx = _add(wm, wx, *_shift(wm, wx, -1))
            sm, sx = _shift(wm, wx, -2)
            m, x = _add(ym, yx, np.where(skip_from, sm, 0.0), np.where(skip_from, sx, ZERO_X))
    gm = np.stack([g[int(t)][0] for t in frames]) if len(frames) else np.zeros((0, S))
    gx = np.stack([g[int(t)][1] for t in frames]) if len(frames) else np.zeros((0, S), dtype=np.int64)
    return gm, np.where(gm == 0, 0, gx), float(zm[0]), int(zx[0])


# ---- the exact form: (M, E) = M 2^E with M = 0 or 2^52 <= M < 2^53, Python integers -----------------------------------------

def _round53(M, E):
    if M == 0:
        return 0, 0
    n = M.bit_length()
    if n <= 53:
        return M << (53 - n), E - (53 - n)
    sh = n - 53
    q, r, half = M >> sh, M & ((1 << sh) - 1), 1 << (sh - 1)
    if r > half or (r == half and (q & 1)):           # to nearest, ties to even
        q += 1
        if q == 1 << 53:
            q, sh = q >> 1, sh + 1
    return q, E + sh


def _of_float(v):
    m, x = math.frexp(float(v))
    return _round53(int(m * (1 << 53)), x - 53)


def _add_exact(a, b):
    if a[0] == 0 or b[0] == 0:
        return a if b[0] == 0 else b
    e = min(a[1], b[1])
    return _round53((a[0] << (a[1] - e)) + (b[0] << (b[1] - e)), e)


def _mul_exact(a, b):
    return _round53(a[0] * b[0], a[1] + b[1])


def _pair(v):
    """(M, E) -> (significand in [0.5, 1), exponent); zero is (0.0, 0)"""
    return (v[0] / float(1 << 53), v[1] + 53) if v[0] else (0.0, 0)


def tables_exact(P, cs, frames=None):
    """`tables` with the arithmetic in Python integers: the rule itself, for small lattices"""
    T, S, E, may_skip = _lattice(P, cs)
    frames = _frames(frames, T)
    E = [[_of_float(v) for v in row] for row in E]
    zero = (0, 0)
    a = [E[0][0], E[0][1]] + [zero] * (S - 2)
    A = [a]
    for t in range(1, T):
        nxt = []
        for s in range(S):
            y = a[s]
            if s >= 1:
                y = _add_exact(y, a[s - 1])
            if may_skip[s]:
                y = _add_exact(y, a[s - 2])
            nxt.append(_mul_exact(y, E[t][s]))
        a = nxt
        A.append(a)
    z = _add_exact(a[S - 1], a[S - 2])
    one = _of_float(1.0)
    b = [zero] * (S - 2) + [one, one]
    B = [None] * T
    B[T - 1] = b
    for t in range(T - 1, 0, -1):
        w = [_mul_exact(b[s], E[t][s]) for s in range(S)]
        nxt = []
        for s in range(S):
            y = w[s]
            if s + 1 < S:
                y = _add_exact(y, w[s + 1])
            if s + 2 < S and may_skip[s + 2]:
                y = _add_exact(y, w[s + 2])
            nxt.append(y)
        b = nxt
        B[t - 1] = b
    gm, gx = np.zeros((len(frames), S)), np.zeros((len(frames), S), dtype=np.int64)
    for k, t in enumerate(frames):
        for s in range(S):
            gm[k, s], gx[k, s] = _pair(_mul_exact(A[t][s], B[t][s]))
    zm, zx = _pair(z)
    return gm, gx, zm, zx


# ---- queries, and the two formulas the host applies --------------------------------------------------------------------------

def query_tables(gm, gx, rows=None):
    """(own_m, own_x, rival_m, rival_x, rival_state) of character i on row rows[i] (row i by default) of a line's g"""
    S = gm.shape[1]
    L = (S - 1) // 2
    rows = np.arange(L) if rows is None else np.asarray(rows, dtype=np.int64)
    if len(rows) != L:
        raise ValueError("a row per character")
    gm, gx = gm[rows].copy(), gx[rows].copy()
    at = np.arange(L)
    own_m, own_x = gm[at, 2 * at + 1].copy(), gx[at, 2 * at + 1].copy()
    key = np.where(gm == 0, ZERO_X, gx)               # by exponent, then significand, then the smaller state
    key[at, 2 * at + 1] = 2 * ZERO_X                  # the own state is no rival
    gm[at, 2 * at + 1] = -1.0
    best_x = key.max(axis=1, keepdims=True)
    best_m = np.where(key == best_x, gm, -1.0).max(axis=1, keepdims=True)
    rival = ((key == best_x) & (gm == best_m)).argmax(axis=1)
    return (own_m, own_x.astype(np.int32), gm[at, rival], gx[at, rival].astype(np.int32), rival.astype(np.int32))


def query(P, cs, tq):
    """{own_m, own_x, rival_m, rival_x, rival_state (L,), z_m, z_x} of one line for the query frames tq"""
    tq = [int(t) for t in tq]
    if len(tq) != len(cs):
        raise ValueError("a query frame per character")
    gm, gx, zm, zx = tables(P, cs, tq)
    out = dict(zip(("own_m", "own_x", "rival_m", "rival_x", "rival_state"), query_tables(gm, gx)))
    out.update(z_m=zm, z_x=zx)
    return out


PER_LABEL = ("own_m", "own_x", "rival_m", "rival_x", "rival_state")
PER_LINE = ("z_m", "z_x")
DTYPES = dict(own_m=np.float64, own_x=np.int32, rival_m=np.float64, rival_x=np.int32, rival_state=np.int32, z_m=np.float64,
              z_x=np.int32)


def query_batch(lines, queries):
    """[(P, cs)], [tq] -> the seven outputs, the per-label ones line after line, the per-line ones one per line"""
    got = [query(P, cs, tq) for (P, cs), tq in zip(lines, queries)]
    out = {k: np.concatenate([g[k] for g in got]).astype(DTYPES[k]) if got else np.zeros(0, DTYPES[k]) for k in PER_LABEL}
    out.update({k: np.asarray([g[k] for g in got], dtype=DTYPES[k]) for k in PER_LINE})
    return out


def posterior(m, x, z_m, z_x):
    """ldexp(m / z_m, x - z_x): the posterior of a state's (m, x) under a line's (z_m, z_x)"""
    return np.ldexp(np.asarray(m, dtype=np.float64) / z_m, np.asarray(x, dtype=np.int64) - z_x)


def loglik_bits(z_m, z_x):
    """log2 P(text | line) = log2(z_m) + z_x"""
    return np.log2(np.asarray(z_m, dtype=np.float64)) + z_x


def same_bits(a, b):
    """float64 arrays equal word for word"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
