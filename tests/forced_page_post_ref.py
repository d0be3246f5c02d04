"""Sum-product posteriors at page scope and the page's likelihood, the specification of record
in plain Python / numpy: what csrc/ta_forced_page_post.hip must write, bit for bit.

The lattice is tests/forced_page_ref.py's, unchanged: the page's labels cs[0 .. n) give the states s = 0 .. 2 n (lab[s] as
forced_ref.states), the windows [lo_k, hi_k) must satisfy windows_ok, during line k only the states 2 lo_k .. 2 hi_k are
live, the frames are ordered (k, t), line after line, a skip into an odd s >= 3 is legal iff lab[s] != lab[s - 2], and a
label state has no stay over a line break.  The emission e(p) and the arithmetic are tests/forced_post_ref.py's, unchanged:
every value a pair (53-bit significand, unbounded integer exponent), every + and * rounded once to nearest-even, no fused
multiply-add, and adding the pair zero returns the other term bit for bit.
    forward   frame (0, 0): a[0] = e(P_0[0, 0]), a[1] = e(P_0[0, lab[1]]), 0 elsewhere.  Every later frame (k, t): y = a[s]
              -- absent for odd s when t = 0 (then k >= 1) --, then + a[s - 1] if s >= 1, then + a[s - 2] if the skip is
              legal; a'[s] = y * e(P_k[t, lab[s]]).  After every frame, (0, 0) included, a state that is not live in
              line k is exactly zero.
    page      Z = a_last[2 n] + a_last[2 n - 1].  Z = 0 exactly: the page has no legal path (every emission is >= 2^-17 and
              exponents are unbounded, so this is topological); status NOPATH, as forced_page_ref.align_page's.
    backward  at the page's last frame b[s] = 1 for s in {2 n, 2 n - 1}, masked to the last window's live states, 0
              elsewhere.  For a frame f with the successor f' = (k', t'): w[s'] = b_f'[s'] * e(P_k'[t', lab[s']]);
              b_f[s] = w[s] -- absent for odd s when t' = 0 --, then + w[s + 1] if s + 1 <= 2 n, then + w[s + 2] if
              s + 2 <= 2 n, s odd and lab[s + 2] != lab[s]; then masked to exact zero outside the live states of f's line.
    query     character i at a frame (k, t) with lo_k <= i < hi_k, the queries never decreasing in (k, t) order as i grows
              (forced_page_conf_ref.queries_ok): g[s] = a_f[s] * b_f[s], one product; own = g[2 i + 1]; rival = the
              largest g[s] over the live states s != 2 i + 1 of line k, ordered by exponent, then significand;
              rival_state the smallest such PAGE state that attains it -- 2 lo_k with rival = (0.0, 0) where every rival
              is zero.
Every output is a pair as frexp gives it, zero is (0.0, 0).  The host forms posterior = ldexp(own_m / z_m, own_x - z_x) and
page_loglik_bits = log2(z_m) + z_x (forced_post_ref.posterior / loglik_bits).  A page has at most MAX_FRAMES = 2^24 frames:
a and b at one frame cover disjoint frames, so every real exponent, g's included, lies above -17 * 2^24 - 2.

Two forms, as forced_post_ref has: `tables_exact` in Python integers with the rounding spelled out (small lattices),
`tables` vectorised on (float64, int64) pairs.  `line_stay=True` drops the rule of the line break: a restatement for
comparison, not the rule.
"""
import numpy as np

import forced_page_conf_ref as CR
import forced_page_ref as PR
import forced_post_ref as R
import forced_ref as FR
from forced_post_ref import ZERO_X, _add, _add_exact, _mul_exact, _norm, _of_float, _pair, _shift  # noqa: F401

OK, BOUNDS, LABEL, NOPATH, QUERY = PR.OK, PR.BOUNDS, PR.LABEL, PR.NOPATH, R.QUERY
MAX_FRAMES = 1 << 24
PER_LABEL, PER_PAGE, DTYPES = R.PER_LABEL, R.PER_LINE, R.DTYPES
queries_ok = CR.queries_ok


def _lattice(Ps, cs, lo, hi):
    cs = [int(c) for c in cs]
    n, nl = len(cs), len(Ps)
    Ps = [np.asarray(p, dtype=np.float32) for p in Ps]
    if n < 1 or nl < 1 or len(lo) != nl or len(hi) != nl or not PR.windows_ok(lo, hi, n) or any(len(p) < 1 for p in Ps):
        raise ValueError("windows")
    no = Ps[0].shape[1]
    if any(c < 1 or c >= no for c in cs):
        raise ValueError("labels")
    if sum(len(p) for p in Ps) > MAX_FRAMES:
        raise ValueError("frames")
    lab = FR.states(cs)
    S = 2 * n + 1
    may_skip = np.zeros(S, dtype=bool)                # into s from s - 2
    may_skip[3::2] = lab[3::2] != lab[1:-2:2]
    skip_from = np.zeros(S, dtype=bool)               # from s to s + 2: the same edges, named by their start
    skip_from[:-2] = may_skip[2:]
    live = np.zeros((nl, S), dtype=bool)
    for k in range(nl):
        live[k, 2 * int(lo[k]):2 * int(hi[k]) + 1] = True
    E = [R.emission(p)[:, lab] for p in Ps]
    return S, E, may_skip, skip_from, live


# ---- the vectorised form ---------------------------------------------------------------------------------------------------

def tables(Ps, cs, lo, hi, line_stay=False):
    """(g_m, g_x, z_m, z_x): g per line as (T_k, 2 n + 1) float64 / int64 arrays, Z a pair; (0.0, 0) is NOPATH"""
    S, E, may_skip, skip_from, live = _lattice(Ps, cs, lo, hi)
    nl = len(E)
    odd = np.arange(S) % 2 == 1
    zx = lambda: np.full(S, ZERO_X, dtype=np.int64)   # noqa: E731
    A = [(np.zeros((len(e), S)), np.zeros((len(e), S), dtype=np.int64)) for e in E]
    m, x = np.zeros(S), zx()
    for k in range(nl):
        for t in range(len(E[k])):
            if k == 0 and t == 0:
                m[:2], x[:2] = _norm(E[0][0, :2], np.zeros(2, dtype=np.int64))
            else:
                drop = odd & (t == 0) & (not line_stay)
                ym, yx = _add(np.where(drop, 0.0, m), np.where(drop, ZERO_X, x), *_shift(m, x, 1))
                sm, sx = _shift(m, x, 2)
                ym, yx = _add(ym, yx, np.where(may_skip, sm, 0.0), np.where(may_skip, sx, ZERO_X))
                m, x = _norm(ym * E[k][t], yx)
            m, x = np.where(live[k], m, 0.0), np.where(live[k], x, ZERO_X)
            A[k][0][t], A[k][1][t] = m, x
    z_m, z_x = _add(m[S - 1:], x[S - 1:], m[S - 2:S - 1], x[S - 2:S - 1])
    gm = [np.zeros((len(e), S)) for e in E]
    gx = [np.zeros((len(e), S), dtype=np.int64) for e in E]
    m, x = np.zeros(S), zx()
    m[S - 2:], x[S - 2:] = 0.5, 1
    m, x = np.where(live[nl - 1], m, 0.0), np.where(live[nl - 1], x, ZERO_X)
    order = [(k, t) for k in range(nl) for t in range(len(E[k]))]
    for f in range(len(order) - 1, -1, -1):
        k, t = order[f]
        if f + 1 < len(order):
            k2, t2 = order[f + 1]
            wm, wx = _norm(m * E[k2][t2], x)
            drop = odd & (t2 == 0) & (not line_stay)
            ym, yx = _add(np.where(drop, 0.0, wm), np.where(drop, ZERO_X, wx), *_shift(wm, wx, -1))
            sm, sx = _shift(wm, wx, -2)
            m, x = _add(ym, yx, np.where(skip_from, sm, 0.0), np.where(skip_from, sx, ZERO_X))
            m, x = np.where(live[k], m, 0.0), np.where(live[k], x, ZERO_X)
        pm, px = _norm(A[k][0][t] * m, A[k][1][t] + x)
        gm[k][t], gx[k][t] = pm, np.where(pm == 0, 0, px)
    return gm, gx, float(z_m[0]), (int(z_x[0]) if z_m[0] != 0 else 0)


# ---- the exact form: forced_post_ref's (M, E) = M 2^E in Python integers -----------------------------------------------------

def tables_exact(Ps, cs, lo, hi, line_stay=False):
    """`tables` with the arithmetic in Python integers: the rule itself, for small lattices"""
    S, E, may_skip, skip_from, live = _lattice(Ps, cs, lo, hi)
    nl = len(E)
    E = [[[_of_float(v) for v in row] for row in e] for e in E]
    zero = (0, 0)
    order = [(k, t) for k in range(nl) for t in range(len(E[k]))]
    a = [E[0][0][0], E[0][0][1]] + [zero] * (S - 2)
    A = []
    for f, (k, t) in enumerate(order):
        if f:
            nxt = []
            for s in range(S):
                y = zero if (s % 2 == 1 and t == 0 and not line_stay) else a[s]
                if s >= 1:
                    y = _add_exact(y, a[s - 1])
                if may_skip[s]:
                    y = _add_exact(y, a[s - 2])
                nxt.append(_mul_exact(y, E[k][t][s]))
            a = nxt
        a = [a[s] if live[k][s] else zero for s in range(S)]
        A.append(a)
    z = _add_exact(a[S - 1], a[S - 2])
    one = _of_float(1.0)
    b = [one if s >= S - 2 and live[nl - 1][s] else zero for s in range(S)]
    gm = [np.zeros((len(e), S)) for e in E]
    gx = [np.zeros((len(e), S), dtype=np.int64) for e in E]
    for f in range(len(order) - 1, -1, -1):
        k, t = order[f]
        if f + 1 < len(order):
            k2, t2 = order[f + 1]
            w = [_mul_exact(b[s], E[k2][t2][s]) for s in range(S)]
            nxt = []
            for s in range(S):
                y = zero if (s % 2 == 1 and t2 == 0 and not line_stay) else w[s]
                if s + 1 < S:
                    y = _add_exact(y, w[s + 1])
                if s + 2 < S and skip_from[s]:
                    y = _add_exact(y, w[s + 2])
                nxt.append(y if live[k][s] else zero)
            b = nxt
        for s in range(S):
            gm[k][t, s], gx[k][t, s] = _pair(_mul_exact(A[f][s], b[s]))
    z_m, z_x = _pair(z)
    return gm, gx, z_m, z_x


# ---- queries ---------------------------------------------------------------------------------------------------------------------

def query_tables(gm, gx, lo, hi, q_line, q_t):
    """(own_m, own_x, rival_m, rival_x, rival_state) (n,) of the queries (q_line[i], q_t[i]) for character i on a page's
    g.  ValueError for queries the kernel refuses (TA_FORCED_QUERY)."""
    n = (gm[0].shape[1] - 1) // 2
    if len(q_line) != n or len(q_t) != n or not queries_ok(q_line, q_t, [len(g) for g in gm], lo, hi):
        raise ValueError("queries")
    out = {name: np.zeros(n, DTYPES[name]) for name in PER_LABEL}
    for i in range(n):
        k, t = int(q_line[i]), int(q_t[i])
        a, b = 2 * int(lo[k]), 2 * int(hi[k]) + 1
        m, x = gm[k][t, a:b].copy(), gx[k][t, a:b].copy()
        own = 2 * i + 1 - a
        out["own_m"][i], out["own_x"][i] = m[own], x[own]
        key = np.where(m == 0, ZERO_X, x)             # by exponent, then significand, then the smaller state
        key[own] = 2 * ZERO_X                         # the own state is no rival
        m[own] = -1.0
        r = int(((key == key.max()) & (m == np.where(key == key.max(), m, -1.0).max())).argmax())
        out["rival_m"][i], out["rival_x"][i], out["rival_state"][i] = m[r], x[r], a + r
    return tuple(out[name] for name in PER_LABEL)


def query(Ps, cs, lo, hi, q_line, q_t, exact=False):
    """{status, own_m, own_x, rival_m, rival_x, rival_state (n,), z_m, z_x} of one page; a page without a path: status
    NOPATH alone.  The queries are checked either way."""
    gm, gx, z_m, z_x = (tables_exact if exact else tables)(Ps, cs, lo, hi)
    got = query_tables(gm, gx, lo, hi, q_line, q_t)
    if z_m == 0:
        return dict(status=NOPATH)
    out = dict(zip(PER_LABEL, got))
    out.update(status=OK, z_m=z_m, z_x=z_x)
    return out


posterior, loglik_bits, same_bits = R.posterior, R.loglik_bits, R.same_bits
