"""Per-character confidence at page scope from max-marginals, the specification of record in
plain Python / numpy int64: what csrc/ta_forced_page_conf.hip must write, integer for integer.

The lattice is tests/forced_page_ref.py's, unchanged: the emission score q, lab, NEG = -2^50, the skip rule, the windows
[lo_k, hi_k) and the live states 2 lo_k .. 2 hi_k during the frames of line k.  The frames of a page are ordered (k, t),
line after line.
    A[k][t][s]  align_page's v after frame (k, t), with both of its clamps: a state whose best candidate lies below
                -2^49 is NEG, and a state that is not live is NEG.
    B           at the page's last frame 0 for s in {2 n, 2 n - 1}, NEG elsewhere, masked to the last window's live states.
                For a frame f with the successor f' = (k', t'): w[s'] = B[f'][s'] + q(P_k'[t', lab[s']]), NEG where B[f'][s']
                lies below -2^49; B[f][s] = max(w[s] -- but not for odd s when t' = 0: a character never stays across a
                line break --, w[s + 1], w[s + 2] if s + 2 is odd and lab[s + 2] != lab[s]); below -2^49 it is NEG; then it
                is masked to the live states of f's own line.  A pure max, no tie rule.
    G           A + B where both are above REACH = -2^49, else exactly NEG: the total of the best legal path of the page
                that spends frame (k, t) in state s.
A query is a character i at a frame (k, t) with lo_k <= i < hi_k: own = G[k][t][2 i + 1], rival = the largest G[k][t][s] over
the live states s != 2 i + 1 of line k's window, rival_state the smallest such PAGE state that attains it, confidence =
own - rival in units of 2^-16 bit.  Where no rival is reachable rival = NEG and rival_state = 2 lo_k: that falls out of
the arithmetic.  The queries must not decrease in (k, t) order as i grows; equal neighbours are allowed, and align_page's
own (line, t_peak) always qualify: there own is the page's score and confidence >= 0.
"""
import numpy as np

import forced_page_ref as P
import forced_ref as R

NEG = R.NEG
REACH = -(1 << 49)
QUERY = 4
MAX_FRAMES = 1 << 25


def tables(Ps, cs, lo, hi):
    """(A, B, G), each a list per line of (T_k, 2 n + 1) int64 arrays.  ValueError as forced_page_ref.align_page."""
    cs = [int(c) for c in cs]
    n, nl = len(cs), len(Ps)
    Ps = [np.asarray(p, dtype=np.float32) for p in Ps]
    if n < 1 or nl < 1 or len(lo) != nl or len(hi) != nl or not P.windows_ok(lo, hi, n) or any(len(p) < 1 for p in Ps):
        raise ValueError("windows")
    no = Ps[0].shape[1]
    if any(c < 1 or c >= no for c in cs):
        raise ValueError("labels")
    lab = R.states(cs)
    S = 2 * n + 1
    may_skip = np.zeros(S, dtype=bool)                # into s from s - 2
    may_skip[3::2] = lab[3::2] != lab[1:-2:2]
    skip_from = np.zeros(S, dtype=bool)               # from s to s + 2: the same edges, named by their start
    skip_from[:-2] = may_skip[2:]
    odd = np.arange(S) % 2 == 1
    E = [R.q_of(p)[:, lab] for p in Ps]
    live = np.zeros((nl, S), dtype=bool)
    for k in range(nl):
        live[k, 2 * int(lo[k]):2 * int(hi[k]) + 1] = True
    A = [np.zeros((len(p), S), dtype=np.int64) for p in Ps]
    v = np.full(S, NEG, dtype=np.int64)
    for k in range(nl):
        for t in range(len(Ps[k])):
            if k == 0 and t == 0:
                v[:2] = E[0][0, :2]
            else:
                stay = v.copy()
                if t == 0:
                    stay[odd] = NEG
                adv = np.concatenate(([NEG], v[:-1]))
                skip = np.where(may_skip, np.concatenate(([NEG, NEG], v[:-2])), NEG)
                best = np.maximum(np.maximum(stay, adv), skip)
                v = np.where(best < REACH, NEG, best + E[k][t])
            v[~live[k]] = NEG
            A[k][t] = v
    B = [np.zeros((len(p), S), dtype=np.int64) for p in Ps]
    b = np.full(S, NEG, dtype=np.int64)
    b[S - 2:] = 0
    b[~live[nl - 1]] = NEG
    B[nl - 1][-1] = b
    order = [(k, t) for k in range(nl) for t in range(len(Ps[k]))]
    for f in range(len(order) - 2, -1, -1):
        (k, t), (k2, t2) = order[f], order[f + 1]
        w = np.where(b < REACH, NEG, b + E[k2][t2])
        stay = w.copy()
        if t2 == 0:
            stay[odd] = NEG
        adv = np.concatenate((w[1:], [NEG]))
        skip = np.where(skip_from, np.concatenate((w[2:], [NEG, NEG])), NEG)
        b = np.maximum(np.maximum(stay, adv), skip)
        b = np.where(b < REACH, NEG, b)
        b[~live[k]] = NEG
        B[k][t] = b
    G = [np.where((a > REACH) & (bb > REACH), a + bb, NEG) for a, bb in zip(A, B)]
    return A, B, G


def queries_ok(q_line, q_t, Ts, lo, hi):
    """a query per character: a line of the page, a frame of that line, the character inside the line's window, and
    (line, frame) never decreasing from one character to the next"""
    last = (0, 0)
    for i, (k, t) in enumerate(zip(q_line, q_t)):
        k, t = int(k), int(t)
        if not 0 <= k < len(Ts) or not 0 <= t < Ts[k] or not int(lo[k]) <= i < int(hi[k]) or (k, t) < last:
            return False
        last = (k, t)
    return True


def query_tables(G, lo, hi, q_line, q_t):
    """(confidence (n,) int64, rival page state (n,) int32, own (n,) int64) of the queries (q_line[i], q_t[i]) for
    character i on a page's G.  ValueError for queries the kernel refuses (TA_FORCED_QUERY)."""
    n = (G[0].shape[1] - 1) // 2
    if len(q_line) != n or len(q_t) != n or not queries_ok(q_line, q_t, [len(g) for g in G], lo, hi):
        raise ValueError("queries")
    conf, rival, own = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int64)
    for i in range(n):
        k, t = int(q_line[i]), int(q_t[i])
        a, b = 2 * int(lo[k]), 2 * int(hi[k]) + 1
        row = G[k][t, a:b].copy()
        own[i] = row[2 * i + 1 - a]
        row[2 * i + 1 - a] = np.iinfo(np.int64).min    # below NEG: the own state is no rival
        r = int(row.argmax())                         # the first largest: the smallest state
        conf[i], rival[i] = own[i] - row[r], a + r
    return conf, rival, own


def query(Ps, cs, lo, hi, q_line, q_t):
    """(confidence (n,) int64, rival page state (n,) int32) of one page"""
    conf, rival, _ = query_tables(tables(Ps, cs, lo, hi)[2], lo, hi, q_line, q_t)
    return conf, rival
