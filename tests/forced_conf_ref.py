"""Per-character confidence of a forced alignment from max-marginals, the specification of record (DESIGN.md section
14.10) in plain Python / numpy int64: what csrc/ta_forced_conf.hip must write, integer for integer.

The lattice, the emission score q, lab, NEG and the skip rule are tests/forced_ref.py's.  For a line with probabilities P
(T x no) and labels cs[0 .. L), S = 2 L + 1 <= T:
    A[t][s]   forced_ref's v after timestep t: the best total of frames 0 .. t of a path that is in state s at t, the
              emission at t included; not clamped, unreachable states carry NEG plus emissions.
    B[T-1][s] 0 for s in {S - 1, S - 2}, NEG elsewhere.  For t < T - 1, with w[s] = B[t+1][s] + q(P[t+1, lab[s]]):
              B[t][s] = max(w[s], w[s+1] if s + 1 < S, w[s+2] if s + 2 < S, s + 2 odd and lab[s+2] != lab[s]).  A pure max.
    G[t][s]   A[t][s] + B[t][s] if both are above REACH = -2^49, else exactly NEG: the total of the best path that spends
              frame t in state s.  (Emission sums stay below 6e9 in magnitude within T <= 5000, so the test is exact.)
A query (character i, frame t): own = G[t][2 i + 1], rival = the largest G[t][s] over s != 2 i + 1, rival_state the
smallest such s that attains it, confidence = own - rival in units of 2^-16 bit -- no special cases.  At the aligner's own
t_peak[i], own is the line's score and confidence >= 0 (0: a tie).
"""
import numpy as np

import forced_ref as R

NEG = R.NEG
REACH = -(1 << 49)
QUERY = 4


def tables(P, cs):
    """(A, B, G), each (T, S) int64, of one line"""
    P = np.asarray(P, dtype=np.float32)
    cs = [int(c) for c in cs]
    T, no = P.shape
    L = len(cs)
    S = 2 * L + 1
    if L < 1 or S > T or any(c < 1 or c >= no for c in cs):
        raise ValueError("forced alignment needs 1 <= L, 2 L + 1 <= T and labels in 1 .. no - 1")
    lab = R.states(cs)
    E = R.q_of(P)[:, lab]                             # (T, S)
    none = np.iinfo(np.int64).min                     # a candidate that does not exist
    may_skip = np.zeros(S, dtype=bool)                # into s from s - 2
    may_skip[3::2] = lab[3::2] != lab[1:-2:2]
    skip_from = np.zeros(S, dtype=bool)               # from s to s + 2: the same edges, named by their start
    skip_from[:-2] = may_skip[2:]
    A = np.zeros((T, S), dtype=np.int64)
    v = np.full(S, NEG, dtype=np.int64)
    v[:2] = E[0, :2]
    A[0] = v
    for t in range(1, T):
        adv = np.concatenate(([none], v[:-1]))
        skip = np.where(may_skip, np.concatenate(([none, none], v[:-2])), none)
        v = np.maximum(np.maximum(v, adv), skip) + E[t]
        A[t] = v
    B = np.zeros((T, S), dtype=np.int64)
    b = np.full(S, NEG, dtype=np.int64)
    b[S - 2:] = 0
    B[T - 1] = b
    for t in range(T - 2, -1, -1):
        w = b + E[t + 1]
        adv = np.concatenate((w[1:], [none]))
        skip = np.where(skip_from, np.concatenate((w[2:], [none, none])), none)
        b = np.maximum(np.maximum(w, adv), skip)
        B[t] = b
    G = np.where((A > REACH) & (B > REACH), A + B, NEG)
    return A, B, G


def query_tables(G, tq):
    """(confidence (L,) int64, rival state (L,) int32, own (L,) int64) of the queries tq[i] for character i on a line's G"""
    S = G.shape[1]
    L = (S - 1) // 2
    tq = [int(t) for t in tq]
    if len(tq) != L or any(t < 0 or t >= len(G) for t in tq):
        raise ValueError("a query frame per character, inside 0 .. T - 1")
    rows = G[np.asarray(tq, dtype=np.int64)]          # (L, S): row i is G at character i's query frame
    at = np.arange(L)
    own = rows[at, 2 * at + 1].copy()
    rows[at, 2 * at + 1] = np.iinfo(np.int64).min     # below NEG: the own state is no rival
    rival = rows.argmax(axis=1).astype(np.int32)      # the first largest: the smallest state
    conf = own - rows[at, rival]
    return conf, rival, own


def query(P, cs, tq):
    """(confidence (L,) int64, rival state (L,) int32) of one line for the query frames tq"""
    conf, rival, _ = query_tables(tables(P, cs)[2], tq)
    return conf, rival


def query_batch(lines, queries):
    """[(P, cs)], [tq] -> confidence (sum L,) int64, rival (sum L,) int32"""
    out = [query(P, cs, tq) for (P, cs), tq in zip(lines, queries)]
    if not out:
        return np.zeros(0, np.int64), np.zeros(0, np.int32)
    return np.concatenate([c for c, _ in out]), np.concatenate([r for _, r in out])
