"""Per-character confidence on the lattice with omission, the specification of record in plain
Python / numpy int64: what csrc/ta_forced_omit_conf.hip must write, integer for integer.

q, lab, the states, the bounds and the moves are tests/forced_omit_ref.py's: 1 <= L <= 1023,
S = 2 L + 1 <= T <= 5000, omit in 0 .. 2^26; stay, advance, skip, and far at `omit` per label state jumped.  With
E[t][s] = q(P[t, lab[s]]), up[s] = ceil(s / 2) and half[s] = floor(s / 2):
    A[t][s]   forced_omit_ref's v after timestep t; A[0][s] = E[0][s] - omit * half[s].  Values only, no tie rule.
    B[T-1][s] -omit * (L - up[s]) for EVERY s: the end rule.
    B[t][s]   t < T - 1, with w[x] = B[t+1][x] + E[t+1][x], the maximum of w[s]; w[s+1] (s + 1 < S); w[s+2] (s odd,
              s + 2 < S, lab[s+2] != lab[s]); far: every x >= 2 up[s] + 2, x < S, offers w[x] - omit * (half[x] - up[s]).
    closed    c[x] = w[x] - omit * half[x], Sm[x] = max(c[x .. S-1]); far of s is Sm[2 up[s] + 2] + omit * up[s]: ONE
              inclusive suffix maximum of the row serves every state.
    G[t][s]   A[t][s] + B[t][s]: the total of the best path that spends frame t in state s.  Every state is reachable on
              this lattice: no REACH test, no NEG.  |G| < 1.5e11.
A query (i, t): own = G[t][2 i + 1], rival = the largest G[t][s] over s != 2 i + 1, rival_state the smallest such s,
confidence = own - rival.

The host's rule for the queries of a line, omit_queries(frames, T): a present character i asks (i, t_peak[i]); an
omitted one asks (i, t_land - 1) and (i, t_land), t_land the t_first of the next present character or T - 1 if none
follows, a frame below 0 dropped; all of a line's queries sorted by (frame, character).  A present character's value is
its one query's (own = score, confidence >= 0); an omitted character's is the largest confidence among its queries
(<= 0: the rival is the best path itself), with the rival state of the FIRST query that attains it.  -value is an UPPER
bound of exact_margin = score - max_t G[t][2 i + 1], what the best path loses if the character must appear at all.
"""
import numpy as np

import forced_omit_ref as R1
from forced_ref import q_of, states

QUERY = 4


def _setup(P, cs, omit):
    P, cs, omit = R1._check(P, cs, omit)
    lab = states(cs)
    E = q_of(P)[:, lab]
    S = len(lab)
    idx = np.arange(S, dtype=np.int64)
    return E, lab, len(cs), S, idx, (idx + 1) // 2, idx // 2, omit


def tables(P, cs, omit):
    """(A, B, G), each (T, S) int64, of one line: the rule edge by edge, O(T S^2)"""
    E, lab, L, S, idx, up, half, omit = _setup(P, cs, omit)
    T = len(E)
    A = np.zeros((T, S), dtype=np.int64)
    A[0] = E[0] - omit * half
    for t in range(1, T):
        v = A[t - 1]
        for s in range(S):
            cand = [int(v[s])]
            if s >= 1:
                cand.append(int(v[s - 1]))
            if s % 2 == 1 and s >= 3 and lab[s] != lab[s - 2]:
                cand.append(int(v[s - 2]))
            i = s // 2
            for sp in range(0, 2 * i - 1):                 # s' <= 2 i - 2
                cand.append(int(v[sp]) - omit * (i - int(up[sp])))
            A[t, s] = max(cand) + E[t, s]
    B = np.zeros((T, S), dtype=np.int64)
    B[T - 1] = -omit * (L - up)
    for t in range(T - 2, -1, -1):
        w = B[t + 1] + E[t + 1]
        for s in range(S):
            cand = [int(w[s])]
            if s + 1 < S:
                cand.append(int(w[s + 1]))
            if s % 2 == 1 and s + 2 < S and lab[s + 2] != lab[s]:
                cand.append(int(w[s + 2]))
            for x in range(2 * int(up[s]) + 2, S):
                cand.append(int(w[x]) - omit * (int(half[x]) - int(up[s])))
            B[t, s] = max(cand)
    return A, B, A + B


def tables_closed(P, cs, omit):
    """the same tables through one prefix maximum (forward) and one suffix maximum (backward) per timestep, O(T S)"""
    E, lab, L, S, idx, up, half, omit = _setup(P, cs, omit)
    T = len(E)
    none = np.iinfo(np.int64).min // 2                    # a candidate that does not exist
    may_skip = np.zeros(S, dtype=bool)                    # into s from s - 2
    may_skip[3::2] = lab[3::2] != lab[1:-2:2]
    skip_from = np.zeros(S, dtype=bool)                   # from s to s + 2: the same edges, named by their start
    skip_from[:-2] = may_skip[2:]
    A = np.zeros((T, S), dtype=np.int64)
    v = E[0] - omit * half
    A[0] = v
    at = np.maximum(2 * half - 2, 0)
    for t in range(1, T):
        Pm = np.maximum.accumulate(v + omit * up)
        adv = np.concatenate(([none], v[:-1]))
        skip = np.where(may_skip, np.concatenate(([none, none], v[:-2])), none)
        far = np.where(half >= 1, Pm[at] - omit * half, none)
        v = np.maximum(np.maximum(v, adv), np.maximum(skip, far)) + E[t]
        A[t] = v
    B = np.zeros((T, S), dtype=np.int64)
    b = -omit * (L - up)
    B[T - 1] = b
    src = 2 * up + 2                                      # the state whose suffix maximum a far move reads
    for t in range(T - 2, -1, -1):
        w = b + E[t + 1]
        Sm = np.maximum.accumulate((w - omit * half)[::-1])[::-1]
        adv = np.concatenate((w[1:], [none]))
        skip = np.where(skip_from, np.concatenate((w[2:], [none, none])), none)
        far = np.where(src < S, Sm[np.minimum(src, S - 1)] + omit * up, none)
        b = np.maximum(np.maximum(w, adv), np.maximum(skip, far))
        B[t] = b
    return A, B, A + B


def query(G, i, t):
    """(confidence, rival state, own) of the query (character i, frame t) on a line's G"""
    T, S = G.shape
    i, t = int(i), int(t)
    if not (0 <= i < (S - 1) // 2 and 0 <= t < T):
        raise ValueError("a query is a character of the text and a frame of the line")
    row = G[t].copy()
    own = int(row[2 * i + 1])
    row[2 * i + 1] = np.iinfo(np.int64).min               # the own state is no rival
    rival = int(row.argmax())                             # the first largest: the smallest state
    return own - int(row[rival]), rival, own


def query_list(G, q_char, q_frame):
    """(confidence (n,) int64, rival (n,) int32) of a list of queries on a line's G"""
    got = [query(G, i, t)[:2] for i, t in zip(q_char, q_frame)]
    return (np.asarray([c for c, _ in got], dtype=np.int64).reshape(-1),
            np.asarray([r for _, r in got], dtype=np.int32).reshape(-1))


def omit_queries(frames, T):
    """[(character, frame)] of one line from its frames (L, 3) as forced_omit_ref writes them, sorted by (frame, character)"""
    frames = np.asarray(frames)
    L = len(frames)
    out = []
    for i in range(L):
        if frames[i][0] >= 0:
            out.append((int(frames[i][2]), i))
            continue
        t_land = T - 1
        for j in range(i + 1, L):
            if frames[j][0] >= 0:
                t_land = int(frames[j][0])
                break
        out += [(t, i) for t in (t_land - 1, t_land) if t >= 0]
    return [(i, t) for t, i in sorted(out)]


def line_values(G, frames):
    """(value (L,) int64, rival state (L,) int32) per character of a line: a present character's one query, an omitted
    character's largest confidence among its queries and the rival state of the first that attains it"""
    frames = np.asarray(frames)
    L = len(frames)
    value, rival = [None] * L, [None] * L
    for i, t in omit_queries(frames, len(G)):
        c, r, _ = query(G, i, t)
        if value[i] is None or c > value[i]:
            value[i], rival[i] = c, r
    return np.asarray(value, dtype=np.int64), np.asarray(rival, dtype=np.int32)


def exact_margin(G, score, i):
    """what the best path loses if character i must appear at all: score - max over all frames of G[t][2 i + 1]"""
    return int(score) - int(G[:, 2 * int(i) + 1].max())
