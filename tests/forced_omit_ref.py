"""Forced alignment that may omit characters, the specification of record in plain Python /
numpy int64: what csrc/ta_forced_omit.hip must write, integer for integer.  q, the states and NEG are forced_ref's.

Inputs: P (T x no) float32, labels cs[0 .. L), omit (an int, 0 <= omit <= 2^26, in units of 2^-16 bit: the price of a
character of the text that the path does not enter).  1 <= L <= 1023, S = 2 L + 1 <= T <= 5000, 1 <= cs < no <= 128.

Start   v[s] = q(P[0, lab[s]]) - omit * (s // 2) for EVERY s: the characters in front of the start state are omitted.
Step    t >= 1; the candidates of s in tie order, the first one wins a tie:
          stay v[s];  advance v[s - 1];  skip v[s - 2] (odd s >= 3, lab[s] != lab[s - 2]);
          far: with i = s // 2 >= 1 every s' <= 2 i - 2 offers v[s'] - omit * (i - ceil(s' / 2)) -- the label states
          strictly between s' and s are paid for; among equal far candidates the LARGEST s' wins.
        v'[s] = best + q(P[t, lab[s]]).  A far move between two equal labels is allowed.
End     fin[s] = v[s] - omit * (L - ceil(s / 2)); the path ends at the s with the largest fin, the largest s on a tie; the
        score is that fin.
Frames  (L, 3) int32: t_first, t_last, t_peak as forced_ref.align's for a character the path spends a frame in,
        (-1, -1, -1) for one it never enters.

`align` is that text, candidate by candidate: O(T S^2).  `align_closed` is the form the kernel computes, O(T S): with
a[x] = v[x] + omit * ceil(x / 2) and Pm[x] = max(a[0 .. x]) the far candidate of blank 2 i and of label 2 i + 1 alike is
Pm[2 i - 2] - omit * i, and its s' is the first x at or below 2 i - 2 with a[x] >= Pm[x - 1].  tests/test_forced_omit.py
holds the two against each other and `align` against the enumeration of all paths; the case tables take `align` for the
lines it answers quickly and `align_closed` for the long ones (`answer`).
"""
import numpy as np

from forced_ref import NEG, q_of, states

OMIT_MAX = 1 << 26
OMITTED = -1
EXPLICIT_BUDGET = 1 << 21          # answer(): T * L * S at or below this goes through `align`


def _check(P, cs, omit):
    P = np.asarray(P, dtype=np.float32)
    cs = [int(c) for c in cs]
    T, no = P.shape
    L = len(cs)
    if L < 1 or 2 * L + 1 > T or any(c < 1 or c >= no for c in cs):
        raise ValueError("forced alignment needs 1 <= L, 2 L + 1 <= T and labels in 1 .. no - 1")
    if isinstance(omit, bool) or not isinstance(omit, (int, np.integer)) or not 0 <= omit <= OMIT_MAX:
        raise ValueError("omit is an integer in 0 .. 2^26")
    return P, cs, int(omit)


def _finish(Q, cs, v, src, omit):
    """the end rule, the walk back through the recorded predecessors and the frames"""
    T, L = len(Q), len(cs)
    S = 2 * L + 1
    up = (np.arange(S, dtype=np.int64) + 1) // 2
    fin = v - omit * (L - up)
    s = S - 1 - int(np.argmax(fin[::-1]))              # the largest s among the largest
    score = int(fin[s])
    path = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = s
        s = int(src[t, s])
    frames = np.full((L, 3), OMITTED, dtype=np.int32)
    for i in range(L):
        ts = np.nonzero(path == 2 * i + 1)[0]
        if len(ts):
            qi = Q[ts[0]:ts[-1] + 1, cs[i]]
            frames[i] = (ts[0], ts[-1], ts[0] + int(np.argmax(qi)))
    return score, frames, path


def align(P, cs, omit):
    """(score, frames (L, 3) int32, path (T,) the state of every timestep) of one line: the rule as it is written"""
    P, cs, omit = _check(P, cs, omit)
    T, L = len(P), len(cs)
    S = 2 * L + 1
    lab = states(cs)
    Q = q_of(P)
    E = Q[:, lab]
    idx = np.arange(S, dtype=np.int64)
    up = (idx + 1) // 2                                # ceil(s / 2)
    v = E[0] - omit * (idx // 2)
    src = np.zeros((T, S), dtype=np.int64)
    src[0] = idx
    for t in range(1, T):
        new = np.empty(S, dtype=np.int64)
        for s in range(S):
            best, frm = int(v[s]), s
            if s >= 1 and v[s - 1] > best:
                best, frm = int(v[s - 1]), s - 1
            if s % 2 == 1 and s >= 3 and lab[s] != lab[s - 2] and v[s - 2] > best:
                best, frm = int(v[s - 2]), s - 2
            i = s // 2
            if i >= 1:
                far = v[:2 * i - 1] - omit * (i - up[:2 * i - 1])
                sp = 2 * i - 2 - int(np.argmax(far[::-1]))         # the largest s' among the largest
                if far[sp] > best:
                    best, frm = int(far[sp]), sp
            new[s] = best + E[t, s]
            src[t, s] = frm
        v = new
    return _finish(Q, cs, v, src, omit)


def align_closed(P, cs, omit):
    """the same answer through one inclusive prefix maximum per timestep"""
    P, cs, omit = _check(P, cs, omit)
    T, L = len(P), len(cs)
    S = 2 * L + 1
    lab = states(cs)
    Q = q_of(P)
    E = Q[:, lab]
    idx = np.arange(S, dtype=np.int64)
    up = (idx + 1) // 2
    half = idx // 2
    may_skip = np.zeros(S, dtype=bool)
    may_skip[3::2] = lab[3::2] != lab[1:-2:2]
    has_far = half >= 1
    at = np.maximum(2 * half - 2, 0)                   # the state whose prefix maximum a far move reads
    v = E[0] - omit * half
    src = np.zeros((T, S), dtype=np.int64)
    src[0] = idx
    for t in range(1, T):
        a = v + omit * up
        Pm = np.maximum.accumulate(a)
        new_max = a >= np.concatenate(([NEG], Pm[:-1]))
        last_new = np.maximum.accumulate(np.where(new_max, idx, -1))
        adv = np.concatenate(([NEG], v[:-1]))
        skip = np.where(may_skip, np.concatenate(([NEG, NEG], v[:-2])), NEG)
        far = np.where(has_far, Pm[at] - omit * half, NEG)
        best, frm = v.copy(), idx.copy()
        for cand, where in ((adv, idx - 1), (skip, idx - 2), (far, last_new[at])):
            take = cand > best
            best = np.where(take, cand, best)
            frm = np.where(take, where, frm)
        v = best + E[t]
        src[t] = frm
    return _finish(Q, cs, v, src, omit)


def answer(P, cs, omit):
    """(score, frames) for the case tables: `align` where it is quick, `align_closed` (held equal to it by
    tests/test_forced_omit.py) for the long lines"""
    T, L = len(P), len(cs)
    f = align if T * L * (2 * L + 1) <= EXPLICIT_BUDGET else align_closed
    return f(P, cs, omit)[:2]


def align_batch(lines, omit):
    """[(P, cs)] -> frames (sum L, 3) int32, score (n,) int64"""
    out = [answer(P, cs, omit) for P, cs in lines]
    return (np.concatenate([f for _, f in out]) if out else np.zeros((0, 3), np.int32),
            np.asarray([s for s, _ in out], dtype=np.int64))


def path_score(P, cs, omit, path, Q=None):
    """the total of a path (a state per timestep) under the rule, or None if no move of the rule makes one of its steps
    (Q: q_of(P), for a caller that scores many paths)"""
    lab = states(cs)
    L = len(cs)
    Q = q_of(P) if Q is None else Q
    total = -omit * (int(path[0]) // 2) - omit * (L - (int(path[-1]) + 1) // 2)
    for a, b in zip(path[:-1], path[1:]):
        a, b = int(a), int(b)
        i = b // 2
        if b - a in (0, 1) or (b - a == 2 and b % 2 == 1 and lab[b] != lab[a]):
            pass
        elif i >= 1 and a <= 2 * i - 2:
            total -= omit * (i - (a + 1) // 2)
        else:
            return None
    return total + int(sum(int(Q[t, lab[s]]) for t, s in enumerate(path)))
