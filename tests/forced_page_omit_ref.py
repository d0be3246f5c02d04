"""Page-scope forced alignment that may omit characters, the specification of record in plain
Python / numpy int64: what csrc/ta_forced_page_omit.hip must write, integer for integer.

The emission score q, the states s = 0 .. 2 n of the page's labels cs[0 .. n), NEG = -2^50 and DEAD = -2^49 are
forced_ref's and forced_page_ref's; pages, lines and the windows [lo_k, hi_k) with their conditions are
forced_page_ref's (section 14.8); omit is forced_omit_ref's integer price, 0 .. 2^26 (section 14.9).

Live    during line k the states 2 lo_k .. 2 hi_k are live; every other state is NEG after each frame.
Start   first frame of the page: v[s] = q(P[0, lab[s]]) - omit * (s // 2) for EVERY s live in window 0.
Step    the candidates of s in tie order, the first one wins a tie:
          stay v[s] -- on the first frame of a line k >= 1 a label state has none: no character spans a line break;
          advance v[s - 1];  skip v[s - 2] (odd s >= 3, lab[s] != lab[s - 2]);
          far: with i = s // 2 >= 1 every s' <= 2 i - 2 offers v[s'] - omit * (i - ceil(s' / 2)); among equal far
          candidates the LARGEST s' wins.  A far move between equal labels is allowed.
        The sources are the PREVIOUS frame's row: on a line's first frame that is the previous line's window, states
        below the new window's first included -- a far move may jump the characters between two windows' cores.
        v'[s] = best + q(P[t, lab[s]]); a state whose best is below DEAD stays NEG; then the states that are not live
        become NEG.
End     fin[s] = v[s] - omit * (n - ceil(s / 2)) over the states live in the last window; the largest, the largest s on a
        tie; the score is that fin.  Below DEAD the page has no path (NOPATH) -- which cannot happen: state 2 lo_{k+1} is
        live in window k, and from any finite state of the old window a stay, advance or far move leads into the new one.
Frames  (n, 4) int32: line, t_first, t_last, t_peak as forced_page_ref's for a character the path spends a frame in,
        (-1, -1, -1, -1) for one it never enters.
Limits  n <= 2^20 characters and at most 2^25 frames per page: omit * n + 2^21 * frames < 2^48, nothing approaches DEAD.

`align_page_omit` is that text, candidate by candidate: O(frames S^2).  `align_page_omit_closed` is the form the kernel
computes: with a[x] = v[x] + omit * ceil(x / 2) and Pm[x] = max(a[0 .. x]) the far candidate of blank 2 i and label
2 i + 1 alike is Pm[2 i - 2] - omit * i, and its s' is the first x at or below 2 i - 2 with a[x] >= Pm[x - 1].  a may be
formed in WINDOW coordinates (x minus 2 lo_k): a window starts at an even page state, so moving to the next window's
coordinates, d = lo_{k+1} - lo_k characters on, adds omit * d to both sides of every comparison and to the candidate's
two terms alike.  The kernel relies on this; window_coordinates=True computes it that way.
"""
import numpy as np

import forced_page_ref as PR
from forced_ref import NEG, q_of, states

DEAD = PR.DEAD
OK, BOUNDS, LABEL, NOPATH = PR.OK, PR.BOUNDS, PR.LABEL, PR.NOPATH
FIELDS = PR.FIELDS
OMIT_MAX = 1 << 26
OMITTED = -1
MAX_CHARS, MAX_FRAMES = 1 << 20, 1 << 25
EXPLICIT_BUDGET = 1 << 21          # answer(): frames * n * S at or below this goes through the written form
# RefineResult.page_scope with page_omit: forced_page_ref's codes, and two more
TOO_LONG, ALL_OMITTED = 8, 9


def _check(Ps, cs, lo, hi, omit):
    cs = [int(c) for c in cs]
    n, nl = len(cs), len(Ps)
    Ps = [np.asarray(P, dtype=np.float32) for P in Ps]
    if n < 1 or nl < 1 or len(lo) != nl or len(hi) != nl or not PR.windows_ok(lo, hi, n) or any(len(P) < 1 for P in Ps):
        raise ValueError("windows")
    if n > MAX_CHARS or sum(len(P) for P in Ps) > MAX_FRAMES:
        raise ValueError("limits")
    no = Ps[0].shape[1]
    if any(c < 1 or c >= no for c in cs):
        raise ValueError("labels")
    if isinstance(omit, bool) or not isinstance(omit, (int, np.integer)) or not 0 <= omit <= OMIT_MAX:
        raise ValueError("omit is an integer in 0 .. 2^26")
    return Ps, cs, [int(v) for v in lo], [int(v) for v in hi], int(omit)


def _finish(Ps, Qs, cs, lo, hi, v, srcs, omit):
    """the end rule, the walk back through the recorded predecessors and the frames"""
    n, nl = len(cs), len(Ps)
    S = 2 * n + 1
    up = (np.arange(S, dtype=np.int64) + 1) // 2
    fin = np.where(np.arange(S) >= 2 * lo[-1], v - omit * (n - up), 2 * NEG)       # hi_last = n: live up to 2 n
    s = S - 1 - int(np.argmax(fin[::-1]))
    score = int(fin[s])
    if score < DEAD:
        return NOPATH, score, None, None
    path = []
    for k in range(nl - 1, -1, -1):
        for t in range(len(Ps[k]) - 1, -1, -1):
            path.append((k, t, s))
            s = int(srcs[k][t, s])
    path.reverse()
    frames = np.full((n, FIELDS), OMITTED, dtype=np.int32)
    for i in range(n):
        at = [(k, t) for k, t, st in path if st == 2 * i + 1]
        if at:
            k, t0, t1 = at[0][0], at[0][1], at[-1][1]
            assert all(a[0] == k for a in at)
            frames[i] = (k, t0, t1, t0 + int(np.argmax(Qs[k][t0:t1 + 1, cs[i]])))
    return OK, score, frames, path


def align_page_omit(Ps, cs, lo, hi, omit):
    """(status, score, frames (n, 4) int32, path [(line, t, state)]) of one page: the rule as it is written"""
    Ps, cs, lo, hi, omit = _check(Ps, cs, lo, hi, omit)
    n = len(cs)
    S = 2 * n + 1
    lab = states(cs)
    idx = np.arange(S, dtype=np.int64)
    up = (idx + 1) // 2
    v = np.full(S, NEG, dtype=np.int64)
    srcs, Qs = [], []
    for k, P in enumerate(Ps):
        Q = q_of(P)
        Qs.append(Q)
        E = Q[:, lab]
        a0, a1 = 2 * lo[k], 2 * hi[k]
        src = np.zeros((len(P), S), dtype=np.int64)
        for t in range(len(P)):
            new = np.full(S, NEG, dtype=np.int64)
            if k == 0 and t == 0:
                new[a0:a1 + 1] = E[0, a0:a1 + 1] - omit * (idx[a0:a1 + 1] // 2)
                src[0] = idx
            else:
                for s in range(a0, a1 + 1):
                    best, frm = int(v[s]), s
                    if t == 0 and s % 2 == 1:
                        best = int(NEG)
                    if s >= 1 and v[s - 1] > best:
                        best, frm = int(v[s - 1]), s - 1
                    if s % 2 == 1 and s >= 3 and lab[s] != lab[s - 2] and v[s - 2] > best:
                        best, frm = int(v[s - 2]), s - 2
                    i = s // 2
                    if i >= 1:
                        far = v[:2 * i - 1] - omit * (i - up[:2 * i - 1])
                        sp = 2 * i - 2 - int(np.argmax(far[::-1]))     # the largest s' among the largest
                        if far[sp] > best:
                            best, frm = int(far[sp]), sp
                    if best >= DEAD:
                        new[s] = best + E[t, s]
                    src[t, s] = frm
            v = new
        srcs.append(src)
    return _finish(Ps, Qs, cs, lo, hi, v, srcs, omit)


def align_page_omit_closed(Ps, cs, lo, hi, omit, window_coordinates=False):
    """the same answer through one inclusive prefix maximum per frame; window_coordinates: a[] formed with the
    characters counted from the old window's first, as the kernel forms it"""
    Ps, cs, lo, hi, omit = _check(Ps, cs, lo, hi, omit)
    n = len(cs)
    S = 2 * n + 1
    lab = states(cs)
    idx = np.arange(S, dtype=np.int64)
    up, half = (idx + 1) // 2, idx // 2
    odd = idx % 2 == 1
    may_skip = np.zeros(S, dtype=bool)
    may_skip[3::2] = lab[3::2] != lab[1:-2:2]
    has_far = half >= 1
    at = np.maximum(2 * half - 2, 0)
    v = np.full(S, NEG, dtype=np.int64)
    srcs, Qs = [], []
    for k, P in enumerate(Ps):
        Q = q_of(P)
        Qs.append(Q)
        E = Q[:, lab]
        live = (idx >= 2 * lo[k]) & (idx <= 2 * hi[k])
        src = np.zeros((len(P), S), dtype=np.int64)
        for t in range(len(P)):
            if k == 0 and t == 0:
                v = np.where(live, E[0] - omit * half, NEG)
                src[0] = idx
                continue
            base = (lo[k - 1] if t == 0 else lo[k]) if window_coordinates else 0   # the window the SOURCES lie in
            a = v + omit * (up - base)
            Pm = np.maximum.accumulate(a)
            new_max = a >= np.concatenate(([2 * NEG], Pm[:-1]))
            last_new = np.maximum.accumulate(np.where(new_max, idx, -1))
            adv = np.concatenate(([NEG], v[:-1]))
            skip = np.where(may_skip, np.concatenate(([NEG, NEG], v[:-2])), NEG)
            far = np.where(has_far, Pm[at] - omit * (half - base), NEG)
            best, frm = v.copy(), idx.copy()
            if t == 0:
                best[odd] = NEG
            for cand, where in ((adv, idx - 1), (skip, idx - 2), (far, last_new[at])):
                take = cand > best
                best = np.where(take, cand, best)
                frm = np.where(take, where, frm)
            v = np.where(live & (best >= DEAD), best + E[t], NEG)
            src[t] = frm
        srcs.append(src)
    return _finish(Ps, Qs, cs, lo, hi, v, srcs, omit)


def answer(Ps, cs, lo, hi, omit):
    """(status, score, frames) for the case tables: the written form where it is quick, the closed form (held equal to it
    by tests/test_forced_page_omit.py) for the long pages"""
    frames, n = sum(len(P) for P in Ps), len(cs)
    f = align_page_omit if frames * n * (2 * n + 1) <= EXPLICIT_BUDGET else align_page_omit_closed
    return f(Ps, cs, lo, hi, omit)[:3]


def path_score(Ps, cs, lo, hi, omit, path):
    """the total of a path [(line, t, state)] over every frame of the page under the rule, or None if the rule does not
    allow it"""
    lab = states(cs)
    n = len(cs)
    want = [(k, t) for k, P in enumerate(Ps) for t in range(len(P))]
    if [(k, t) for k, t, _ in path] != want:
        return None
    total = -omit * (path[0][2] // 2) - omit * (n - (path[-1][2] + 1) // 2)
    for j, (k, t, s) in enumerate(path):
        if not 2 * lo[k] <= s <= 2 * hi[k]:
            return None
        if j:
            a = path[j - 1][2]
            i = s // 2
            if s == a:
                if t == 0 and s % 2 == 1:
                    return None
            elif s - a == 1 or (s - a == 2 and s % 2 == 1 and lab[s] != lab[a]):
                pass
            elif i >= 1 and a <= 2 * i - 2:
                total -= omit * (i - (a + 1) // 2)
            else:
                return None
        total += int(q_of(Ps[k][t, lab[s]]))
    return total
