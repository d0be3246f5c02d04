"""Page-scope forced alignment, the specification of record in plain Python / numpy int64: what
csrc/ta_forced_page.hip must write, integer for integer.

ONE best CTC path through the frames of all the lines of a page, one after the other.  The page's labels cs[0 .. n) give
the states s = 0 .. 2 n (lab[s] as forced_ref.states), the emission score is forced_ref.q_of, NEG = -2^50.  Line k has T_k
frames and a window of characters [lo_k, hi_k): during its frames only the states 2 lo_k .. 2 hi_k (blank to blank) are
live, every other state is NEG after each of them.  Windows: lo_0 = 0, hi_last = n, lo_k <= lo_{k+1} <= hi_k <= hi_{k+1},
0 <= hi_k - lo_k <= 1023 (an empty window is its one blank).
The page's first frame initialises the states 0 and 1 as forced_ref.align does.  Every later frame takes stay, adv, skip
(odd s >= 3, lab[s] != lab[s - 2]) in this order, ties to the earlier; a candidate whose source is not live in the
PREVIOUS frame's window is NEG, and on the first frame of a line k >= 1 a label state has no stay candidate: no character
spans a line break.  A state all of whose candidates are NEG (below -2^49: a value that started as NEG) stays NEG.
The path ends at the larger of 2 n and 2 n - 1, 2 n on a tie; below -2^49 the page has no path (NOPATH).
Per character: line, t_first, t_last, t_peak -- frame numbers local to that line, t_peak the first frame of the range with
the largest q of the character.
"""
import numpy as np

import forced_ref as R

NEG = R.NEG
DEAD = -(1 << 49)
OK, BOUNDS, LABEL, NOPATH = 0, 1, 2, 3
FIELDS = 4
MAX_TARGET = R.MAX_TARGET
H_EMPTY, H_PAGE = 1, 64              # harvest reason bits (harvest.EMPTY, harvest.PAGE)
# why a page was not refined at page scope (RefineResult.page_scope); 0 = refined
REFINED, NOT_PLAIN, HARVEST, CLASS0, NO_TEXT, WINDOWS, FRAMES, NO_PATH = range(8)


def windows_ok(lo, hi, n):
    lo, hi = [int(v) for v in lo], [int(v) for v in hi]
    if not lo or len(lo) != len(hi) or lo[0] != 0 or hi[-1] != n:
        return False
    for k in range(len(lo)):
        if not 0 <= hi[k] - lo[k] <= MAX_TARGET or lo[k] < 0:
            return False
        if k + 1 < len(lo) and not lo[k] <= lo[k + 1] <= hi[k] <= hi[k + 1]:
            return False
    return True


def align_page(Ps, cs, lo, hi, line_stay=False):
    """(status, score, frames (n, 4) int32 = line, t_first, t_last, t_peak, path [(line, t, state)]) of one page.
    Ps: the lines' probability rows.  ValueError for what the kernel refuses (windows, labels).  line_stay=True drops
    the rule of the line break (a label state may stay into a new line): the unconstrained lattice, for comparison."""
    cs = [int(c) for c in cs]
    n, nl = len(cs), len(Ps)
    Ps = [np.asarray(P, dtype=np.float32) for P in Ps]
    no = Ps[0].shape[1]
    if n < 1 or len(lo) != nl or len(hi) != nl or not windows_ok(lo, hi, n) or any(len(P) < 1 for P in Ps):
        raise ValueError("windows")
    if any(c < 1 or c >= no for c in cs):
        raise ValueError("labels")
    lab = R.states(cs)
    S = 2 * n + 1
    may_skip = np.zeros(S, dtype=bool)
    may_skip[3::2] = lab[3::2] != lab[1:-2:2]
    odd = np.arange(S) % 2 == 1
    v = np.full(S, NEG, dtype=np.int64)
    moves, Qs = [], []
    for k, P in enumerate(Ps):
        Q = R.q_of(P)
        Qs.append(Q)
        E = Q[:, lab]
        live = np.zeros(S, dtype=bool)
        live[2 * int(lo[k]):2 * int(hi[k]) + 1] = True
        mv = np.zeros((len(P), S), dtype=np.int8)
        for t in range(len(P)):
            if k == 0 and t == 0:
                v[:2] = E[0, :2]
            else:
                stay = v.copy()
                if t == 0 and not line_stay:
                    stay[odd] = NEG
                adv = np.concatenate(([NEG], v[:-1]))
                skip = np.where(may_skip, np.concatenate(([NEG, NEG], v[:-2])), NEG)
                m = np.where(adv > stay, 1, 0)
                best = np.maximum(stay, adv)
                m = np.where(skip > best, 2, m)
                best = np.maximum(best, skip)
                v = np.where(best < DEAD, NEG, best + E[t])
                mv[t] = m
            v[~live] = NEG
        moves.append(mv)
    s = S - 2 if v[S - 2] > v[S - 1] else S - 1
    score = int(v[s])
    if score < DEAD:
        return NOPATH, score, None, None
    path = []
    for k in range(nl - 1, -1, -1):
        for t in range(len(Ps[k]) - 1, -1, -1):
            path.append((k, t, s))
            s -= 1 if (k == 0 and t == 0) else int(moves[k][t, s])
    path.reverse()
    frames = np.zeros((n, FIELDS), dtype=np.int32)
    for i in range(n):
        at = [(k, t) for k, t, st in path if st == 2 * i + 1]
        k, t0, t1 = at[0][0], at[0][1], at[-1][1]
        assert all(a[0] == k for a in at) or line_stay
        qi = Qs[k][t0:t1 + 1, cs[i]]
        frames[i] = (k, t0, t1, t0 + int(np.argmax(qi))) if all(a[0] == k for a in at) else (k, t0, t1, t0)
    return OK, score, frames, path


def path_score(Ps, cs, lo, hi, path):
    """the total of a path [(line, t, state)] over every frame of the page, or None if the rule does not allow it"""
    lab = R.states(cs)
    S = len(lab)
    want = [(k, t) for k, P in enumerate(Ps) for t in range(len(P))]
    if [(k, t) for k, t, _ in path] != want or path[0][2] not in (0, 1) or path[-1][2] not in (S - 1, S - 2):
        return None
    total = 0
    for i, (k, t, s) in enumerate(path):
        if not 2 * lo[k] <= s <= 2 * hi[k]:
            return None
        if i:
            d = s - path[i - 1][2]
            if d not in (0, 1, 2) or (d == 2 and not (s % 2 == 1 and s >= 3 and lab[s] != lab[s - 2])):
                return None
            if d == 0 and s % 2 == 1 and t == 0:
                return None
        total += int(R.q_of(Ps[k][t, lab[s]]))
    return total


def page_windows(table_rows, n, margin=16):
    """(lo, hi) int64 per line from the harvest rows of a page's lines (fields 0 - 2: reason, t_first, L), or None if
    a window is wider than MAX_TARGET.  A line without EMPTY / PAGE has the core [t_first, t_first + L), any other the
    empty range at the previous core's end (0 in front); lo = max(0, core_lo - margin), hi = min(n, core_hi + margin);
    lo_0 = 0, hi_last = n; then forwards lo_k = max(lo_k, lo_{k-1}), hi_k = max(hi_k, hi_{k-1}), lo_k = min(lo_k, hi_{k-1})."""
    rows = np.asarray(table_rows, dtype=np.int64).reshape(len(table_rows), -1)
    nl = len(rows)
    if margin < 0 or nl < 1:
        raise ValueError("margin >= 0 and at least one line")
    lo, hi = np.zeros(nl, np.int64), np.zeros(nl, np.int64)
    end = 0
    for k in range(nl):
        if int(rows[k, 0]) & (H_EMPTY | H_PAGE):
            a = b = end
        else:
            a, b = int(rows[k, 1]), int(rows[k, 1]) + int(rows[k, 2])
        end = b
        lo[k], hi[k] = max(0, a - margin), min(n, b + margin)
    lo[0], hi[-1] = 0, n
    for k in range(1, nl):
        lo[k] = max(lo[k], lo[k - 1])
        hi[k] = max(hi[k], hi[k - 1])
        lo[k] = min(lo[k], hi[k - 1])
    if (hi - lo > MAX_TARGET).any():
        return None
    return lo, hi
