"""Forced alignment, the specification of record in plain Python / numpy int64: what
csrc/ta_forced.hip must write, integer for integer.

Emission score q(p) of a float32 probability, in units of 2^-16 bit, q <= 0:
    p' = p > 2^-17 ? p : 2^-17          (NaN, 0 and negatives go to the floor: the comparison form matters)
    p' = p' < 1 ? p' : 1
    u = bit pattern of p';  e = (u >> 23) - 127  (-17 .. 0);  g = (u & 0x7FFFFF) >> 7  (0 .. 65535)
    q = e * 65536 + g + ((((g * (65536 - g)) >> 16) * 22713) >> 16)
g + corr approximates 65536 log2(1 + g / 65536) to within 0.008 bit; no transcendental function anywhere.

Lattice of a line with probabilities P (T x no) and labels cs[0 .. L), 1 <= cs < no, L >= 1, S = 2 L + 1 <= T:
lab[s] = 0 for even s, cs[(s - 1) / 2] for odd s.  v[s] = q(P[0, lab[s]]) for s in {0, 1}, NEG = -2^50 elsewhere; for
t >= 1 the candidates of s are stay = v[s], adv = v[s - 1] (s >= 1), skip = v[s - 2] (odd s >= 3, lab[s] != lab[s - 2]);
the largest wins, on ties stay beats adv beats skip; v'[s] = best + q(P[t, lab[s]]).  The path ends at S - 1 or S - 2,
whichever is larger, S - 1 on a tie, and the recorded moves are walked back from t = T - 1.
Per character i: t_first / t_last = the first / last timestep the path spends in state 2 i + 1, t_peak = the first t of
that range with the largest q(P[t, cs[i]]).
"""
import numpy as np

NEG = -(1 << 50)
FLOOR = np.float32(2.0 ** -17)
OK, BOUNDS, LABEL = 0, 1, 2
MAX_TARGET, MAX_T, MAX_CLASSES, WALK_BLOCK = 1023, 5000, 128, 32


def q_of(p):
    """the emission scores (int64, same shape) of float32 probabilities"""
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        a = np.where(p > FLOOR, p, FLOOR).astype(np.float32)
        a = np.where(a < np.float32(1), a, np.float32(1)).astype(np.float32)
    u = a.view(np.uint32).astype(np.int64)
    e = (u >> 23) - 127
    g = (u & 0x7FFFFF) >> 7
    return e * 65536 + g + ((((g * (65536 - g)) >> 16) * 22713) >> 16)


def states(cs):
    lab = np.zeros(2 * len(cs) + 1, dtype=np.int64)
    lab[1::2] = cs
    return lab


def align(P, cs):
    """(score, frames (L, 3) int32, path (T,) the state of every timestep) of one line"""
    P = np.asarray(P, dtype=np.float32)
    cs = [int(c) for c in cs]
    T, no = P.shape
    L = len(cs)
    S = 2 * L + 1
    if L < 1 or S > T or any(c < 1 or c >= no for c in cs):
        raise ValueError("forced alignment needs 1 <= L, 2 L + 1 <= T and labels in 1 .. no - 1")
    lab = states(cs)
    Q = q_of(P)                                       # (T, no)
    E = Q[:, lab]                                     # (T, S)
    none = np.iinfo(np.int64).min                     # a candidate that does not exist
    may_skip = np.zeros(S, dtype=bool)
    may_skip[3::2] = lab[3::2] != lab[1:-2:2]
    v = np.full(S, NEG, dtype=np.int64)
    v[:2] = E[0, :2]
    moves = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):                             # all states of a timestep at once; the rule is per state
        adv = np.concatenate(([none], v[:-1]))
        skip = np.where(may_skip, np.concatenate(([none, none], v[:-2])), none)
        m = np.where(adv > v, 1, 0)
        best = np.maximum(v, adv)
        m = np.where(skip > best, 2, m)
        best = np.maximum(best, skip)
        v = best + E[t]
        moves[t] = m
    s = S - 2 if v[S - 2] > v[S - 1] else S - 1
    score = int(v[s])
    path = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = s
        s -= int(moves[t, s])
    frames = np.zeros((L, 3), dtype=np.int32)
    for i in range(L):
        ts = np.nonzero(path == 2 * i + 1)[0]
        qi = Q[ts[0]:ts[-1] + 1, cs[i]]
        frames[i] = (ts[0], ts[-1], ts[0] + int(np.argmax(qi)))
    return score, frames, path


def path_score(P, cs, path):
    """the total of a path (a state per timestep), or None if the topology does not allow it"""
    lab = states(cs)
    S = len(lab)
    if path[0] not in (0, 1) or path[-1] not in (S - 1, S - 2):
        return None
    for a, b in zip(path[:-1], path[1:]):
        d = b - a
        if d not in (0, 1, 2) or (d == 2 and not (b % 2 == 1 and b >= 3 and lab[b] != lab[b - 2])):
            return None
    Q = q_of(P)
    return int(sum(int(Q[t, lab[s]]) for t, s in enumerate(path)))


def align_batch(lines):
    """[(P, cs)] -> frames (sum L, 3) int32, score (n,) int64"""
    out = [align(P, cs) for P, cs in lines]
    return (np.concatenate([f for _, f, _ in out]) if out else np.zeros((0, 3), np.int32),
            np.asarray([s for s, _, _ in out], dtype=np.int64))


def peak_x(t_peak, T, raw_w, pad):
    """the .llocs position of a timestep: x = (t - pad) raw_w / (T - 2 pad), in raw strip pixels"""
    return (np.asarray(t_peak, dtype=np.float64) - pad) * (float(raw_w) / (T - 2 * pad))


# ---- boxes under refinement: the per-character rule ----------------------------------------------------------------------

def char_boxes(tra, ocr, o_line, ocr_boxes, refined):
    """per transcript character its box (a 4-tuple ulx, uly, lrx, lry) or None.  tra / ocr: the page's two aligned lists
    (None for a gap); o_line / ocr_boxes: per OCR character its text line and its box; refined: {line: (t_first, L,
    boxes)} of the refined lines, boxes being the L boxes of the line's kept transcript characters t_first .. + L.
    A kept character of a refined line gets that line's box for it; any other character the box of the OCR character it
    shares a column with -- unless there is none, or that OCR character lies on a refined line."""
    kept = {}
    for t_first, L, boxes in refined.values():
        for k in range(L):
            kept[t_first + k] = tuple(int(v) for v in boxes[k])
    out, i, j = [], 0, 0
    for t, o in zip(tra, ocr):
        if t is not None:
            if i in kept:
                out.append(kept[i])
            elif o is not None and o_line[j] not in refined:
                out.append(tuple(int(v) for v in ocr_boxes[j]))
            else:
                out.append(None)
            i += 1
        if o is not None:
            j += 1
    return out


def syllable_box(boxes, first, last):
    """the box of a syllable over the transcript characters first .. last, before the rotation back: the largest uly
    under it, the union of the boxes with that uly; None if no character under it has a box"""
    have = [b for b in boxes[first:last + 1] if b is not None]
    if not have:
        return None
    low = max(b[1] for b in have)
    on = [b for b in have if b[1] == low]
    return (min(b[0] for b in on), min(b[1] for b in on), max(b[2] for b in on), max(b[3] for b in on))


def peak_boxes(t_peak, T, raw_w, x_min, y_min, y_max, pad):
    """one line's boxes for the entries (t_peak[i], .): x = (t - pad) raw_w / (T - 2 pad) as the .llocs file carries it
    (one decimal), plus x_min, rounded half to even; a box runs from the previous position (the strip's x_min for the
    first) to its own, over the strip's y_min .. y_max"""
    out, left = [], int(x_min)
    for t in t_peak:
        x = (float(t) - pad) * (float(raw_w) / (T - 2 * pad))
        right = int(np.round(float("%.1f" % x) + x_min))
        out.append((left, int(y_min), right, int(y_max)))
        left = right
    return out
