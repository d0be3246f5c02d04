"""The cases of page-scope forced alignment with omission that tests/test_forced_page_omit_sim.py (the host build of
csrc/ta_forced_page_omit.hip) and tests/test_forced_page_omit_gpu.py (the real kernel) share, the layout both drive the
kernel with (forced_page_cases.pack: gaps, labels of 999 around the texts, pieces 16 bytes apart, everything poisoned),
and the checker's answers (tests/forced_page_omit_ref.py), computed once per process.

A case is (name, no, omit, [page, ...]); a page is (Ps, cs, lo, hi) as in forced_page_cases.  Each case is the smallest
shape at which its mechanism can fail.  The scripted pages (`_ink`) make the recogniser's rows say which characters the
page holds, so that the best path provably omits the others: tests/test_forced_page_omit_sim.py checks on the checker's
own path that every such case exercises the move it was written for.
"""
import numpy as np

import forced_page_cases as PC
import forced_page_omit_ref as R
import forced_page_ref as PR
from text_alignment_amd import _abi

UNIT = 1 << 16
POISON32, POISON64, POISON_BYTE = PC.POISON32, PC.POISON64, PC.POISON_BYTE
STRICT = "strict: "                  # the cases whose answer is forced_page_ref's as well
KS = (2, 4, 8, 16, 32)                       # the variants built
WIDTH = {2: 40, 4: 100, 8: 200, 16: 400, 32: 600}      # a window that asks for each
probs, text, _page = PC.probs, PC.text, PC._page


def bind(lib):
    return _abi.bind(lib, ["ta_forced_page_omit_workspace_bytes", "ta_forced_align_pages_omit"])


def _ink(classes, no, hot=0.9):
    """rows that say class c at every frame of `classes`: hot for c, the rest shared among the others"""
    P = np.full((len(classes), no), (1.0 - hot) / (no - 1), np.float32)
    P[np.arange(len(classes)), np.asarray(classes)] = hot
    return P


def break_run(K, run, frames0=6):
    """two lines, a window that asks for variant K, and `run` characters of the text that the page lacks between the
    last character of line 0 and the first of line 1 -- the run in class 4, the filler in class 5, the ink in 1 .. 3 and
    without a blank, so the path's move at line 1's first frame is ONE far move over the run (for run 0: an advance or
    skip).  The text starts with K / 2 + 1 characters of filler (an absent prefix) and ends with filler up to the
    window's width (an absent suffix); the second window starts in the middle of the run.  frames0: the frames of line 0."""
    no, w = 6, WIDTH[K]
    a0 = K // 2 + 1
    ink = [1, 2, 3, 1, 2, 3]
    cs = [5] * a0 + ink[:3] + [4] * run + ink[3:]
    n = w + 5
    cs += [5] * (n - len(cs))
    per = frames0 // 3
    line0 = [c for c in ink[:3] for _ in range(per)] + [ink[2]] * (frames0 - 3 * per)
    line1 = [c for c in ink[3:] for _ in range(2)]
    lo1 = a0 + 3 + run // 2
    return [_ink(line0, no), _ink(line1, no)], np.asarray(cs, np.int32), [0, lo1], [w, n]


def far_first_frame():
    """far moves on a line's first frame, by where they start: (a) the blank 2 lo_new - 2 -- a candidate that can only
    tie, with the path through the blank 2 lo_new, and the tie order takes the other; (b) a label several states below the
    new window; (c) with a shift of more than K states, a source in lane >= 1 of the old layout"""
    no = 6
    # (a) text 1 2 [4] 3 1: line 0 ends in the blank behind '2', line 1 starts with '3'; the window starts at '3'
    a = ([_ink([1, 1, 2, 2, 0], no), _ink([3, 3, 1, 1], no)], np.asarray([1, 2, 4, 3, 1], np.int32), [0, 3], [4, 5])
    # (b) text 1 2 [4 4 4] 3 1: line 0 ends IN '2' (state 3), the new window starts at '3' (state 10)
    b = ([_ink([1, 1, 2, 2], no), _ink([3, 3, 1, 1], no)], np.asarray([1, 2, 4, 4, 4, 3, 1], np.int32), [0, 5], [6, 7])
    # (c) K = 4 (a window of 100): line 0 ends in character 8 (old state 17, lane 4), twelve absent, a shift of 40 states
    cs = [5] * 6 + [1, 2, 3] + [4] * 12 + [1, 2, 3]
    cs += [5] * (105 - len(cs))
    c = ([_ink([1, 1, 2, 2, 3, 3], no), _ink([1, 1, 2, 2, 3, 3], no)], np.asarray(cs, np.int32), [0, 20], [100, 105])
    return [a, b, c]


def equal_across_break():
    """text 1 [2] 1, the 2 absent: the far move at the break joins two EQUAL labels -- allowed, where a skip is not"""
    no = 4
    return [([_ink([1, 1], no), _ink([1, 1], no)], np.asarray([1, 2, 1], np.int32), [0, 0], [3, 3]),
            ([_ink([1, 1, 1], no), _ink([1], no)], np.asarray([3, 1, 2, 1, 3], np.int32), [0, 2], [4, 5])]


def prefix_suffix():
    """the ink holds only the middle of the text: the path starts above state 1 and ends far below 2 n"""
    no = 6
    cs = np.asarray([4] * 7 + [1, 2, 3] + [5] * 9, np.int32)
    return [([_ink([1, 1, 0, 2, 2, 3, 3], no)], cs, [0], [len(cs)]),
            ([_ink([1, 1, 2], no), _ink([2, 0, 3, 3], no)], cs, [0, 6], [12, len(cs)])]


def _wide(rng, w, T=None, no=6):
    """a line with a window of w characters and few frames (more characters than frames), a short line with a narrow
    window behind it"""
    n = w + 3
    return _page(rng, (w // 2 + 11 if T is None else T, 12), n, (0, w - 2), (w, n), no)


def cases():
    rng = np.random.default_rng(1412)
    out = []
    one = [_page(rng, (T,), n, (0,), (n,), 5) for T in (1, 3, 8, 9, 31, 32, 33, 65) for n in (1, 3)]      # n > T included
    out.append(("one line", 5, 3 * UNIT, one))
    out.append(("more characters than frames", 5, 2 * UNIT, [_page(rng, (2, 2, 2), 20, (0, 5, 12), (9, 16, 20), 5),
                                                            _page(rng, (1, 1), 9, (0, 2), (6, 9), 5)]))
    shifts = [
        _page(rng, (12, 11), 8, (0, 4), (4, 8), 7),                       # windows that share no character
        _page(rng, (12, 11), 8, (0, 3), (4, 8), 7),                       # one
        _page(rng, (14, 13, 9), 9, (0, 1, 2), (8, 9, 9), 7),              # many
        _page(rng, (10, 10), 7, (0, 3), (5, 7), 7),                       # an odd shift: every state changes lane and register
        _page(rng, (10, 9, 11), 9, (0, 1, 6), (5, 6, 9), 7),              # odd shifts, three lines
        _page(rng, (3, 2, 4), 30, (0, 7, 18), (11, 22, 30), 7),           # long shifts, more characters than frames
    ]
    out.append(("window shifts", 7, 2 * UNIT, shifts))
    out.append(("window shifts, dear", 7, 9 * UNIT, shifts))
    empty = [
        _page(rng, (3, 8), 4, (0, 0), (0, 4), 7),                         # an empty FIRST window
        _page(rng, (9, 4, 9), 6, (0, 3, 3), (3, 3, 6), 7),                # an empty window in the middle
        _page(rng, (5, 6), 4, (0, 4), (4, 4), 7),                         # an empty LAST window
        _page(rng, (2, 1, 2), 9, (0, 0, 5), (0, 5, 9), 7),                # the same with fewer frames than characters
    ]
    out.append(("empty windows", 7, 2 * UNIT, empty))
    out.append(("lines of one frame", 7, UNIT, [_page(rng, (9, 1, 9), 6, (0, 2, 3), (4, 4, 6), 7),
                                                _page(rng, (1, 1, 1, 1), 3, (0, 0, 0, 0), (3, 3, 3, 3), 7),
                                                _page(rng, (1, 1, 1), 12, (0, 3, 7), (5, 9, 12), 7)]))
    out.append(("far on a first frame", 6, 2 * UNIT, far_first_frame()))
    out.append(("equal characters across a break", 4, UNIT, equal_across_break()))
    for K in KS:
        out.append(("absent runs K=%d" % K, 6, 2 * UNIT, [break_run(K, K // 2 + e) for e in (-1, 0, 1)]))
    out.append(("absent prefix and suffix", 6, 2 * UNIT, prefix_suffix()))
    out.append(("walk blocks", 6, 2 * UNIT, [break_run(2, 3, frames0=T) for T in (31, 32, 33)]))
    out.append(("chunk edges", 6, 2 * UNIT, [_page(rng, (7, 8, 9), 14, (0, 3, 8), (6, 11, 14), 6),
                                             _page(rng, (9, 8, 7), 30, (0, 8, 19), (12, 24, 30), 6),
                                             _page(rng, (8, 16, 17), 11, (0, 2, 6), (5, 9, 11), 6)]))
    for w in (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513):
        out.append(("window %d" % w, 6, 2 * UNIT, [_wide(rng, w)]))
    n = 1027
    out.append(("window 1023", 6, 2 * UNIT, [_page(rng, (2100, 20), n, (0, 1019), (1023, n), 6)]))
    out.append(("mixed K", 6, 2 * UNIT, [_wide(rng, 70), _page(rng, (12, 11), 8, (0, 3), (4, 8), 6), _wide(rng, 130),
                                         break_run(16, 8), _page(rng, (20,), 4, (0,), (4,), 6), break_run(32, 17)]))
    u = lambda T: np.full((T, 4), 0.25, np.float32)                        # noqa: E731
    ties = [([u(9)], np.asarray([1, 2, 3], np.int32), [0], [3]),
            ([u(4), u(5)], np.asarray([1, 2, 3], np.int32), [0, 1], [2, 3]),
            ([u(6), u(1), u(6)], np.asarray([1, 1, 2, 2], np.int32), [0, 1, 1], [3, 3, 4]),
            ([u(2), u(2)], np.asarray([1, 2, 3, 1, 2, 3, 1], np.int32), [0, 3], [5, 7])]
    out.append(("all ties, omit 0", 4, 0, ties))
    out.append(("all ties", 4, UNIT, ties))
    out.append(("omit 0", 7, 0, shifts + empty))
    for name, no, pages in PC.cases():                 # what has a strict path and at most 40 frames: priced out, the same answer
        kept = [pg for pg in pages if sum(len(P) for P in pg[0]) <= 40 and PR.align_page(*pg)[0] == PR.OK]
        if kept:
            out.append((STRICT + name, no, 1 << 26, kept))
    zeros = dict((c[0], c) for c in PC.cases())["zeros and NaN"]
    out.append(("zeros and NaN", 5, 2 * UNIT, zeros[2]))
    return out


_WANT = {}


def want(name, pages, omit):
    """the checker's [(status, score, frames)] of a case, computed once"""
    if name not in _WANT:
        _WANT[name] = [R.answer(*pg, omit) for pg in pages]
    return _WANT[name]


class _Sizes(object):
    """forced_page_cases.pack sizes the pieces with ta_forced_page_workspace_bytes: here the entry with omission's"""
    def __init__(self, lib):
        self.ta_forced_page_workspace_bytes = lib.ta_forced_page_omit_workspace_bytes


def pack(lib, pages, no):
    return PC.pack(_Sizes(lib), pages, no)


INPUTS, OUTPUTS, HOST = PC.INPUTS, PC.OUTPUTS, PC.HOST
check = PC.check


def call(lib, pk, ptr, omit, stream=None, **over):
    """ta_forced_align_pages_omit on pk's arrays, as forced_page_cases.call"""
    a = dict(npages=pk.npages, nlines=pk.nlines, no=pk.no, rows=pk.rows, nlabels=pk.nlabels, T_host=pk.T,
             line_first_host=pk.line_first, lo_host=pk.lo, hi_host=pk.hi, lab_off_host=pk.lab_off,
             workspace=ptr("ws"), workspace_bytes=pk.ws_bytes, omit_q=omit)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    keep = []
    for name in HOST:
        if isinstance(a[name], np.ndarray):
            keep.append(np.ascontiguousarray(a[name]))
            a[name] = keep[-1].ctypes.data
    return lib.ta_forced_align_pages_omit(
        a["probs"], a["row_off"], a["T"], a["line_first"], a["lo"], a["hi"], a["labels"], a["lab_off"], a["ws_off"],
        a["npages"], a["nlines"], a["no"], a["rows"], a["nlabels"], a["T_host"], a["line_first_host"], a["lo_host"],
        a["hi_host"], a["lab_off_host"], a["omit_q"], a["workspace"], a["workspace_bytes"], a["frames"], a["score"],
        a["status"], stream)


def strict_want(pages):
    """forced_page_ref's answers, for the case that prices an omission out"""
    return [PR.align_page(*pg)[:3] for pg in pages]
