"""The page-scope forced-alignment cases that tests/test_forced_page.py (the checker against brute force),
tests/test_forced_page_sim.py (the host build of csrc/ta_forced_page.hip) and tests/test_forced_page_gpu.py (the real
kernel) share, the layout the last two drive the kernel with, and the checker's answers, computed once per process.

A case is (name, no, [page, ...]); a page is (Ps, cs, lo, hi): the lines' probability rows, the page's labels and a window
of characters per line.  `pack` lays a case out the way a caller would not: rows and labels with gaps in front of every
line (rows of 0.5) and labels of 999 -- a label no page may read -- around the pages' texts, workspace pieces that start
at byte 256 and are 16 bytes apart; `call` runs ta_forced_align_pages on it with every output and the workspace poisoned.
"""
import numpy as np

import forced_cases as FC
import forced_page_ref as R
from text_alignment_amd import _abi

POISON32, POISON64, POISON_BYTE = FC.POISON32, FC.POISON64, FC.POISON_BYTE
probs, text = FC.probs, FC.text


def bind(lib):
    return _abi.bind(lib, ["ta_forced_page_workspace_bytes", "ta_forced_page_variant", "ta_forced_align_pages"])


def variant(width):
    """states per lane for a window of `width` characters (forced_k of its 2 width + 1 states)"""
    S = 2 * width + 1
    return 2 if S <= 128 else 4 if S <= 256 else 8 if S <= 512 else 16 if S <= 1024 else 32


def _page(rng, Ts, n, lo, hi, no):
    return [probs(rng, T, no) for T in Ts], text(rng, n, no), list(lo), list(hi)


def _wide(rng, w, no=6):
    """a line with a window of w characters and T = 2 w + 11 frames, and a short line with a narrow window behind it"""
    n = w + 3
    return _page(rng, (2 * w + 11, 12), n, (0, w - 2), (w, n), no)


def break_case():
    """one character, two lines of two frames, the character likely everywhere: the unconstrained lattice keeps it over
    the line break, the rule forbids that"""
    P = np.asarray([[0.1, 0.9]] * 2, np.float32)
    return [P, P.copy()], np.asarray([1], np.int32), [0, 0], [1, 1]


def cases():
    rng = np.random.default_rng(1409)
    out = []
    one = []
    for T in (1, 7, 8, 9, 31, 32, 33, 65):            # the chunk's and the walk block's edges
        for n in sorted({1, max(1, (T - 1) // 2)}):
            one.append(_page(rng, (T,), n, (0,), (n,), 5))
    out.append(("one line", 5, one))
    out.append(("overlaps", 7, [
        _page(rng, (12, 11), 8, (0, 4), (4, 8), 7),                       # windows that share no character
        _page(rng, (12, 11), 8, (0, 3), (4, 8), 7),                       # one
        _page(rng, (14, 13, 9), 9, (0, 1, 2), (8, 9, 9), 7),              # many
        _page(rng, (10, 10), 7, (0, 3), (5, 7), 7),                       # an odd shift: every state changes lane and register
        _page(rng, (10, 9, 11), 9, (0, 1, 6), (5, 6, 9), 7),              # odd shifts, three lines
        _page(rng, (9, 4, 9), 6, (0, 3, 3), (3, 3, 6), 7),                # an empty window in the middle
        _page(rng, (9, 1, 9), 6, (0, 2, 3), (4, 4, 6), 7),                # a line of one frame
        _page(rng, (1, 1, 1, 1), 3, (0, 0, 0, 0), (3, 3, 3, 3), 7),       # nothing but lines of one frame
        _page(rng, (5, 6), 4, (0, 4), (4, 4), 7),                         # an empty LAST window: the end is the last blank
        _page(rng, (3, 8), 4, (0, 0), (0, 4), 7),                         # an empty FIRST window
    ]))
    out.append(("straddling", 6, [
        _page(rng, (5, 13, 37, 30), 20, (0, 0, 3, 9), (6, 12, 20, 20), 6),       # chunks of 8 and blocks of 32 across the breaks
        _page(rng, (31, 33, 3), 25, (0, 10, 22), (14, 25, 25), 6),
        _page(rng, (9, 7, 8, 1, 15, 17), 18, (0, 1, 2, 5, 5, 11), (6, 7, 9, 9, 16, 18), 6),
    ]))
    for w in (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513):
        out.append(("window %d" % w, 6, [_wide(rng, w)]))
    n = 1027
    out.append(("window 1023", 6, [_page(rng, (2100, 20), n, (0, 1019), (1023, n), 6)]))
    out.append(("mixed K", 6, [_wide(rng, 70), _page(rng, (12, 11), 8, (0, 3), (4, 8), 6), _wide(rng, 130),
                               _page(rng, (20,), 4, (0,), (4,), 6)]))
    u = lambda T: np.full((T, 4), 0.25, np.float32)                        # noqa: E731
    out.append(("all ties", 4, [([u(9)], np.asarray([1, 2, 3], np.int32), [0], [3]),
                                ([u(4), u(5)], np.asarray([1, 2, 3], np.int32), [0, 1], [2, 3]),
                                ([u(6), u(1), u(6)], np.asarray([1, 1, 2, 2], np.int32), [0, 1, 1], [3, 3, 4])]))
    out.append(("repeats", 4, [([probs(rng, 7, 4), probs(rng, 6, 4)], np.asarray([2, 2, 2, 3, 3], np.int32), [0, 1], [3, 5]),
                               ([probs(rng, 5, 4), probs(rng, 4, 4)], np.asarray([2, 2, 2], np.int32), [0, 0], [3, 3])]))
    out.append(("ends in 2n-1", 6, [([probs(rng, 4, 6)], np.asarray([1, 2, 3, 4], np.int32), [0], [4]),
                                    ([probs(rng, 2, 6), probs(rng, 3, 6)], np.asarray([1, 2, 3, 4, 5], np.int32), [0, 1], [3, 5])]))
    P = probs(rng, 24, 5)
    P[3] = 0.0
    P[4] = np.nan
    P[7, 2] = np.nan
    P[9, :] = [np.inf, -1.0, 0.0, 2.0 ** -17, 2.0 ** -18]
    P[11] = 1.0
    P[12] = [1e-40, 1.5, -np.inf, -0.0, 0.999999]
    out.append(("zeros and NaN", 5, [([P[:10], P[10:]], np.asarray([1, 2, 2, 4, 3], np.int32), [0, 1], [4, 5]),
                                     ([np.zeros((4, 5), np.float32), np.zeros((5, 5), np.float32)],
                                      np.asarray([1, 1, 2], np.int32), [0, 0], [3, 3])]))
    out.append(("no path", 5, [_page(rng, (2, 1), 5, (0, 2), (4, 5), 5), _page(rng, (6, 5), 4, (0, 2), (3, 4), 5),
                               ([probs(rng, 2, 5), probs(rng, 2, 5)], np.asarray([3, 3, 3], np.int32), [0, 0], [3, 3])]))
    out.append(("line break", 2, [break_case()]))
    return out


_WANT = {}


def want(name, pages):
    """the checker's [(status, score, frames)] of a case, computed once"""
    if name not in _WANT:
        _WANT[name] = [R.align_page(*pg)[:3] for pg in pages]
    return _WANT[name]


class Packed(object):
    pass


def pack(lib, pages, no):
    """host arrays of one call"""
    pk = Packed()
    rows, labs, row_off, lab_off, T, lo, hi, line_first = [], [np.full(2, 999, np.int32)], [], [2], [], [], [], [0]
    nr, nlab = 0, 2
    q = 0
    for p, (Ps, cs, los, his) in enumerate(pages):
        for k, P in enumerate(Ps):
            gap = 1 + q % 3
            rows.append(np.full((gap, no), 0.5, np.float32))
            nr += gap
            row_off.append(nr)
            rows.append(np.asarray(P, np.float32))
            nr += len(P)
            T.append(len(P))
            q += 1
        lo += [int(v) for v in los]
        hi += [int(v) for v in his]
        line_first.append(q)
        labs.append(np.array(cs, dtype=np.int32))
        nlab += len(cs)
        lab_off.append(nlab)
    rows.append(np.full((2, no), 0.5, np.float32))
    labs.append(np.full(3, 999, np.int32))
    pk.probs = np.ascontiguousarray(np.concatenate(rows))
    pk.labels = np.concatenate(labs)
    pk.row_off = np.asarray(row_off, np.int64)
    pk.T, pk.lo, pk.hi = np.asarray(T, np.int32), np.asarray(lo, np.int32), np.asarray(hi, np.int32)
    pk.line_first = np.asarray(line_first, np.int64)
    pk.lab_off = np.asarray(lab_off, np.int64)
    pk.K = [max(variant(int(h) - int(l)) for l, h in zip(pg[2], pg[3])) for pg in pages]
    need = []
    for p in range(len(pages)):
        for k in range(int(line_first[p]), int(line_first[p + 1])):
            one = np.asarray([T[k]], np.int32)
            need.append(int(lib.ta_forced_page_workspace_bytes(1, one.ctypes.data, pk.K[p])))
    assert min(need) > 0
    off, ws_off = 256, []
    for b in need:
        ws_off.append(off)
        off += b + 16
    pk.ws_off, pk.ws_bytes = np.asarray(ws_off, np.int64), off
    pk.npages, pk.nlines, pk.no, pk.rows, pk.nlabels = len(pages), q, no, len(pk.probs), len(pk.labels)
    pk.frames = np.full((pk.nlabels, R.FIELDS), POISON32, np.int32)
    pk.score = np.full(pk.npages, POISON64, np.int64)
    pk.status = np.full(pk.npages, POISON32, np.int32)
    pk.ws = np.full(pk.ws_bytes, POISON_BYTE, np.uint8)
    return pk


INPUTS = ("probs", "row_off", "T", "line_first", "lo", "hi", "labels", "lab_off", "ws_off")
OUTPUTS = ("frames", "score", "status")
HOST = ("T_host", "line_first_host", "lo_host", "hi_host", "lab_off_host")


def call(lib, pk, ptr, stream=None, **over):
    """ta_forced_align_pages on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to replace
    (host copies as arrays)"""
    a = dict(npages=pk.npages, nlines=pk.nlines, no=pk.no, rows=pk.rows, nlabels=pk.nlabels, T_host=pk.T,
             line_first_host=pk.line_first, lo_host=pk.lo, hi_host=pk.hi, lab_off_host=pk.lab_off,
             workspace=ptr("ws"), workspace_bytes=pk.ws_bytes)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    keep = []
    for name in HOST:
        if isinstance(a[name], np.ndarray):
            keep.append(np.ascontiguousarray(a[name]))
            a[name] = keep[-1].ctypes.data
    return lib.ta_forced_align_pages(
        a["probs"], a["row_off"], a["T"], a["line_first"], a["lo"], a["hi"], a["labels"], a["lab_off"], a["ws_off"],
        a["npages"], a["nlines"], a["no"], a["rows"], a["nlabels"], a["T_host"], a["line_first_host"], a["lo_host"],
        a["hi_host"], a["lab_off_host"], a["workspace"], a["workspace_bytes"], a["frames"], a["score"], a["status"], stream)


def check(pk, want_pages):
    """every output of a call against the checker's answers; what belongs to no accepted page must still be poison"""
    own = np.zeros(len(pk.frames), dtype=bool)
    for p, (status, score, frames) in enumerate(want_pages):
        assert int(pk.status[p]) == status, (p, int(pk.status[p]), status)
        if status == R.OK:
            a = int(pk.lab_off[p])
            assert int(pk.score[p]) == score, (p, int(pk.score[p]), score)
            assert np.array_equal(pk.frames[a:a + len(frames)], frames), p
            own[a:a + len(frames)] = True
        else:
            assert int(pk.score[p]) == POISON64, p
    assert (pk.frames[~own] == POISON32).all(), "a row of frames outside every aligned page was written"
