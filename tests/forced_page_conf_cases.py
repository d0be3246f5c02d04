"""What tests/test_forced_page_conf_sim.py (the host build of csrc/ta_forced_page_conf.hip) and
tests/test_forced_page_conf_gpu.py (the real kernel) share: the cases -- tests/forced_page_cases.cases(), imported and not
edited --, the queries, the layout both drive the kernel with, and the checker's answers, computed once per process.

Every page is queried twice: at the aligner's own (line, t_peak) ("peak"; a page without a path has none and takes its
seeded queries) and at a seeded set ("seeded") that never decreases in (line, frame) order, has equal neighbours, moves on
to a later line than it has to now and then, and holds frame 0 of a line and the last frame of a line.  `pack` is
forced_page_cases.pack (rows and labels with gaps, the aligner's own workspace and outputs) plus the query rows (fields 1
and 2, which the kernel does not read, and every row outside the pages' texts hold -7), a workspace piece per page (the
first at byte 512, 16 bytes apart) and the poisoned outputs.
"""
import ctypes

import numpy as np

import forced_page_cases as C
import forced_page_conf_ref as R
import forced_page_ref as PR
from text_alignment_amd import _abi

POISON32, POISON64, POISON_BYTE = C.POISON32, C.POISON64, C.POISON_BYTE
SETS = ("peak", "seeded")
FIELDS = PR.FIELDS
cases = C.cases


def bind(lib):
    return _abi.bind(lib, ["ta_forced_page_confidence_workspace_bytes", "ta_forced_page_confidence"])


def seeded_queries(rng, Ts, n, lo, hi):
    """(line (n,), frame (n,)) int32: see the module's text"""
    nl = len(Ts)
    line = np.zeros(n, np.int32)
    k = 0
    for i in range(n):
        while i >= hi[k]:
            k += 1
        if k + 1 < nl and lo[k + 1] <= i < hi[k + 1] and rng.random() < 0.2:
            k += 1                                    # later than it has to
        line[i] = k
    frame = np.zeros(n, np.int32)
    used = sorted(set(line.tolist()))
    for k in used:
        at = np.flatnonzero(line == k)
        ts = rng.integers(0, Ts[k], size=len(at))
        same = rng.random(len(at)) < 0.3
        for j in range(1, len(at)):
            if same[j]:
                ts[j] = ts[j - 1]
        ts = np.sort(ts)
        if k == used[0]:
            ts[0] = 0
        if k == used[-1]:
            ts[-1] = Ts[k] - 1
        frame[at] = ts
    return line, frame


_WANT, _G = {}, {}


def tables(name, pages):
    """the checker's G per page of a case (None for a page without a path), computed once"""
    want(name, pages)
    return _G[name]


def want(name, pages):
    """{set: [(status, line, frame, confidence, rival, own)]} of a case from the checker, the tables of a page computed
    once; a page without a path: (NOPATH, line, frame, None, None, None)"""
    if name not in _WANT:
        _G[name] = []
        rng = np.random.default_rng(sum(name.encode()) + 1413)
        aligned = C.want(name, pages)
        got = {w: [] for w in SETS}
        for (Ps, cs, lo, hi), (status, _, frames) in zip(pages, aligned):
            seeded = seeded_queries(rng, [len(P) for P in Ps], len(cs), lo, hi)
            if status != PR.OK:
                for w in SETS:
                    got[w].append((status,) + seeded + (None, None, None))
                _G[name].append(None)
                continue
            G = R.tables(Ps, cs, lo, hi)[2]
            _G[name].append(G)
            for w, (ql, qt) in (("peak", (frames[:, 0].copy(), frames[:, 3].copy())), ("seeded", seeded)):
                got[w].append((PR.OK, ql, qt) + R.query_tables(G, lo, hi, ql, qt))
        _WANT[name] = got
    return _WANT[name]


class AlignerSizes(object):
    """forced_page_cases.pack asks its library for the aligner's workspace pieces; a host build of the confidence kernel
    alone does not export that function, so here is the header's rule: 256 bytes per row of 64 move words"""

    @staticmethod
    def ta_forced_page_workspace_bytes(nl, T, K):
        Ts = (ctypes.c_int32 * nl).from_address(T)
        return sum(256 * (2 * t if K == 32 else -(-t // (16 // K))) for t in Ts)


def pack(lib, pages, no, queries, aligner=None):
    """host arrays of one call; queries: per page (line, frame); aligner: the library forced_page_cases.pack sizes the
    aligner's workspace with (the real one; by default the rule restated above)"""
    pk = C.pack(aligner or AlignerSizes, pages, no)
    pk.query = np.full((pk.nlabels, FIELDS), -7, np.int32)
    for p, (ql, qt) in enumerate(queries):
        a = int(pk.lab_off[p])
        pk.query[a:a + len(ql), 0] = ql
        pk.query[a:a + len(qt), 3] = qt
    off, cws_off = 512, []
    pk.piece = []
    for p, pg in enumerate(pages):
        need = int(lib.ta_forced_page_confidence_workspace_bytes(len(pg[1]), pk.K[p]))
        assert need == 512 * pk.K[p] * len(pg[1])
        cws_off.append(off)
        pk.piece.append(need)
        off += need + 16
    pk.cws_off, pk.cws_bytes = np.asarray(cws_off, np.int64), off
    pk.cws = np.full(pk.cws_bytes, POISON_BYTE, np.uint8)
    pk.confidence = np.full(pk.nlabels, POISON64, np.int64)
    pk.rival = np.full(pk.nlabels, POISON32, np.int32)
    pk.cstatus = np.full(pk.npages, POISON32, np.int32)
    return pk


INPUTS = ("probs", "row_off", "T", "line_first", "lo", "hi", "labels", "lab_off", "cws_off", "query")
OUTPUTS = ("confidence", "rival", "cstatus")
HOST = C.HOST


def call(lib, pk, ptr, stream=None, **over):
    """ta_forced_page_confidence on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to
    replace (host copies as arrays)"""
    a = dict(npages=pk.npages, nlines=pk.nlines, no=pk.no, rows=pk.rows, nlabels=pk.nlabels, T_host=pk.T,
             line_first_host=pk.line_first, lo_host=pk.lo, hi_host=pk.hi, lab_off_host=pk.lab_off,
             workspace=ptr("cws"), workspace_bytes=pk.cws_bytes)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    keep = []
    for name in HOST:
        if isinstance(a[name], np.ndarray):
            keep.append(np.ascontiguousarray(a[name]))
            a[name] = keep[-1].ctypes.data
    return lib.ta_forced_page_confidence(
        a["probs"], a["row_off"], a["T"], a["line_first"], a["lo"], a["hi"], a["labels"], a["lab_off"], a["cws_off"],
        a["query"], a["npages"], a["nlines"], a["no"], a["rows"], a["nlabels"], a["T_host"], a["line_first_host"],
        a["lo_host"], a["hi_host"], a["lab_off_host"], a["workspace"], a["workspace_bytes"], a["confidence"], a["rival"],
        a["cstatus"], stream)


def untouched(pk):
    return ((pk.confidence == POISON64).all() and (pk.rival == POISON32).all() and (pk.cstatus == POISON32).all() and
            (pk.cws == POISON_BYTE).all())


def check(pk, want_pages):
    """every output of a call against [(status, line, frame, confidence, rival, own)] per page.  The rows of a page that
    is not OK, every row outside the pages' texts and the workspace outside the pieces of the pages that ran a fill (OK
    and NOPATH) must still be poison."""
    own = np.zeros(pk.nlabels, dtype=bool)
    piece = np.zeros(pk.cws_bytes, dtype=bool)
    for p, w in enumerate(want_pages):
        assert int(pk.cstatus[p]) == w[0], (p, int(pk.cstatus[p]), w[0])
        a, o = int(pk.lab_off[p]), int(pk.cws_off[p])
        if w[0] in (PR.OK, PR.NOPATH):
            piece[o:o + pk.piece[p]] = True
        if w[0] == PR.OK:
            n = len(w[3])
            assert np.array_equal(pk.confidence[a:a + n], w[3]), p
            assert np.array_equal(pk.rival[a:a + n], w[4]), p
            own[a:a + n] = True
    assert (pk.confidence[~own] == POISON64).all() and (pk.rival[~own] == POISON32).all(), \
        "a row outside every accepted page was written"
    assert (pk.cws[~piece] == POISON_BYTE).all(), "the workspace outside the pages' rows was written"
