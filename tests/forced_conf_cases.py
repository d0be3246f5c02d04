"""The confidence cases that tests/test_forced_conf_sim.py (the host build of csrc/ta_forced_conf.hip) and
tests/test_forced_conf_gpu.py (the real kernel) share, the layout both drive it with, and the checker's answers, computed
once per process.

The lines are tests/forced_cases.py's (every variant K at both edges, T = S, walk-block edges, repeats, no = 2 / 128,
zeros / NaN, all ties) plus lines whose T is and is not a multiple of the emission chunk (8) at either end, for the
backward fill's chunk walk.  Every line is queried twice: at the aligner's own t_peak ("peak") and at a seeded set of
frames that never decreases, has equal neighbours and holds 0 and T - 1 ("seeded").  `pack` is forced_cases.pack with the
queries (gaps of -7 between the lines), and the two outputs poisoned.
"""
import numpy as np

import forced_cases as C0
import forced_conf_ref as R
from text_alignment_amd import _abi

POISON32, POISON64, POISON_BYTE = C0.POISON32, C0.POISON64, C0.POISON_BYTE
SETS = ("peak", "seeded")


def bind(lib):
    return _abi.bind(lib, ["ta_forced_confidence_workspace_bytes", "ta_forced_confidence"])


def cases():
    """[(name, no, lines)]: forced_cases.cases() and the chunk edges"""
    rng = np.random.default_rng(1410)
    out = list(C0.cases())
    out.append(("chunk edges", 5, [(C0.probs(rng, T, 5), C0.text(rng, L, 5))
                                   for T, L in ((7, 3), (8, 3), (9, 4), (15, 7), (16, 3), (17, 8), (23, 5), (24, 1))]))
    return out


def seeded_queries(rng, T, L):
    """L frames in 0 .. T - 1 that never decrease, with equal neighbours, the first 0 and the last T - 1 (L = 1: T - 1)"""
    tq = rng.integers(0, T, size=L)
    same = rng.random(L) < 0.3
    for i in range(1, L):
        if same[i]:
            tq[i] = tq[i - 1]
    tq = np.sort(tq)
    tq[0], tq[-1] = 0, T - 1
    return tq.astype(np.int32)


def queries(name, lines, which):
    """per line its query frames of the set `which`"""
    if which == "peak":
        frames, _ = C0.want(name, lines)
        off = np.cumsum([0] + [len(cs) for _, cs in lines])
        return [frames[a:b, 2].astype(np.int32) for a, b in zip(off[:-1], off[1:])]
    rng = np.random.default_rng(sum(name.encode()) + 77)
    return [seeded_queries(rng, len(P), len(cs)) for P, cs in lines]


_WANT = {}


def want(name, lines):
    """{set: (queries per line, confidence, rival)} of a case from the checker, the tables of a line computed once"""
    if name not in _WANT:
        qs = {w: queries(name, lines, w) for w in SETS}
        got = {w: [] for w in SETS}
        for k, (P, cs) in enumerate(lines):
            G = R.tables(P, cs)[2]
            for w in SETS:
                got[w].append(R.query_tables(G, qs[w][k])[:2])
        _WANT[name] = {w: (qs[w], np.concatenate([c for c, _ in got[w]]), np.concatenate([r for _, r in got[w]]))
                       for w in SETS}
    return _WANT[name]


class _Sizes(object):
    """forced_cases.pack asks its library for the workspace pieces under the aligner's name"""

    def __init__(self, lib):
        self.ta_forced_workspace_bytes = lib.ta_forced_confidence_workspace_bytes


def pack(lib, lines, no, tqs, **edits):
    """forced_cases.pack (rows, labels and workspace pieces with gaps) plus the queries and the poisoned outputs"""
    pk = C0.pack(_Sizes(lib), lines, no, **edits)
    pk.t_query = np.full(pk.nlabels, -7, np.int32)
    for o, tq in zip(pk.lab_off, tqs):
        pk.t_query[o:o + len(tq)] = tq
    pk.confidence = np.full(pk.nlabels, POISON64, np.int64)
    pk.rival = np.full(pk.nlabels, POISON32, np.int32)
    del pk.frames, pk.score
    return pk


INPUTS = C0.INPUTS + ("t_query",)
OUTPUTS = ("confidence", "rival", "status")


def call(lib, pk, ptr, stream=None, **over):
    """ta_forced_confidence on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to replace
    (forced_cases.refusals' `frames` stands for the first output here)"""
    a = dict(nlines=pk.n, no=pk.no, rows=pk.rows, nlabels=pk.nlabels, T_host=pk.T_host.ctypes.data,
             L_host=pk.L_host.ctypes.data, workspace=ptr("ws"), workspace_bytes=pk.ws_bytes)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    if "frames" in over:
        over = dict(over)
        over["confidence"] = over.pop("frames")
    a.update(over)
    for name in ("T_host", "L_host"):
        if isinstance(a[name], np.ndarray):
            a[name] = a[name].ctypes.data
    return lib.ta_forced_confidence(a["probs"], a["row_off"], a["T"], a["labels"], a["lab_off"], a["L"], a["ws_off"],
                                    a["t_query"], a["nlines"], a["no"], a["rows"], a["nlabels"], a["T_host"], a["L_host"],
                                    a["workspace"], a["workspace_bytes"], a["confidence"], a["rival"], a["status"], stream)


def gather(pk, out, poison):
    """the lines' own rows of an output, line after line; everything else must still be poison"""
    own = np.zeros(len(out), dtype=bool)
    for o, l in zip(pk.lab_off, pk.L_host):
        own[o:o + l] = True
    assert (out[~own] == poison).all(), "a row outside every line was written"
    return out[own]
