"""The cases of the confidence on the lattice with omission that tests/test_forced_omit_conf_sim.py (the host build of
csrc/ta_forced_omit_conf.hip) and tests/test_forced_omit_conf_gpu.py (the real kernel) share, the layout both drive it
with, and the checker's answers, computed once per process.

A case is (name, no, omit, [(P, cs), ...]).  The lines are tests/forced_omit_cases.py's (every variant K at both edges at
T = 2 L + 1 and 2 L + 38, L = 1023, absent runs inside a lane, over one lane boundary and over many, `a b a`, an absent
prefix and suffix, ties) plus lines whose T is and is not a multiple of the emission chunk (8) at either end, for the
backward fill's chunk walk, and a set of lines -- random, with an absent run, and constant, where all candidates tie -- at
each of four prices.  Every line is queried twice: by the host's rule on the checker's own frames ("rule") and by a seeded
list ("seeded") of 0, 1, L or 2 L queries with repeated frames, frames 0 and T - 1 and several queries per character.
`pack` is forced_cases.pack's layout (gaps in front of every line's rows and labels) with the queries (gaps of -7 between
the lines' pieces of q_char / q_frame) and the poisoned outputs and workspace.
"""
import numpy as np

import forced_cases as C0
import forced_omit_cases as C1
import forced_omit_conf_ref as R
from text_alignment_amd import _abi

POISON32, POISON64, POISON_BYTE = C0.POISON32, C0.POISON64, C0.POISON_BYTE
UNIT = C1.UNIT
SETS = ("rule", "seeded")
OMITS = (0, UNIT, 4 * UNIT, 1 << 26)
ABSENT_AT_4_BITS = "absent"       # the cases of this prefix must hold omitted AND present characters (their price is 4 bits)


def bind(lib):
    return _abi.bind(lib, ["ta_forced_omit_confidence_workspace_bytes", "ta_forced_omit_confidence"])


def cases():
    rng = np.random.default_rng(1418)
    line = lambda T, L, no: (C0.probs(rng, T, no), C0.text(rng, L, no))                             # noqa: E731
    const = lambda T, cs, no: (np.full((T, no), 1.0 / no, np.float32), np.asarray(cs, np.int32))    # noqa: E731
    out = list(C1.cases())
    out.append(("chunk edges", 5, 3 * UNIT, [line(T, L, 5) for T, L in ((7, 3), (8, 3), (9, 2), (15, 3), (16, 1), (17, 3),
                                                                         (23, 2), (24, 3))]))
    for omit in OMITS:
        out.append(("price %d" % omit, 6, omit, [line(9, 3, 6), line(40, 12, 6), line(150, 66, 6), C1.absent(rng, 30, 6, 10, 5)]))
        out.append(("price %d constant" % omit, 4, omit, [const(9, [1, 2, 3], 4), const(8, [1, 1], 4), const(3, [2], 4),
                                                          const(140, [1, 2, 3] * 22, 4)]))
    return out


NQ_KINDS = ("0", "1", "L", "2L")


def nq_kind(name, k):
    """which of the four query counts line k of a case takes in the seeded set"""
    return NQ_KINDS[(sum(name.encode()) + k) % 4]


def seeded_queries(rng, T, L, kind):
    """(q_char, q_frame) int32: 0, 1, L or 2 L queries; frames that never decrease, with equal neighbours, the first 0 and
    the last T - 1 (a single query: T - 1); characters at random, the first two queries on the same one"""
    nq = {"0": 0, "1": 1, "L": L, "2L": 2 * L}[kind]
    qf = rng.integers(0, T, size=nq)
    same = rng.random(nq) < 0.3
    for j in range(1, nq):
        if same[j]:
            qf[j] = qf[j - 1]
    qf = np.sort(qf)
    if nq:
        qf[0], qf[-1] = 0, T - 1
    qc = rng.integers(0, L, size=nq)
    if nq >= 2:
        qc[1] = qc[0]
    return qc.astype(np.int32), qf.astype(np.int32)


def rule_queries(frames, T):
    """(q_char, q_frame) int32 of a line by the host's rule, the checker's omit_queries"""
    got = R.omit_queries(frames, T)
    return np.asarray([i for i, _ in got], np.int32), np.asarray([t for _, t in got], np.int32)


def line_frames(name, lines, omit):
    """per line its frames (L, 3) from the aligner's checker (forced_omit_cases.want, computed once)"""
    frames, _ = C1.want(name, lines, omit)
    off = np.cumsum([0] + [len(cs) for _, cs in lines])
    return [frames[a:b] for a, b in zip(off[:-1], off[1:])]


_WANT = {}


def want(name, lines, omit):
    """{set: (queries per line, confidence, rival)} of a case from the checker, the tables of a line computed once"""
    if name not in _WANT:
        rng = np.random.default_rng(sum(name.encode()) + 99)
        fr = line_frames(name, lines, omit)
        qs = {"rule": [rule_queries(f, len(P)) for f, (P, _) in zip(fr, lines)],
              "seeded": [seeded_queries(rng, len(P), len(cs), nq_kind(name, k)) for k, (P, cs) in enumerate(lines)]}
        got = {w: [] for w in SETS}
        for k, (P, cs) in enumerate(lines):
            G = R.tables_closed(P, cs, omit)[2]
            for w in SETS:
                got[w].append(R.query_list(G, *qs[w][k]))
        _WANT[name] = {w: (qs[w], np.concatenate([c for c, _ in got[w]]), np.concatenate([r for _, r in got[w]]))
                       for w in SETS}
    return _WANT[name]


class _NoSizes(object):
    """forced_cases.pack asks a library for the workspace pieces; here they depend on the queries and are laid out below"""

    @staticmethod
    def ta_forced_workspace_bytes(T, L):
        return 16


def pack(lib, lines, no, qs, nq_dev=None, **edits):
    """forced_cases.pack (rows and labels with gaps) plus the queries, the workspace pieces (from byte 256, 16 bytes apart)
    and the poisoned outputs.  qs: per line (q_char, q_frame); nq_dev: {line: value} for the device's copy of nq alone"""
    pk = C0.pack(_NoSizes, lines, no, **edits)
    del pk.frames, pk.score
    pk.nq_host = np.asarray([len(qc) for qc, _ in qs], np.int32)
    pk.nq = pk.nq_host.copy()
    for k, v in (nq_dev or {}).items():
        pk.nq[k] = v
    need = [int(lib.ta_forced_omit_confidence_workspace_bytes(int(t), int(l), int(n)))
            for t, l, n in zip(pk.T_host, pk.L_host, pk.nq_host)]
    assert min(need) >= 0
    off, ws_off = 256, []
    for b in need:
        ws_off.append(off)
        off += b + 16
    pk.ws_off, pk.ws_bytes = np.asarray(ws_off, np.int64), off
    pk.ws = np.full(pk.ws_bytes, POISON_BYTE, np.uint8)
    qcs, qfs, q_off, nqs = [], [], [], 0
    for k, (qc, qf) in enumerate(qs):
        gap = 1 + k % 2
        qcs.append(np.full(gap, -7, np.int32))
        qfs.append(np.full(gap, -7, np.int32))
        nqs += gap
        q_off.append(nqs)
        qcs.append(np.asarray(qc, np.int32))
        qfs.append(np.asarray(qf, np.int32))
        nqs += len(qc)
    pk.q_char = np.concatenate(qcs + [np.full(2, -7, np.int32)])
    pk.q_frame = np.concatenate(qfs + [np.full(2, -7, np.int32)])
    pk.q_off, pk.nqueries = np.asarray(q_off, np.int64), nqs + 2
    pk.confidence = np.full(pk.nqueries, POISON64, np.int64)
    pk.rival = np.full(pk.nqueries, POISON32, np.int32)
    return pk


INPUTS = C0.INPUTS + ("q_char", "q_frame", "q_off", "nq")
OUTPUTS = ("confidence", "rival", "status")


def call(lib, pk, ptr, omit, stream=None, **over):
    """ta_forced_omit_confidence on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to replace
    (forced_cases.refusals' `frames` stands for the first output here)"""
    a = dict(nlines=pk.n, no=pk.no, rows=pk.rows, nlabels=pk.nlabels, nqueries=pk.nqueries, T_host=pk.T_host, L_host=pk.L_host,
             nq_host=pk.nq_host, workspace=ptr("ws"), workspace_bytes=pk.ws_bytes, omit_q=omit)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    if "frames" in over:
        over = dict(over)
        over["confidence"] = over.pop("frames")
    a.update(over)
    for name in ("T_host", "L_host", "nq_host"):
        if isinstance(a[name], np.ndarray):
            a[name] = a[name].ctypes.data
    return lib.ta_forced_omit_confidence(a["probs"], a["row_off"], a["T"], a["labels"], a["lab_off"], a["L"], a["ws_off"],
                                         a["q_char"], a["q_frame"], a["q_off"], a["nq"], a["nlines"], a["no"], a["rows"],
                                         a["nlabels"], a["nqueries"], a["T_host"], a["L_host"], a["nq_host"], a["omit_q"],
                                         a["workspace"], a["workspace_bytes"], a["confidence"], a["rival"], a["status"], stream)


def gather(pk, out, poison):
    """the lines' own rows of an output, line after line; everything else must still be poison"""
    own = np.zeros(len(out), dtype=bool)
    for o, n in zip(pk.q_off, pk.nq_host):
        own[o:o + n] = True
    assert (out[~own] == poison).all(), "a row outside every line's queries was written"
    return out[own]


def pieces(lib, pk):
    """a mask of the workspace bytes that lie in a line's piece"""
    piece = np.zeros(pk.ws_bytes, dtype=bool)
    for o, t, l, n in zip(pk.ws_off, pk.T_host, pk.L_host, pk.nq_host):
        piece[o:o + lib.ta_forced_omit_confidence_workspace_bytes(int(t), int(l), int(n))] = True
    return piece


def refusals(pk):
    """forced_omit_cases.refusals (forced_cases' and omit_q out of range) plus what the queries add"""
    def arr(base, k, v):
        a = base.copy()
        a[k] = v
        return a
    return C1.refusals(pk) + [("null q_char", -1, dict(q_char=None)), ("null q_frame", -1, dict(q_frame=None)),
                              ("null q_off", -1, dict(q_off=None)), ("null nq", -1, dict(nq=None)),
                              ("null nq_host", -1, dict(nq_host=None)), ("null rival", -1, dict(rival=None)),
                              ("negative nqueries", -1, dict(nqueries=-1)),
                              ("nqueries too few", -1, dict(nqueries=int(pk.nq_host.sum()) - 1)),
                              ("nq = -1", -1, dict(nq_host=arr(pk.nq_host, 0, -1))),
                              ("nq = 2 L + 1", -1, dict(nq_host=arr(pk.nq_host, 1, 2 * int(pk.L_host[1]) + 1)))]


# the good lines and the refused one of the tests of a line between good ones
def three(rng):
    return [(C0.probs(rng, 30, 6), C0.text(rng, 7, 6)), (C0.probs(rng, 21, 6), C0.text(rng, 5, 6)),
            (C0.probs(rng, 140, 6), C0.text(rng, 66, 6))]


def three_queries(rng, lines):
    return [seeded_queries(rng, len(P), len(cs), kind) for (P, cs), kind in zip(lines, ("2L", "L", "L"))]
