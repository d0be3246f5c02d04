"""The cases of the omission-tolerant forced alignment that tests/test_forced_omit_sim.py (the host build of
csrc/ta_forced_omit.hip) and tests/test_forced_omit_gpu.py (the real kernel) share, the layout both drive it with
(forced_cases.pack's: gaps in front of every line, poisoned outputs and workspace) and the checker's answers, computed
once per process.

A case is (name, no, omit, [(P, cs), ...]).  The shapes are the ones at which the kernel can go wrong: every variant K
and each switch of K, the chunk of 8 and the walk block of 32, far moves that stay inside a lane, cross one lane boundary
and cross many, an absent prefix / suffix (the start and the end rule), a far move between equal labels, and ties.
"""
import numpy as np

import forced_cases as C
import forced_omit_ref as R
from text_alignment_amd import _abi

POISON32, POISON64, POISON_BYTE = C.POISON32, C.POISON64, C.POISON_BYTE
UNIT = 1 << 16
K_OF = ((2, 10), (4, 70), (8, 130), (16, 260), (32, 520))          # a text length inside each variant


def bind(lib):
    return _abi.bind(lib, ["ta_forced_omit_workspace_bytes", "ta_forced_align_omit"])


class _Sizes(object):
    """forced_cases.pack asks its library for the size of a line's workspace piece: the tolerant kernel's here"""

    def __init__(self, lib):
        self.ta_forced_workspace_bytes = lib.ta_forced_omit_workspace_bytes


def pack(lib, lines, no, **kw):
    return C.pack(_Sizes(lib), lines, no, **kw)


def peaked(rng, T, no, shown):
    """posteriors of T frames that show the characters `shown` (blank, c, blank, c ... spread evenly) and nothing else"""
    n = len(shown)
    seq = np.zeros(2 * n + 1, dtype=np.int64)
    seq[1::2] = shown
    frame = seq[(np.arange(T) * len(seq)) // T] if n else np.zeros(T, dtype=np.int64)
    P = rng.random((T, no)).astype(np.float32) * 0.02 + 0.001
    P[np.arange(T), frame] = 0.9
    return (P / P.sum(axis=1, keepdims=True)).astype(np.float32)


def absent(rng, L, no, at, run, slack=5):
    """a text of L characters whose `run` characters from `at` on the page does not show, T = 2 L + 1 + slack.  The run
    is written in the upper half of the classes and the rest in the lower, so no character of the run can pass for one
    the page shows"""
    half = max(1, (no - 1) // 2)
    cs = C.text(rng, L, half + 1)
    cs[at:at + run] = half + C.text(rng, run, no - half)
    shown = np.concatenate([cs[:at], cs[at + run:]])
    return peaked(rng, 2 * L + 1 + slack, no, shown), cs


def cases():
    rng = np.random.default_rng(1409)
    line = lambda T, L, no: (C.probs(rng, T, no), C.text(rng, L, no))                               # noqa: E731
    out = []
    # every variant and each switch of K, at T = S and a walk block and a chunk edge beyond
    for L in (1, 2, 63, 64, 127, 128, 255, 256, 511, 512):
        out.append(("variant L=%d" % L, 6, 3 * UNIT, [line(2 * L + 1, L, 6), line(2 * L + 1 + 37, L, 6)]))
    out.append(("variant L=1023", 6, 3 * UNIT, [line(2047, 1023, 6)]))
    out.append(("chunk and walk block", 5, 2 * UNIT,
                [line(T, L, 5) for T in (3, 8, 9, 31, 32, 33, 64, 65) for L in (1, 2, 3) if 2 * L + 1 <= T]))
    # far moves: an absent run in the middle, inside a lane, over one lane boundary, over many
    out.append(("absent run 1 2", 8, 4 * UNIT, [absent(rng, 12, 8, 5, 1), absent(rng, 12, 8, 5, 2), absent(rng, 12, 8, 4, 2)]))
    for K, L in K_OF:
        runs = [r for r in (K // 2 - 1, K // 2, K // 2 + 1) if r >= 1]
        out.append(("absent run K=%d" % K, 8, 4 * UNIT,
                     [absent(rng, L, 8, L // 2 - r // 2 + d, r) for r in runs for d in (0, 1)]))
    out.append(("absent run 70", 8, 4 * UNIT, [absent(rng, 80, 8, 4, 70)]))
    out.append(("absent run 200", 8, 4 * UNIT, [absent(rng, 210, 8, 6, 200)]))
    out.append(("absent run 600", 8, 4 * UNIT, [absent(rng, 610, 8, 3, 600)]))
    out.append(("absent prefix", 8, 4 * UNIT, [absent(rng, 9, 8, 0, 3), absent(rng, 70, 8, 0, 40), absent(rng, 5, 8, 0, 4)]))
    out.append(("absent suffix", 8, 4 * UNIT, [absent(rng, 9, 8, 6, 3), absent(rng, 70, 8, 30, 40), absent(rng, 5, 8, 1, 4)]))
    aba = np.asarray([1, 2, 1], np.int32)
    out.append(("far between equal labels", 4, 2 * UNIT, [(peaked(rng, T, 4, [1, 1]), aba) for T in (7, 8, 12, 40)]))
    # ties
    out.append(("omit 0 random", 6, 0, [line(9, 3, 6), line(40, 12, 6), line(150, 66, 6), line(300, 130, 6)]))
    const = lambda T, cs, no: (np.full((T, no), 1.0 / no, np.float32), np.asarray(cs, np.int32))    # noqa: E731
    out.append(("omit 0 constant", 4, 0, [const(9, [1, 2, 3], 4), const(8, [1, 1], 4), const(3, [2], 4),
                                          const(70, [1, 2, 2, 3] * 8, 4), const(140, [1, 2, 3] * 22, 4)]))
    out.append(("omit 3 constant", 4, 3 * UNIT, [const(9, [1, 2, 3], 4), const(8, [1, 1], 4), const(140, [1, 2, 3] * 22, 4)]))
    # an omission dearer than any strict path can lose: the strict aligner's answer (T <= 40)
    out.append(("omit 2^26", 6, R.OMIT_MAX, [line(T, L, 6) for T, L in ((3, 1), (7, 3), (12, 2), (40, 19), (33, 9), (40, 5))]))
    out.append(("zeros and NaN", 5, 2 * UNIT, [dict((c[0], c) for c in C.cases())["zeros and NaN"][2][0]]))
    for no in (3, 6, 96, 128):
        out.append(("mixed no=%d" % no, no, 3 * UNIT,
                    [line(2 * L + 1 + d, L, no) for L, d in ((3, 0), (65, 3), (129, 0), (257, 9), (513, 0), (20, 33))] +
                    [absent(rng, 40, no, 10, 12)]))
    return out


STRICT = "omit 2^26"        # the case whose answers must also be forced_ref.align's

_WANT = {}


def want(name, lines, omit):
    """the checker's (frames, score) of a case, computed once"""
    if name not in _WANT:
        _WANT[name] = R.align_batch(lines, omit)
    return _WANT[name]


INPUTS, OUTPUTS = C.INPUTS, C.OUTPUTS
gather = C.gather


def call(lib, pk, ptr, omit, stream=None, **over):
    """ta_forced_align_omit on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to replace"""
    a = dict(nlines=pk.n, no=pk.no, rows=pk.rows, nlabels=pk.nlabels, T_host=pk.T_host.ctypes.data,
             L_host=pk.L_host.ctypes.data, workspace=ptr("ws"), workspace_bytes=pk.ws_bytes, omit_q=omit)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    for name in ("T_host", "L_host"):
        if isinstance(a[name], np.ndarray):
            a[name] = a[name].ctypes.data
    return lib.ta_forced_align_omit(a["probs"], a["row_off"], a["T"], a["labels"], a["lab_off"], a["L"], a["ws_off"],
                                    a["nlines"], a["no"], a["rows"], a["nlabels"], a["T_host"], a["L_host"], a["omit_q"],
                                    a["workspace"], a["workspace_bytes"], a["frames"], a["score"], a["status"], stream)


def refusals(pk):
    """forced_cases.refusals plus omit_q out of range"""
    return C.refusals(pk) + [("omit_q = -1", -1, dict(omit_q=-1)), ("omit_q = 2^26 + 1", -1, dict(omit_q=R.OMIT_MAX + 1))]
