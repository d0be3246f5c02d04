"""The forced-alignment cases that tests/test_forced_sim.py (the host build of csrc/ta_forced.hip) and
tests/test_forced_gpu.py (the real kernel) share, the layout both drive it with, and the checker's answers, computed once
per process.

A case is (name, no, [(P, cs), ...]).  `pack` lays a case out the way a caller would not: rows and labels with gaps in
front of every line (rows of 0.5, labels of 999 -- a label no line may read), workspace pieces that start at byte 256 and
are 16 bytes apart; `call` runs ta_forced_align on it with every output and the workspace poisoned.
"""
import os

import numpy as np

import forced_ref as R
from text_alignment_amd import _abi

POISON32, POISON64, POISON_BYTE = -0x21212122, -0x2121212121212122, 0xDE
# the largest lattice each variant (K states per lane) takes, as characters, and the smallest of the next: 2 L + 1 <= 64 K
EDGES = [(2, 63, 64), (4, 127, 128), (8, 255, 256), (16, 511, 512), (32, 1023, None)]
WB = R.WALK_BLOCK

# what every host build of a forced-alignment kernel file (tests/native/sim_forced*.cpp) is made of besides its own sources:
# tests/test_forced*_sim.py rebuild their library when one of these is newer
_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DEPS = [os.path.join(_REPO, "tests", "native", "sim_forced_shim.h"),
            os.path.join(_REPO, "tests", "native", "hipshim", "hip", "hip_runtime.h"),
            os.path.join(_REPO, "text_alignment_amd", "csrc", "forced_common.h"),
            os.path.join(_REPO, "text_alignment_amd", "csrc", "forced_two_fill.h"),
            os.path.join(_REPO, "include", "text_alignment_amd.h")]


def bind(lib):
    return _abi.bind(lib, ["ta_forced_workspace_bytes", "ta_forced_align"])


def probs(rng, T, no, sharp=3.0):
    """rows of a softmax over scaled normal draws, float32"""
    z = rng.normal(size=(T, no)) * sharp
    p = np.exp(z - z.max(axis=1, keepdims=True))
    return (p / p.sum(axis=1, keepdims=True)).astype(np.float32)


def text(rng, L, no):
    """L labels in 1 .. no - 1, with repeats next to each other now and then"""
    cs = rng.integers(1, no, size=L)
    rep = rng.random(L) < 0.15
    for i in range(1, L):
        if rep[i]:
            cs[i] = cs[i - 1]
    return cs.astype(np.int32)


def _line(rng, T, L, no):
    return probs(rng, T, no), text(rng, L, no)


def cases():
    rng = np.random.default_rng(1408)
    out = [("L=1 T=3", 4, [_line(rng, 3, 1, 4)])]
    for K, lmax, lnext in EDGES:                      # each variant's edges, at T = S and at T = S + over two walk blocks
        ls = []
        for L in (lmax, lnext):
            if L is not None:
                S = 2 * L + 1
                ls += [_line(rng, S, L, 6), _line(rng, S + 2 * WB + 7, L, 6)]
        out.append(("variant K=%d" % K, 6, ls))
    out.append(("walk block", 5, [_line(rng, T, 3, 5) for T in (WB - 1, WB, WB + 1, 2 * WB - 1, 2 * WB, 2 * WB + 1)] +
                [_line(rng, T, (T - 1) // 2, 5) for T in (WB - 1, WB, WB + 1)]))
    rep = [[2, 2], [2, 2, 3], [2, 2, 2]]
    out.append(("repeats", 4, [(probs(rng, T, 4), np.asarray(cs, np.int32)) for cs in rep
                               for T in (2 * len(cs) + 1, 2 * len(cs) + 1 + len(cs) - 1, 12)]))
    out.append(("no=2", 2, [(probs(rng, 9, 2), np.ones(3, np.int32)), (probs(rng, 3, 2), np.ones(1, np.int32))]))
    out.append(("no=128", 128, [_line(rng, 41, 17, 128), (probs(rng, 20, 128), np.asarray([127, 1, 127], np.int32))]))
    P = probs(rng, 24, 5)
    P[3] = 0.0
    P[4] = np.nan
    P[7, 2] = np.nan
    P[9, :] = [np.inf, -1.0, 0.0, 2.0 ** -17, 2.0 ** -18]
    P[11] = 1.0
    P[12] = [1e-40, 1.5, -np.inf, -0.0, 0.999999]
    out.append(("zeros and NaN", 5, [(P, np.asarray([1, 2, 2, 4, 3], np.int32)),
                                     (np.zeros((7, 5), np.float32), np.asarray([1, 1, 2], np.int32))]))
    out.append(("all ties", 4, [(np.full((9, 4), 0.25, np.float32), np.asarray([1, 2, 3], np.int32)),
                                (np.full((8, 4), 0.25, np.float32), np.asarray([1, 1], np.int32))]))
    out.append(("typical", 40, [_line(rng, T, L, 40) for T, L in ((150, 60), (203, 61), (400, 100), (130, 64))]))
    return out


_WANT = {}


def want(name, lines):
    """the checker's (frames, score) of a case, computed once"""
    if name not in _WANT:
        _WANT[name] = R.align_batch(lines)
    return _WANT[name]


class Packed(object):
    pass


def pack(lib, lines, no, L_dev=None, labels_edit=None):
    """host arrays of one call.  L_dev: {line: value} for the device's copy of L alone; labels_edit: {line: (i, code)}"""
    pk = Packed()
    n = len(lines)
    rows, labs, row_off, lab_off = [], [], [], []
    nr = nl = 0
    for k, (P, cs) in enumerate(lines):
        gap = 1 + k % 3
        rows.append(np.full((gap, no), 0.5, np.float32))
        nr += gap
        row_off.append(nr)
        rows.append(np.asarray(P, np.float32))
        nr += len(P)
        labs.append(np.full(gap + 1, 999, np.int32))
        nl += gap + 1
        lab_off.append(nl)
        cs = np.array(cs, dtype=np.int32)
        if labels_edit and k in labels_edit:
            cs[labels_edit[k][0]] = labels_edit[k][1]
        labs.append(cs)
        nl += len(cs)
    rows.append(np.full((2, no), 0.5, np.float32))
    labs.append(np.full(3, 999, np.int32))
    pk.probs = np.ascontiguousarray(np.concatenate(rows))
    pk.labels = np.concatenate(labs)
    pk.row_off, pk.lab_off = np.asarray(row_off, np.int64), np.asarray(lab_off, np.int64)
    pk.T_host = np.asarray([len(P) for P, _ in lines], np.int32)
    pk.L_host = np.asarray([len(cs) for _, cs in lines], np.int32)
    pk.T, pk.L = pk.T_host.copy(), pk.L_host.copy()
    for k, v in (L_dev or {}).items():
        pk.L[k] = v
    need = [int(lib.ta_forced_workspace_bytes(int(t), int(l))) for t, l in zip(pk.T_host, pk.L_host)]
    assert min(need) > 0
    off, ws_off = 256, []
    for b in need:
        ws_off.append(off)
        off += b + 16
    pk.ws_off, pk.ws_bytes = np.asarray(ws_off, np.int64), off
    pk.n, pk.no, pk.rows, pk.nlabels = n, no, len(pk.probs), len(pk.labels)
    pk.frames = np.full((pk.nlabels, 3), POISON32, np.int32)
    pk.score = np.full(n, POISON64, np.int64)
    pk.status = np.full(n, POISON32, np.int32)
    pk.ws = np.full(pk.ws_bytes, POISON_BYTE, np.uint8)
    return pk


INPUTS = ("probs", "row_off", "T", "labels", "lab_off", "L", "ws_off")
OUTPUTS = ("frames", "score", "status")


def call(lib, pk, ptr, stream=None, **over):
    """ta_forced_align on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to replace"""
    a = dict(nlines=pk.n, no=pk.no, rows=pk.rows, nlabels=pk.nlabels, T_host=pk.T_host.ctypes.data,
             L_host=pk.L_host.ctypes.data, workspace=ptr("ws"), workspace_bytes=pk.ws_bytes)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    for name in ("T_host", "L_host"):
        if isinstance(a[name], np.ndarray):
            a[name] = a[name].ctypes.data
    return lib.ta_forced_align(a["probs"], a["row_off"], a["T"], a["labels"], a["lab_off"], a["L"], a["ws_off"], a["nlines"],
                               a["no"], a["rows"], a["nlabels"], a["T_host"], a["L_host"], a["workspace"],
                               a["workspace_bytes"], a["frames"], a["score"], a["status"], stream)


def gather(pk, frames):
    """the lines' own rows of frames, line after line; everything else must still be poison"""
    own = np.zeros(len(frames), dtype=bool)
    for o, l in zip(pk.lab_off, pk.L_host):
        own[o:o + l] = True
    assert (frames[~own] == POISON32).all(), "a row of frames outside every line was written"
    return frames[own]


def refusals(pk):
    """(what, expected code, arguments to replace) of the host-side refusals; T_host / L_host edits as arrays to keep alive"""
    EINVAL, ELIMIT = -1, -4

    def arr(base, k, v):
        a = base.copy()
        a[k] = v
        return a
    out = [("null probs", EINVAL, dict(probs=None)), ("null frames", EINVAL, dict(frames=None)),
           ("null workspace", EINVAL, dict(workspace=None)), ("null T_host", EINVAL, dict(T_host=None)),
           ("negative nlines", EINVAL, dict(nlines=-1)), ("negative rows", EINVAL, dict(rows=-1)),
           ("no = 1", EINVAL, dict(no=1)), ("no = 129", EINVAL, dict(no=129)),
           ("rows too few", EINVAL, dict(rows=int(pk.T_host.sum()) - 1)),
           ("nlabels too few", EINVAL, dict(nlabels=int(pk.L_host.sum()) - 1)),
           ("workspace too small", EINVAL, dict(workspace_bytes=int(pk.ws_bytes) // 4)),
           ("workspace misaligned", EINVAL, "misalign"),
           ("L = 0", EINVAL, dict(L_host=arr(pk.L_host, 0, 0))),
           ("2 L + 1 > T", EINVAL, dict(L_host=arr(pk.L_host, 1, (int(pk.T_host[1]) + 1) // 2))),
           ("L > 1023", ELIMIT, dict(L_host=arr(pk.L_host, 0, 1024), T_host=arr(pk.T_host, 0, 4000))),
           ("T > 5000", ELIMIT, dict(T_host=arr(pk.T_host, 0, 5001)))]
    return out
