"""The layout tests/test_forced_page_gated_sim.py (the host build) and tests/test_forced_page_gated_gpu.py (the real kernel)
drive ta_forced_align_pages_gated with, on the pages of tests/forced_page_cases.py and the
answers of tests/forced_page_ref.py.

A slot is (page, gate, cap): page = (Ps, cs, lo, hi) as forced_page_cases has them -- for a gated page anything, also
([], [], [], []): no lines and no text; gate: 0 lets the page through; cap: the widest window the host sizes for (None:
min(n, MAX_TARGET), what the pipeline passes).  `pack` lays the slots out as forced_page_cases.pack does: gaps in front of
every line's rows, labels of 999 around the texts, workspace pieces that start at byte 256 and lie 16 bytes apart -- each
sized by its page's CAP -- and every output and the workspace poisoned.
"""
import numpy as np

import forced_page_cases as C
import forced_page_ref as R
from text_alignment_amd import _abi

POISON32, POISON64, POISON_BYTE = C.POISON32, C.POISON64, C.POISON_BYTE
SKIPPED = _abi.CONSTANTS["TA_FORCED_SKIPPED"]
MAX_TARGET = _abi.CONSTANTS["TA_FORCED_MAX_TARGET"]


def bind(lib):
    return _abi.bind(lib, ["ta_forced_page_gated_workspace_bytes", "ta_forced_align_pages_gated"])


def slots(pages, gate=0, cap=None):
    return [(pg, gate, cap) for pg in pages]


def pack(lib, slot_list, no):
    pk = C.Packed()
    rows, labs, row_off, lab_off, T, lo, hi, line_first, gate, cap = [], [np.full(2, 999, np.int32)], [], [2], [], [], [], [0], [], []
    nr, nlab, q = 0, 2, 0
    for (Ps, cs, los, his), g, c in slot_list:
        for P in Ps:
            gap = 1 + q % 3
            rows.append(np.full((gap, no), 0.5, np.float32))
            nr += gap
            row_off.append(nr)
            rows.append(np.asarray(P, np.float32).reshape(-1, no))
            nr += len(P)
            T.append(len(P))
            q += 1
        lo += [int(v) for v in los]
        hi += [int(v) for v in his]
        line_first.append(q)
        labs.append(np.array(cs, dtype=np.int32).reshape(-1))
        nlab += len(cs)
        lab_off.append(nlab)
        gate.append(int(g))
        cap.append(min(len(cs), MAX_TARGET) if c is None else int(c))
    rows.append(np.full((2, no), 0.5, np.float32))
    labs.append(np.full(3, 999, np.int32))
    pk.probs = np.ascontiguousarray(np.concatenate(rows))
    pk.labels = np.concatenate(labs)
    pk.row_off = np.asarray(row_off + [0] * (q == 0), np.int64)
    pad = lambda a: np.asarray(a + [0] * (q == 0), np.int32)                                        # noqa: E731
    pk.T, pk.lo, pk.hi = pad(T), pad(lo), pad(hi)
    pk.line_first, pk.lab_off = np.asarray(line_first, np.int64), np.asarray(lab_off, np.int64)
    pk.gate, pk.cap = np.asarray(gate, np.int32), np.asarray(cap, np.int32)
    off, ws_off, pk.pieces = 256, [], []
    for p in range(len(slot_list)):
        for k in range(line_first[p], line_first[p + 1]):
            one = np.asarray([T[k]], np.int32)
            b = int(lib.ta_forced_page_gated_workspace_bytes(1, one.ctypes.data, int(pk.cap[p])))
            assert b > 0
            ws_off.append(off)
            pk.pieces.append(b)
            off += b + 16
    pk.ws_off, pk.ws_bytes = np.asarray(ws_off + [0] * (q == 0), np.int64), off
    pk.npages, pk.nlines, pk.no, pk.rows, pk.nlabels = len(slot_list), q, no, len(pk.probs), len(pk.labels)
    pk.frames = np.full((pk.nlabels, R.FIELDS), POISON32, np.int32)
    pk.score = np.full(max(pk.npages, 1), POISON64, np.int64)
    pk.status = np.full(max(pk.npages, 1), POISON32, np.int32)
    pk.ws = np.full(pk.ws_bytes, POISON_BYTE, np.uint8)
    return pk


INPUTS = C.INPUTS + ("gate", "cap")
OUTPUTS = C.OUTPUTS
HOST = ("T_host", "line_first_host", "lab_off_host", "cap_host")


def call(lib, pk, ptr, stream=None, **over):
    """ta_forced_align_pages_gated on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to
    replace (host copies as arrays)"""
    a = dict(npages=pk.npages, nlines=pk.nlines, no=pk.no, rows=pk.rows, nlabels=pk.nlabels, T_host=pk.T,
             line_first_host=pk.line_first, lab_off_host=pk.lab_off, cap_host=pk.cap, workspace=ptr("ws"),
             workspace_bytes=pk.ws_bytes)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    keep = []
    for name in HOST:
        if isinstance(a[name], np.ndarray):
            keep.append(np.ascontiguousarray(a[name]))
            a[name] = keep[-1].ctypes.data
    return lib.ta_forced_align_pages_gated(
        a["probs"], a["row_off"], a["T"], a["line_first"], a["lo"], a["hi"], a["labels"], a["lab_off"], a["ws_off"],
        a["gate"], a["cap"], a["npages"], a["nlines"], a["no"], a["rows"], a["nlabels"], a["T_host"], a["line_first_host"],
        a["lab_off_host"], a["cap_host"], a["workspace"], a["workspace_bytes"], a["frames"], a["score"], a["status"], stream)


def want(slot_list):
    """[(status, score, frames)] per slot: SKIPPED for a gated page, else the checker's"""
    return [(SKIPPED, None, None) if g != 0 else R.align_page(*pg)[:3] for pg, g, _ in slot_list]


def check(pk, want_pages):
    """every output against the expected answers (forced_page_cases.check), and not a byte of the workspace pieces of a
    page that was passed over or refused may have been touched"""
    C.check(pk, want_pages)
    for p, (status, _, _) in enumerate(want_pages):
        if status in (R.OK, R.NOPATH):
            continue
        for k in range(int(pk.line_first[p]), int(pk.line_first[p + 1])):
            a = int(pk.ws_off[k])
            assert (pk.ws[a:a + pk.pieces[k]] == POISON_BYTE).all(), (p, k)
