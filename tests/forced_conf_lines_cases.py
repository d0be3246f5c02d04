"""ta_forced_confidence_lines -- the confidence whose line list lies on the device -- on the lines of
tests/forced_conf_cases.py: the layout that tests/test_forced_conf_lines_sim.py (the host build of
csrc/ta_forced_conf.hip) and tests/test_forced_conf_lines_gpu.py (the real kernel) share.

`pack` is forced_lines_cases.pack (a scattered CHUNK with holes, caps equal to L and larger, two slots behind count[0]
whose arrays are poison) plus what the aligner leaves behind it: align_status per slot and frames -- the checker's own
(tests/forced_ref.py), all three fields, so the queries are the t_peak column and nothing else.  The workspace is
ta_forced_confidence_lines_workspace_bytes(label_cap, largest cap) plus a tail; it and every output are poisoned.
"""
import numpy as np

import forced_cases as C0
import forced_conf_cases as CC
import forced_lines_cases as LC
import forced_ref as R0
from text_alignment_amd import _abi

POISON32, POISON64, POISON_BYTE = C0.POISON32, C0.POISON64, C0.POISON_BYTE
SKIPPED = 5
TAIL = 64


def bind(lib):
    return _abi.bind(lib, ["ta_forced_confidence_lines_workspace_bytes", "ta_forced_confidence_lines"])


class _Sizes(object):
    """forced_lines_cases.pack sizes the ALIGNER's workspace pieces, which this call does not have"""

    @staticmethod
    def ta_forced_workspace_bytes(T, L):
        return 16


def variant(L):
    return [K for K, lmax, _ in C0.EDGES if L <= lmax][0]


def pack(lib, lines, no, frames=None, align_status=None, **edits):
    """host arrays of one call.  frames: the aligner's rows of the lines one after the other (default: the checker's);
    align_status: {slot: status}; edits: forced_lines_cases.pack's"""
    pk = LC.pack(_Sizes, lines, no, **edits)
    if frames is None:
        frames = R0.align_batch(lines)[0]
    at = 0
    for o, l in zip(pk.lab_off, pk.L_host):
        pk.frames[o:o + l] = frames[at:at + l]
        at += l
    pk.align_status = np.concatenate([np.zeros(pk.n, np.int32), np.full(pk.nslots - pk.n, POISON32, np.int32)])
    for k, v in (align_status or {}).items():
        pk.align_status[k] = v
    pk.kmax = variant(int(pk.Lcap_host.max())) if pk.Lcap_host.max() > 0 else 0
    need = int(lib.ta_forced_confidence_lines_workspace_bytes(pk.nlabels, int(pk.Lcap_host.max())))
    assert need == 512 * pk.kmax * pk.nlabels
    pk.ws_bytes = need + TAIL
    pk.ws = np.full(pk.ws_bytes, POISON_BYTE, np.uint8)
    pk.confidence = np.full(pk.nlabels, POISON64, np.int64)
    pk.rival = np.full(pk.nlabels, POISON32, np.int32)
    del pk.score, pk.ws_off_all
    return pk


INPUTS = ("probs", "row_off_all", "T_all", "Lcap", "acc_line", "L", "lab_off", "labels", "count", "align_status", "frames")
OUTPUTS = ("confidence", "rival", "status")


def call(lib, pk, ptr, stream=None, **over):
    """ta_forced_confidence_lines on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to replace"""
    a = dict(nlines_all=pk.nlines_all, nslots=pk.nslots, no=pk.no, rows=pk.rows, label_cap=pk.nlabels,
             T_all_host=pk.T_all_host, Lcap_host=pk.Lcap_host, workspace=ptr("ws"), workspace_bytes=pk.ws_bytes)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    for name in ("T_all_host", "Lcap_host"):
        if isinstance(a[name], np.ndarray):
            a[name] = a[name].ctypes.data
    return lib.ta_forced_confidence_lines(*[a[k] for k in INPUTS], a["nlines_all"], a["nslots"], a["no"], a["rows"],
                                          a["label_cap"], a["T_all_host"], a["Lcap_host"], a["workspace"],
                                          a["workspace_bytes"], a["confidence"], a["rival"], a["status"], stream)


def untouched(pk, ws=None, **outs):
    """not one output word, nor the workspace, was written (outs: the arrays to look at in place of pk's)"""
    get = lambda name: outs.get(name, getattr(pk, name))                                            # noqa: E731
    return bool((get("confidence") == POISON64).all() and (get("rival") == POISON32).all() and
                (get("status") == POISON32).all() and ((pk.ws if ws is None else ws) == POISON_BYTE).all())


def outside_pieces(pk, ws, slots):
    """the workspace bytes outside the pieces of `slots`: slot k's piece is 512 kmax lab_off[k] .. + 512 K(L[k]) L[k]"""
    piece = np.zeros(pk.ws_bytes, dtype=bool)
    for k in slots:
        a, l = 512 * pk.kmax * int(pk.lab_off[k]), int(pk.L_host[k])
        piece[a:a + 512 * variant(l) * l] = True
    return ws[~piece]


def refusals(pk):
    """forced_lines_cases.refusals (the aligner's, from the host's copies alone) and this call's own pointers"""
    return LC.refusals(pk) + [("null align_status", -1, dict(align_status=None)), ("null frames", -1, dict(frames=None)),
                              ("null rival", -1, dict(rival=None)), ("null confidence", -1, dict(confidence=None)),
                              ("workspace one byte short", -1, dict(workspace_bytes=pk.ws_bytes - TAIL - 1))]


def check_case(pk, name, lines, confidence, rival, status, ws):
    """a good call on a case's lines: every slot OK, the rows equal to the checker at the aligner's own peaks, everything
    outside the slots' rows and pieces still poison"""
    n = len(lines)
    _, conf, riv = CC.want(name, lines)["peak"]
    assert status[:n].tolist() == [R0.OK] * n and (status[n:] == POISON32).all()
    assert np.array_equal(CC.gather(pk, confidence, POISON64), conf)
    assert np.array_equal(CC.gather(pk, rival, POISON32), riv)
    assert (outside_pieces(pk, ws, range(n)) == POISON_BYTE).all()
