"""ta_forced_align_lines -- forced alignment whose line list lies on the device -- on the cases of tests/forced_cases.py:
the layout that tests/test_forced_lines_sim.py (the host build of csrc/ta_forced.hip) and tests/test_refine_gpu.py (the
real kernel) share.

`pack` takes forced_cases.pack's rows and labels (gaps everywhere, labels of 999 between the lines) and makes a CHUNK of
them: the case's lines are scattered over more chunk lines than there are texts (acc_line is a permutation with holes;
a hole is a chunk line of one timestep that can receive no text, cap 0), packed slot k carries case line k, the caps are
equal to L for even k and larger for odd k where the line's timesteps allow it, the workspace pieces are sized by the
CAPS, start at byte 256 and lie 16 bytes apart.  Every output and the workspace are poisoned.
"""
import numpy as np

import forced_cases as C
import forced_ref as R
from text_alignment_amd import _abi

POISON32, POISON64, POISON_BYTE = C.POISON32, C.POISON64, C.POISON_BYTE


def bind(lib):
    C.bind(lib)
    return _abi.bind(lib, ["ta_forced_align_lines"])


def pack(lib, lines, no, seed=0, holes=3, extra_slots=2, count=None, L_dev=None, labels_edit=None, cap_edit=None):
    """host arrays of one call.  extra_slots: slots behind the filled ones (their acc_line / L / lab_off are poison: the
    kernel may not read through them); count: the device's count[0] if not the number of lines; L_dev: {slot: value} for
    the device's L alone; cap_edit: {slot: cap} for that slot's line, host and device"""
    pk = C.pack(lib, lines, no, L_dev=L_dev, labels_edit=labels_edit)
    rng = np.random.default_rng(seed)
    n = pk.n
    pk.nlines_all = n + holes
    where = np.sort(rng.choice(pk.nlines_all, size=n, replace=False))
    pk.slot_line = where[rng.permutation(n)].astype(np.int32)              # slot k -> its chunk line
    pk.T_all_host = np.ones(pk.nlines_all, np.int32)
    pk.Lcap_host = np.zeros(pk.nlines_all, np.int32)
    pk.row_off_all = np.zeros(pk.nlines_all, np.int64)                      # a hole: the first gap row
    for k, q in enumerate(pk.slot_line):
        T, L = int(pk.T_host[k]), int(pk.L_host[k])
        pk.T_all_host[q], pk.row_off_all[q] = T, pk.row_off[k]
        pk.Lcap_host[q] = L if k % 2 == 0 else min((T - 1) // 2, R.MAX_TARGET, L + 5 + 60 * (k % 4 == 3))
    for k, v in (cap_edit or {}).items():
        pk.Lcap_host[pk.slot_line[k]] = v
    off, ws_off = 256, np.zeros(pk.nlines_all, np.int64)
    for q in range(pk.nlines_all):
        ws_off[q] = off
        if pk.Lcap_host[q] > 0:
            b = int(lib.ta_forced_workspace_bytes(int(pk.T_all_host[q]), int(pk.Lcap_host[q])))
            assert b > 0
            off += b + 16
    pk.ws_off_all, pk.ws_bytes = ws_off, off
    pk.T_all, pk.Lcap = pk.T_all_host.copy(), pk.Lcap_host.copy()
    pk.nslots = n + extra_slots
    pk.acc_line = np.concatenate([pk.slot_line, np.full(extra_slots, 0x7FFFFFF0, np.int32)]).astype(np.int32)
    pk.L = np.concatenate([pk.L, np.full(extra_slots, 5, np.int32)]).astype(np.int32)
    pk.lab_off = np.concatenate([pk.lab_off, np.full(extra_slots, 1 << 40, np.int64)]).astype(np.int64)
    pk.count = np.asarray([n if count is None else count, int(pk.L_host.sum())], np.int64)
    if count is not None and count < 0:
        pk.count[1] = count
    pk.score = np.full(pk.nslots, POISON64, np.int64)
    pk.status = np.full(pk.nslots, POISON32, np.int32)
    pk.ws = np.full(pk.ws_bytes, POISON_BYTE, np.uint8)
    return pk


INPUTS = ("probs", "row_off_all", "T_all", "ws_off_all", "Lcap", "acc_line", "L", "lab_off", "labels", "count")
OUTPUTS = ("frames", "score", "status")


def call(lib, pk, ptr, stream=None, **over):
    """ta_forced_align_lines on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to replace"""
    a = dict(nlines_all=pk.nlines_all, nslots=pk.nslots, no=pk.no, rows=pk.rows, label_cap=pk.nlabels,
             T_all_host=pk.T_all_host, Lcap_host=pk.Lcap_host, workspace=ptr("ws"), workspace_bytes=pk.ws_bytes)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    for name in ("T_all_host", "Lcap_host"):
        if isinstance(a[name], np.ndarray):
            a[name] = a[name].ctypes.data
    return lib.ta_forced_align_lines(*[a[k] for k in INPUTS], a["nlines_all"], a["nslots"], a["no"], a["rows"],
                                     a["label_cap"], a["T_all_host"], a["Lcap_host"], a["workspace"], a["workspace_bytes"],
                                     a["frames"], a["score"], a["status"], stream)


def untouched(pk):
    """not one output word, nor the workspace, was written"""
    return bool((pk.frames == POISON32).all() and (pk.score == POISON64).all() and (pk.status == POISON32).all() and
                (pk.ws == POISON_BYTE).all())


def refusals(pk):
    """(what, expected code, arguments to replace) of the host-side refusals"""
    EINVAL, ELIMIT = -1, -4
    q0, q1 = int(pk.slot_line[0]), int(pk.slot_line[1])

    def arr(base, q, v):
        a = base.copy()
        a[q] = v
        return a
    return [("null probs", EINVAL, dict(probs=None)), ("null count", EINVAL, dict(count=None)),
            ("null Lcap", EINVAL, dict(Lcap=None)), ("null status", EINVAL, dict(status=None)),
            ("null Lcap_host", EINVAL, dict(Lcap_host=None)), ("null workspace", EINVAL, dict(workspace=None)),
            ("negative nslots", EINVAL, dict(nslots=-1)), ("negative label_cap", EINVAL, dict(label_cap=-1)),
            ("more slots than lines", EINVAL, dict(nslots=pk.nlines_all + 1)),
            ("no = 1", EINVAL, dict(no=1)), ("no = 129", EINVAL, dict(no=129)),
            ("rows too few", EINVAL, dict(rows=int(pk.T_all_host.sum()) - 1)),
            ("workspace too small", EINVAL, dict(workspace_bytes=int(pk.ws_bytes) // 4)),
            ("workspace misaligned", EINVAL, "misalign"),
            ("T = 0", EINVAL, dict(T_all_host=arr(pk.T_all_host, q0, 0))),
            ("cap < 0", EINVAL, dict(Lcap_host=arr(pk.Lcap_host, q0, -1))),
            ("2 cap + 1 > T", EINVAL, dict(Lcap_host=arr(pk.Lcap_host, q1, (int(pk.T_all_host[q1]) + 1) // 2))),
            ("cap > 1023", ELIMIT, dict(Lcap_host=arr(pk.Lcap_host, q0, 1024), T_all_host=arr(pk.T_all_host, q0, 4000))),
            ("T > 5000", ELIMIT, dict(T_all_host=arr(pk.T_all_host, q0, 5001)))]
