"""The posterior cases that tests/test_forced_post_sim.py (the host build of csrc/ta_forced_post.hip) and
tests/test_forced_post_gpu.py (the real kernel) share, the layout both drive it with, and the checker's answers, computed
once per process.

The lines and the two query sets ("peak": the aligner's own t_peak; "seeded": frames that never decrease, with equal
neighbours, 0 and T - 1) are tests/forced_conf_cases.py's.  `pack` is forced_cases.pack with the queries (gaps of -7
between the lines) and the eight outputs poisoned; the float64 outputs carry the poison's bit pattern and are compared
through their int64 view.
"""
import numpy as np

import forced_cases as C0
import forced_conf_cases as C1
import forced_post_ref as R
from text_alignment_amd import _abi

POISON32, POISON64, POISON_BYTE = C0.POISON32, C0.POISON64, C0.POISON_BYTE
SETS = C1.SETS
cases, seeded_queries = C1.cases, C1.seeded_queries
PER_LABEL, PER_LINE = R.PER_LABEL, R.PER_LINE


def bind(lib):
    return _abi.bind(lib, ["ta_forced_posterior_workspace_bytes", "ta_forced_posterior"])


_WANT = {}


def want(name, lines):
    """{set: (queries per line, the checker's seven outputs)} of a case, the fills of a line run once for both sets"""
    if name not in _WANT:
        qs = {w: C1.queries(name, lines, w) for w in SETS}
        got = {w: [] for w in SETS}
        for k, (P, cs) in enumerate(lines):
            L = len(cs)
            gm, gx, zm, zx = R.tables(P, cs, np.concatenate([qs[w][k] for w in SETS]))
            for n, w in enumerate(SETS):
                one = dict(zip(PER_LABEL, R.query_tables(gm, gx, np.arange(n * L, (n + 1) * L))))
                one.update(z_m=zm, z_x=zx)
                got[w].append(one)
        _WANT[name] = {w: (qs[w], _join(got[w])) for w in SETS}
    return _WANT[name]


def _join(got):
    out = {k: np.concatenate([g[k] for g in got]).astype(R.DTYPES[k]) for k in PER_LABEL}
    out.update({k: np.asarray([g[k] for g in got], dtype=R.DTYPES[k]) for k in PER_LINE})
    return out


class _Sizes(object):
    """forced_cases.pack asks its library for the workspace pieces under the aligner's name"""

    def __init__(self, lib):
        self.ta_forced_workspace_bytes = lib.ta_forced_posterior_workspace_bytes


def _poison(n, dtype):
    if dtype == np.float64:
        return np.full(n, POISON64, np.int64).view(np.float64)
    return np.full(n, POISON32, np.int32)


def pack(lib, lines, no, tqs, **edits):
    """forced_cases.pack (rows, labels and workspace pieces with gaps) plus the queries and the poisoned outputs"""
    pk = C0.pack(_Sizes(lib), lines, no, **edits)
    pk.t_query = np.full(pk.nlabels, -7, np.int32)
    for o, tq in zip(pk.lab_off, tqs):
        pk.t_query[o:o + len(tq)] = tq
    for name in PER_LABEL:
        setattr(pk, name, _poison(pk.nlabels, R.DTYPES[name]))
    for name in PER_LINE:
        setattr(pk, name, _poison(pk.n, R.DTYPES[name]))
    del pk.frames, pk.score
    return pk


INPUTS = C0.INPUTS + ("t_query",)
OUTPUTS = PER_LABEL + PER_LINE + ("status",)


def call(lib, pk, ptr, stream=None, **over):
    """ta_forced_posterior on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to replace
    (forced_cases.refusals' `frames` stands for the first output here)"""
    a = dict(nlines=pk.n, no=pk.no, rows=pk.rows, nlabels=pk.nlabels, T_host=pk.T_host.ctypes.data,
             L_host=pk.L_host.ctypes.data, workspace=ptr("ws"), workspace_bytes=pk.ws_bytes)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    if "frames" in over:
        over = dict(over)
        over["own_m"] = over.pop("frames")
    a.update(over)
    for name in ("T_host", "L_host"):
        if isinstance(a[name], np.ndarray):
            a[name] = a[name].ctypes.data
    return lib.ta_forced_posterior(a["probs"], a["row_off"], a["T"], a["labels"], a["lab_off"], a["L"], a["ws_off"],
                                   a["t_query"], a["nlines"], a["no"], a["rows"], a["nlabels"], a["T_host"], a["L_host"],
                                   a["workspace"], a["workspace_bytes"], a["own_m"], a["own_x"], a["rival_m"], a["rival_x"],
                                   a["rival_state"], a["z_m"], a["z_x"], a["status"], stream)


def words(a):
    """an output as integers: a float64 array through its int64 view"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def poison_of(a):
    return POISON64 if a.dtype.itemsize == 8 else POISON32


def gather(pk, out):
    """the lines' own rows of a per-label output as integer words, line after line; everything else must still be poison"""
    out = words(out)
    own = np.zeros(len(out), dtype=bool)
    for o, l in zip(pk.lab_off, pk.L_host):
        own[o:o + l] = True
    assert (out[~own] == poison_of(out)).all(), "a row outside every line was written"
    return out[own]


def differing(pk, got, wanted):
    """the names of the outputs (`got`: name -> array as laid out by pack) of which a word differs from the checker's"""
    return ([name for name in PER_LABEL if not np.array_equal(gather(pk, got(name)), words(wanted[name]))] +
            [name for name in PER_LINE if not np.array_equal(words(got(name)), words(wanted[name]))])


def untouched(got):
    return all((words(got(name)) == poison_of(got(name))).all() for name in OUTPUTS) and (got("ws") == POISON_BYTE).all()
