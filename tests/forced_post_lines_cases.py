"""ta_forced_posterior_lines -- the posteriors whose line list lies on the device -- on the lines of
tests/forced_conf_cases.py: the layout that tests/test_forced_post_lines_sim.py (the host build of
csrc/ta_forced_post.hip) and tests/test_forced_post_lines_gpu.py (the real kernel) share.

`pack` is forced_lines_cases.pack (a scattered CHUNK with holes, caps equal to L and larger, two slots behind count[0]
whose arrays are poison) plus what the aligner leaves behind it: align_status per slot and frames -- the checker's own
(tests/forced_ref.py), all three fields, so the queries are the t_peak column and nothing else.  The workspace is
ta_forced_posterior_lines_workspace_bytes(label_cap, largest cap) plus a tail; it and every output are poisoned, the
float64 outputs with the poison's bit pattern (they are compared through their int64 view).  z_m, z_x and status are PER
SLOT.
"""
import numpy as np

import forced_cases as C0
import forced_conf_lines_cases as CL
import forced_lines_cases as LC
import forced_post_cases as PC
import forced_post_ref as R
import forced_ref as R0
from text_alignment_amd import _abi

POISON32, POISON64, POISON_BYTE = C0.POISON32, C0.POISON64, C0.POISON_BYTE
SKIPPED = 5
TAIL = 64
PER_LABEL, PER_LINE = R.PER_LABEL, R.PER_LINE
variant, words, poison_of = CL.variant, PC.words, PC.poison_of


def bind(lib):
    return _abi.bind(lib, ["ta_forced_posterior_lines_workspace_bytes", "ta_forced_posterior_lines"])


def _poison(n, dtype):
    if dtype == np.float64:
        return np.full(n, POISON64, np.int64).view(np.float64)
    return np.full(n, POISON32, np.int32)


def pack(lib, lines, no, frames=None, align_status=None, **edits):
    """host arrays of one call.  frames: the aligner's rows of the lines one after the other (default: the checker's);
    align_status: {slot: status}; edits: forced_lines_cases.pack's"""
    pk = LC.pack(CL._Sizes, lines, no, **edits)
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
    need = int(lib.ta_forced_posterior_lines_workspace_bytes(pk.nlabels, int(pk.Lcap_host.max())))
    assert need == 768 * pk.kmax * pk.nlabels
    pk.ws_bytes = need + TAIL
    pk.ws = np.full(pk.ws_bytes, POISON_BYTE, np.uint8)
    for name in PER_LABEL:
        setattr(pk, name, _poison(pk.nlabels, R.DTYPES[name]))
    for name in PER_LINE:
        setattr(pk, name, _poison(pk.nslots, R.DTYPES[name]))
    del pk.score, pk.ws_off_all
    return pk


INPUTS = CL.INPUTS
OUTPUTS = PER_LABEL + PER_LINE + ("status",)


def call(lib, pk, ptr, stream=None, **over):
    """ta_forced_posterior_lines on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to replace"""
    a = dict(nlines_all=pk.nlines_all, nslots=pk.nslots, no=pk.no, rows=pk.rows, label_cap=pk.nlabels,
             T_all_host=pk.T_all_host, Lcap_host=pk.Lcap_host, workspace=ptr("ws"), workspace_bytes=pk.ws_bytes)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    for name in ("T_all_host", "Lcap_host"):
        if isinstance(a[name], np.ndarray):
            a[name] = a[name].ctypes.data
    return lib.ta_forced_posterior_lines(*[a[k] for k in INPUTS], a["nlines_all"], a["nslots"], a["no"], a["rows"],
                                         a["label_cap"], a["T_all_host"], a["Lcap_host"], a["workspace"],
                                         a["workspace_bytes"], *[a[k] for k in OUTPUTS], stream)


def untouched(pk, got=None):
    """not one output word, nor the workspace, was written (got: name -> the array to look at in place of pk's)"""
    got = got or (lambda name: getattr(pk, name))
    return bool(all((words(got(name)) == poison_of(got(name))).all() for name in OUTPUTS) and
                (got("ws") == POISON_BYTE).all())


def outside_pieces(pk, ws, slots):
    """the workspace bytes outside the pieces of `slots`: slot k's piece is 768 kmax lab_off[k] .. + 768 K(L[k]) L[k]"""
    piece = np.zeros(pk.ws_bytes, dtype=bool)
    for k in slots:
        a, l = 768 * pk.kmax * int(pk.lab_off[k]), int(pk.L_host[k])
        piece[a:a + 768 * variant(l) * l] = True
    return ws[~piece]


def refusals(pk):
    """forced_lines_cases.refusals (the aligner's, from the host's copies alone) and this call's own pointers"""
    return LC.refusals(pk) + [("null align_status", -1, dict(align_status=None)), ("null frames", -1, dict(frames=None)),
                              ("workspace one byte short", -1, dict(workspace_bytes=pk.ws_bytes - TAIL - 1))] + \
        [("null " + name, -1, {name: None}) for name in OUTPUTS if name != "status"]


def answer(lines, frames):
    """the checker's seven outputs for the lines queried at the t_peak column of `frames`"""
    off = np.cumsum([0] + [len(cs) for _, cs in lines])
    return R.query_batch(lines, [frames[a:b, 2] for a, b in zip(off[:-1], off[1:])])


def check_slots(pk, got, wanted, ok, nlines):
    """the slots `ok` (of the nlines the case has) hold the checker's words, every other row of the per-label outputs and
    every other slot's z is still poison"""
    off = np.cumsum([0] + [int(l) for l in pk.L_host])
    keep = np.zeros(int(off[-1]), dtype=bool)
    for k in ok:
        keep[off[k]:off[k + 1]] = True
    for name in PER_LABEL:
        mine = PC.gather(pk, got(name))
        assert np.array_equal(mine[keep], words(wanted[name])[keep]), name
        assert (mine[~keep] == poison_of(mine)).all(), name
    for name in PER_LINE:
        mine = words(got(name))
        ok = list(ok)
        assert np.array_equal(mine[ok], words(wanted[name])[ok]), name
        rest = np.ones(len(mine), dtype=bool)
        rest[ok] = False
        assert (mine[rest] == poison_of(mine)).all(), name


def check_case(pk, name, lines, got):
    """a good call on a case's lines: every slot OK, every word equal to the checker at the aligner's own peaks, everything
    outside the slots' rows and pieces still poison"""
    n = len(lines)
    _, wanted = PC.want(name, lines)["peak"]
    status = got("status")
    assert status[:n].tolist() == [R0.OK] * n and (status[n:] == POISON32).all()
    check_slots(pk, got, wanted, range(n), n)
    assert (outside_pieces(pk, got("ws"), range(n)) == POISON_BYTE).all()
