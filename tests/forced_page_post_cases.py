"""What tests/test_forced_page_post_sim.py (the host build of csrc/ta_forced_page_post.hip) and
tests/test_forced_page_post_gpu.py (the real kernel) share: the cases -- tests/forced_page_cases.cases(), imported and not
edited --, the two query sets of tests/forced_page_conf_cases.py ("peak": the aligner's own (line, t_peak); "seeded": never
decreasing, equal neighbours, a later line than needed, a line's frame 0 and last frame), the layout both drive the kernel
with, and the checker's answers, computed once per process.

`pack` is forced_page_cases.pack (rows and labels with gaps, the aligner's own workspace and outputs) plus the query rows
(fields 1 and 2, which the kernel does not read, and every row outside the pages' texts hold -7), a workspace piece per
page (the first at byte 512, 16 bytes apart) and the poisoned outputs.  A page's answer is a dict: status, line, frame and,
for a page with a path, forced_page_post_ref.query's seven outputs.
"""
import numpy as np

import forced_page_cases as C
import forced_page_conf_cases as CC
import forced_page_post_ref as R
import forced_page_ref as PR
from text_alignment_amd import _abi

POISON32, POISON64, POISON_BYTE = C.POISON32, C.POISON64, C.POISON_BYTE
SETS = CC.SETS
FIELDS = PR.FIELDS
cases = C.cases
seeded_queries = CC.seeded_queries
PER_LABEL, PER_PAGE = R.PER_LABEL, R.PER_PAGE


def bind(lib):
    return _abi.bind(lib, ["ta_forced_page_posterior_workspace_bytes", "ta_forced_page_posterior"])


def answer(page, ql, qt):
    """the checker's answer for one page and its queries"""
    out = R.query(*page, ql, qt)
    out.update(line=np.asarray(ql, np.int32), frame=np.asarray(qt, np.int32))
    return out


_WANT = {}


def want(name, pages):
    """{set: [answer]} of a case from the checker, the tables of a page computed once; a page without a path has no peaks
    and takes its seeded queries in both sets"""
    if name not in _WANT:
        rng = np.random.default_rng(sum(name.encode()) + 1415)
        aligned = C.want(name, pages)
        got = {w: [] for w in SETS}
        for (Ps, cs, lo, hi), (status, _, frames) in zip(pages, aligned):
            seeded = seeded_queries(rng, [len(P) for P in Ps], len(cs), lo, hi)
            gm, gx, z_m, z_x = R.tables(Ps, cs, lo, hi)
            assert (z_m == 0) == (status == PR.NOPATH), "Z = 0 iff the aligner finds no path"
            sets = dict(peak=seeded if status != PR.OK else (frames[:, 0].copy(), frames[:, 3].copy()), seeded=seeded)
            for w in SETS:
                ql, qt = sets[w]
                one = dict(status=PR.NOPATH if z_m == 0 else PR.OK, line=np.asarray(ql, np.int32), frame=np.asarray(qt, np.int32))
                if z_m != 0:
                    one.update(zip(PER_LABEL, R.query_tables(gm, gx, lo, hi, ql, qt)))
                    one.update(z_m=z_m, z_x=z_x)
                got[w].append(one)
        _WANT[name] = got
    return _WANT[name]


def refused(status):
    return dict(status=status)


def pack(lib, pages, no, queries, aligner=None):
    """host arrays of one call; queries: per page (line, frame); aligner: the library forced_page_cases.pack sizes the
    aligner's workspace with (the real one; by default forced_page_conf_cases' restatement of the header's rule)"""
    pk = C.pack(aligner or CC.AlignerSizes, pages, no)
    pk.query = np.full((pk.nlabels, FIELDS), -7, np.int32)
    for p, (ql, qt) in enumerate(queries):
        a = int(pk.lab_off[p])
        pk.query[a:a + len(ql), 0] = ql
        pk.query[a:a + len(qt), 3] = qt
    off, pws_off = 512, []
    pk.piece = []
    for p, pg in enumerate(pages):
        need = int(lib.ta_forced_page_posterior_workspace_bytes(len(pg[1]), pk.K[p]))
        assert need == 768 * pk.K[p] * len(pg[1])
        pws_off.append(off)
        pk.piece.append(need)
        off += need + 16
    pk.pws_off, pk.pws_bytes = np.asarray(pws_off, np.int64), off
    pk.pws = np.full(pk.pws_bytes, POISON_BYTE, np.uint8)
    for name in PER_LABEL:
        setattr(pk, name, _poison(pk.nlabels, R.DTYPES[name]))
    for name in PER_PAGE:
        setattr(pk, name, _poison(pk.npages, R.DTYPES[name]))
    pk.pstatus = np.full(pk.npages, POISON32, np.int32)
    return pk


def _poison(count, dtype):
    return np.full(count * np.dtype(dtype).itemsize, POISON_BYTE, np.uint8).view(dtype)


def _is_poison(a):
    return (np.ascontiguousarray(a).view(np.uint8) == POISON_BYTE).all()


INPUTS = ("probs", "row_off", "T", "line_first", "lo", "hi", "labels", "lab_off", "pws_off", "query")
OUTPUTS = PER_LABEL + PER_PAGE + ("pstatus",)
HOST = C.HOST


def call(lib, pk, ptr, stream=None, **over):
    """ta_forced_page_posterior on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to replace
    (host copies as arrays)"""
    a = dict(npages=pk.npages, nlines=pk.nlines, no=pk.no, rows=pk.rows, nlabels=pk.nlabels, T_host=pk.T,
             line_first_host=pk.line_first, lo_host=pk.lo, hi_host=pk.hi, lab_off_host=pk.lab_off,
             workspace=ptr("pws"), workspace_bytes=pk.pws_bytes)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    keep = []
    for name in HOST:
        if isinstance(a[name], np.ndarray):
            keep.append(np.ascontiguousarray(a[name]))
            a[name] = keep[-1].ctypes.data
    return lib.ta_forced_page_posterior(
        a["probs"], a["row_off"], a["T"], a["line_first"], a["lo"], a["hi"], a["labels"], a["lab_off"], a["pws_off"],
        a["query"], a["npages"], a["nlines"], a["no"], a["rows"], a["nlabels"], a["T_host"], a["line_first_host"],
        a["lo_host"], a["hi_host"], a["lab_off_host"], a["workspace"], a["workspace_bytes"], a["own_m"], a["own_x"],
        a["rival_m"], a["rival_x"], a["rival_state"], a["z_m"], a["z_x"], a["pstatus"], stream)


def untouched(pk):
    return all(_is_poison(getattr(pk, name)) for name in OUTPUTS + ("pws",))


def _same(got, want_):
    got, want_ = np.ascontiguousarray(got), np.ascontiguousarray(want_, dtype=got.dtype)
    return got.shape == want_.shape and got.tobytes() == want_.tobytes()


def check(pk, want_pages):
    """every output word of a call against the answers per page, bit for bit.  The rows of a page that is not OK, its
    z_m / z_x, every row outside the pages' texts and the workspace outside the pieces of the pages that ran a fill (OK
    and NOPATH) must still be poison."""
    own = np.zeros(pk.nlabels, dtype=bool)
    ran = np.zeros(pk.npages, dtype=bool)
    piece = np.zeros(pk.pws_bytes, dtype=bool)
    for p, w in enumerate(want_pages):
        assert int(pk.pstatus[p]) == w["status"], (p, int(pk.pstatus[p]), w["status"])
        a, o = int(pk.lab_off[p]), int(pk.pws_off[p])
        if w["status"] in (PR.OK, PR.NOPATH):
            piece[o:o + pk.piece[p]] = True
        if w["status"] == PR.OK:
            n = len(w["own_m"])
            for name in PER_LABEL:
                assert _same(getattr(pk, name)[a:a + n], w[name]), (p, name)
            for name in PER_PAGE:
                assert _same(getattr(pk, name)[p:p + 1], [w[name]]), (p, name, getattr(pk, name)[p], w[name])
            own[a:a + n] = True
            ran[p] = True
    for name in PER_LABEL:
        assert _is_poison(getattr(pk, name)[~own]), "a row outside every accepted page was written: " + name
    for name in PER_PAGE:
        assert _is_poison(getattr(pk, name)[~ran]), "a page without values had its %s written" % name
    assert (pk.pws[~piece] == POISON_BYTE).all(), "the workspace outside the pages' rows was written"
