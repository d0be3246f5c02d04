"""The page-scope confidence kernel without a GPU: tests/native/sim_forced_page_conf.cpp compiles
csrc/ta_forced_page_conf.hip ITSELF for the host (a wave = 64 coroutines that meet at every DPP move, ballot and hand-over
of LDS; tests/native/hipshim, sim_forced_shim.h and sim_forced_conf_shim.h, which states the DPP control of the move from
the right lane) and every integer it writes must equal the checker tests/forced_page_conf_ref.py -- the cases of
tests/forced_page_cases.py with the queries of tests/forced_page_conf_cases.py, which tests/test_forced_page_conf_gpu.py
drives through the real kernel."""
import ctypes

import numpy as np
import pytest

import forced_cases as C0
import forced_page_cases as PC
import forced_page_conf_cases as C
import forced_page_conf_ref as R
import forced_page_ref as PR
import simlib


@pytest.fixture(scope="module")
def sim():
    deps = [simlib.NAT + "sim_forced_conf_shim.h", simlib.CSRC + "ta_forced_page_conf.hip",
            simlib.CSRC + "forced_page_two_fill.h", simlib.CSRC + "forced_page_common.h",
            simlib.CSRC + "forced_two_fill.h"] + C0.SIM_DEPS
    return C.bind(simlib.load("forced_page_conf", deps, include=["hipshim"]))


def _run(lib, pk, **over):
    return C.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, **over)


@pytest.mark.parametrize("which", C.SETS)
@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_host_build_of_the_kernel_equals_the_checker(sim, case, which):
    name, no, pages = case
    want = C.want(name, pages)[which]
    pk = C.pack(sim, pages, no, [(w[1], w[2]) for w in want])
    assert _run(sim, pk) == 0
    C.check(pk, want)


def test_workspace_bytes(sim):
    f = sim.ta_forced_page_confidence_workspace_bytes
    # a forward row of 64 K int64 per character: 512 K n bytes
    assert f(1, 2) == 1024 and f(9, 2) == 9216 and f(70, 4) == 2048 * 70 and f(300, 8) == 4096 * 300
    assert f(1027, 32) == 16384 * 1027 and f(5, 16) == 8192 * 5 and f(1 << 29, 32) == 1 << 43
    for n, K in ((0, 2), (-1, 2), ((1 << 29) + 1, 2), (5, 0), (5, 3), (5, 64), (5, -2)):
        assert f(n, K) == -1


def _three(rng):
    return [PC._page(rng, (12, 11), 8, (0, 3), (4, 8), 6), PC._page(rng, (10, 9, 11), 9, (0, 1, 6), (5, 6, 9), 6),
            PC._wide(rng, 70)]


def _wants(rng, pages):
    out = []
    for Ps, cs, lo, hi in pages:
        ql, qt = C.seeded_queries(rng, [len(P) for P in Ps], len(cs), lo, hi)
        out.append((PR.OK, ql, qt) + R.query(Ps, cs, lo, hi, ql, qt) + (None,))
    return out


def test_a_page_without_a_path_between_two_good_ones(sim):
    rng = np.random.default_rng(11)
    pages = _three(rng)
    pages[1] = PC._page(rng, (2, 1), 5, (0, 2), (4, 5), 6)              # five characters on three frames
    want = _wants(rng, [pages[0]]) + [None] + _wants(rng, [pages[2]])
    ql, qt = C.seeded_queries(rng, [2, 1], 5, pages[1][2], pages[1][3])
    want[1] = (PR.NOPATH, ql, qt, None, None, None)
    pk = C.pack(sim, pages, 6, [(w[1], w[2]) for w in want])
    assert _run(sim, pk) == 0
    C.check(pk, want)


def test_a_page_refused_through_its_data_leaves_its_neighbours_alone(sim):
    rng = np.random.default_rng(7)
    pages = _three(rng)
    want = _wants(rng, pages)
    # page 1's lines have 10, 9 and 11 frames and the windows [0, 5), [1, 6), [6, 9); its queries are chosen by hand
    Ps, cs, lo, hi = pages[1]
    ql, qt = np.asarray([0, 0, 0, 0, 0, 1, 2, 2, 2], np.int32), np.asarray([0, 2, 2, 5, 9, 4, 0, 3, 10], np.int32)
    want[1] = (PR.OK, ql, qt) + R.query(Ps, cs, lo, hi, ql, qt) + (None,)
    queries = [(w[1], w[2]) for w in want]

    def refused(status, **edit):
        pk = C.pack(sim, pages, 6, queries)
        for name, (k, v) in edit.items():
            getattr(pk, name)[k] = v
        host = {h: getattr(C.pack(sim, pages, 6, queries), h[:-5]) for h in C.HOST}      # the host's copies stay right
        assert _run(sim, pk, **host) == 0
        w = list(want)
        w[1] = (status,)
        C.check(pk, w)

    a = int(C.pack(sim, pages, 6, queries).lab_off[1])
    refused(PR.LABEL, labels=(a + 2, 6))
    refused(PR.LABEL, labels=(a + 8, 0))
    refused(PR.BOUNDS, lo=(2, 1))                          # lo_0 != 0
    refused(PR.BOUNDS, hi=(4, 8))                          # hi_last != n
    refused(PR.BOUNDS, lo=(3, 6))                          # lo_1 > hi_0: a character no window holds
    refused(PR.BOUNDS, lo=(4, 0))                          # lo_2 < lo_1: not monotone
    refused(PR.BOUNDS, hi=(3, 4))                          # hi_1 < hi_0
    refused(PR.BOUNDS, T=(3, 0))
    refused(PR.BOUNDS, T=(3, 5001))
    refused(PR.BOUNDS, row_off=(2, -3))
    refused(PR.BOUNDS, row_off=(4, 10 ** 9))
    refused(PR.BOUNDS, cws_off=(1, 8))
    refused(PR.BOUNDS, cws_off=(1, 10 ** 12))
    refused(PR.BOUNDS, cws_off=(1, -16))
    # each refusal of a query
    def query(i, k, t):
        return (a + i, [k, -7, -7, t])
    refused(R.QUERY, query=query(0, -1, 0))                # a line outside the page
    refused(R.QUERY, query=query(8, 3, 0))
    refused(R.QUERY, query=query(8, 10 ** 9, 0))
    refused(R.QUERY, query=query(3, 0, -1))                # a frame outside its line
    refused(R.QUERY, query=query(4, 0, 10))
    refused(R.QUERY, query=query(8, 2, 11))
    refused(R.QUERY, query=query(0, 2, 0))                 # character 0 is not in line 2's window [6, 9)
    refused(R.QUERY, query=query(8, 1, 8))                 # character 8 is not in line 1's window [1, 6)
    refused(R.QUERY, query=query(5, 0, 9))                 # ... nor character 5 in line 0's [0, 5)
    refused(R.QUERY, query=query(2, 0, 6))                 # queries that decrease inside a line: character 3 is at (0, 5)
    refused(R.QUERY, query=query(3, 1, 0))                 # ... and from line to line: character 4 is at (0, 9)
    with pytest.raises(ValueError):
        R.query(Ps, cs, lo, hi, np.asarray([0, 0, 0, 1, 0, 1, 2, 2, 2]), qt * 0)
    # the device's windows ask for a variant that the host's copies did not launch: refused, not left without a status
    wide = PC._page(np.random.default_rng(8), (150, 12), 73, (0, 68), (70, 73), 6)
    two = [pages[0], wide]
    w2 = _wants(rng, two)
    pk2 = C.pack(sim, two, 6, [(w[1], w[2]) for w in w2])
    narrow, early = pk2.hi.copy(), pk2.lo.copy()
    narrow[2], early[3] = 60, 58                          # the host's copy says K = 2, the device's 70 characters need K = 4
    assert _run(sim, pk2, hi_host=narrow, lo_host=early) == 0
    C.check(pk2, [w2[0], (PR.BOUNDS,)])
    # equal neighbours are allowed
    same = [(l.copy(), t.copy()) for l, t in queries]
    same[1][0][6:], same[1][1][6:] = 2, 4
    pk = C.pack(sim, pages, 6, same)
    assert _run(sim, pk) == 0
    w = list(want)
    Ps, cs, lo, hi = pages[1]
    w[1] = (PR.OK,) + same[1] + R.query(Ps, cs, lo, hi, *same[1]) + (None,)
    C.check(pk, w)


def test_host_side_refusals_touch_nothing(sim):
    rng = np.random.default_rng(9)
    pages = _three(rng)[:2]
    want = _wants(rng, pages)
    pk = C.pack(sim, pages, 6, [(w[1], w[2]) for w in want])
    EINVAL, ELIMIT = -1, -4

    def arr(name, k, v):
        a = getattr(pk, name).copy()
        a[k] = v
        return a
    wide_hi, wide_lab = pk.hi.copy(), pk.lab_off.copy()
    wide_hi[:2] = 1024                                   # one window of 1024 characters: [0, 1024) on both lines of page 0
    wide_lab[1:] += 1016
    cap_hi, cap_lab = pk.hi.copy(), pk.lab_off.copy()
    cap_hi[1] = (1 << 29) + 1                            # a page of 2^29 + 1 characters behind a narrow first window
    cap_lab[1:] += (1 << 29) + 1 - 8
    need = sum(pk.piece)
    sim.sim_forced_page_conf_last_error.restype = ctypes.c_char_p
    last_error = sim.sim_forced_page_conf_last_error
    # every refusal with its text, word for word: forced_check_pages', with the rule of this call's workspace
    refusals = [
        ("null probs", EINVAL, "null pointer argument", dict(probs=None)), ("null query", EINVAL, "null pointer argument", dict(query=None)),
        ("null rival", EINVAL, "null pointer argument", dict(rival=None)), ("null confidence", EINVAL, "null pointer argument", dict(confidence=None)),
        ("null workspace", EINVAL, "null pointer argument", dict(workspace=None)), ("null lo_host", EINVAL, "null pointer argument", dict(lo_host=None)),
        ("negative npages", EINVAL, "negative size", dict(npages=-1)), ("negative rows", EINVAL, "negative size", dict(rows=-1)),
        ("no = 1", EINVAL, "no outside 2 .. TA_TRAIN_MAX_CLASSES", dict(no=1)), ("no = 129", EINVAL, "no outside 2 .. TA_TRAIN_MAX_CLASSES", dict(no=129)),
        ("rows too few", EINVAL, "the lines' timesteps exceed rows", dict(rows=int(pk.T.sum()) - 1)),
        ("nlabels too few", EINVAL, "the pages' texts exceed nlabels", dict(nlabels=int(pk.lab_off[-1]) - 1)),
        ("workspace too small", EINVAL, "workspace smaller than the pages' ta_forced_page_confidence_workspace_bytes", dict(workspace_bytes=need - 1)),
        ("workspace misaligned", EINVAL, "workspace not 16-byte aligned", dict(workspace=pk.cws.ctypes.data + 4)),
        ("nlines wrong", EINVAL, "line_first does not run from 0 to nlines", dict(nlines=pk.nlines + 1)),
        ("a page without lines", EINVAL, "a page without lines", dict(line_first_host=np.asarray([0, 0, pk.nlines], np.int64))),
        ("a page without text", EINVAL, "a page without text", dict(lab_off_host=arr("lab_off", 1, int(pk.lab_off[0])))),
        ("T = 0", EINVAL, "a line without timesteps", dict(T_host=arr("T", 1, 0))), ("T > 5000", ELIMIT, "a line has more than TA_TRAIN_MAX_T timesteps", dict(T_host=arr("T", 1, 5001))),
        ("lo_0 != 0", EINVAL, "the first window does not start at the text's start", dict(lo_host=arr("lo", 0, 1))), ("hi_last != n", EINVAL, "the last window does not end at the text's end", dict(hi_host=arr("hi", 1, 7))),
        ("non-monotone lo", EINVAL, "windows must move forwards and leave no character out", dict(lo_host=arr("lo", 4, 0))),
        ("a gap between windows", EINVAL, "windows must move forwards and leave no character out", dict(lo_host=arr("lo", 1, 5))),
        ("hi decreases", EINVAL, "windows must move forwards and leave no character out", dict(hi_host=arr("hi", 3, 4))),
        ("width 1024", ELIMIT, "a window of more than TA_FORCED_MAX_TARGET characters", dict(hi_host=wide_hi, lab_off_host=wide_lab, nlabels=10 ** 6)),
        ("2^29 + 1 characters", ELIMIT, "a page's text is too long",
         dict(hi_host=cap_hi, lab_off_host=cap_lab, nlabels=1 << 40)),
        ("lo_0 = -1", EINVAL, "a window outside its page's text", dict(lo_host=arr("lo", 0, -1))),
        ("hi_0 > n", EINVAL, "a window outside its page's text", dict(hi_host=arr("hi", 0, 9))),
        ("hi_0 < lo_0", EINVAL, "a window outside its page's text", dict(hi_host=arr("hi", 0, -1))),
        ("T > 5000 and lo_0 != 0 on one line", ELIMIT, "a line has more than TA_TRAIN_MAX_T timesteps",
         dict(T_host=arr("T", 0, 5001), lo_host=arr("lo", 0, 1))),
        ("nlines wrong and a page without text", EINVAL, "line_first does not run from 0 to nlines",
         dict(nlines=pk.nlines + 1, lab_off_host=arr("lab_off", 1, int(pk.lab_off[0])))),
    ]
    for what, code, text, over in refusals:
        assert _run(sim, pk, **over) == code, what
        assert last_error().decode() == text, what
        assert C.untouched(pk), what
    # more than 2^25 frames on one page: 6 712 lines of 5 000 frames; the host refuses before it looks at anything else
    nl = 6712
    big = dict(nlines=nl, npages=1, rows=1 << 40, T_host=np.full(nl, 5000, np.int32), lo_host=np.zeros(nl, np.int32),
               hi_host=np.full(nl, 8, np.int32), line_first_host=np.asarray([0, nl], np.int64),
               lab_off_host=np.asarray([int(pk.lab_off[0]), int(pk.lab_off[0]) + 8], np.int64))
    assert _run(sim, pk, **big) == ELIMIT and last_error().decode() == "a page has more than 2^25 frames"
    assert C.untouched(pk)
    assert _run(sim, pk, npages=0) == 0 and C.untouched(pk)
    assert _run(sim, pk) == 0
    C.check(pk, want)
