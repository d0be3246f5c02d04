"""The page-scope forced-alignment kernel with omission without a GPU: tests/native/sim_forced_page_omit.cpp compiles
csrc/ta_forced_page_omit.hip ITSELF for the host (a wave = 64 coroutines that meet at every DPP move, ballot and hand-over
of LDS; tests/native/hipshim, sim_forced_shim.h and sim_forced_omit_shim.h) and every integer it writes must equal the
checker tests/forced_page_omit_ref.py -- the cases of tests/forced_page_omit_cases.py, which
tests/test_forced_page_omit_gpu.py drives through the real kernel."""
import ctypes

import numpy as np
import pytest

import forced_cases as C0
import forced_page_cases as PC
import forced_page_omit_cases as C
import forced_page_omit_ref as R
import simlib

UNIT = C.UNIT


@pytest.fixture(scope="module")
def sim():
    deps = [simlib.NAT + "sim_forced_omit_shim.h", simlib.CSRC + "ta_forced_page_omit.hip",
            simlib.CSRC + "forced_page_common.h"] + C0.SIM_DEPS
    return C.bind(simlib.load("forced_page_omit", deps, include=["hipshim"]))


def _run(lib, pk, omit, **over):
    return C.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, omit, **over)


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_host_build_of_the_kernel_equals_the_checker(sim, case):
    name, no, omit, pages = case
    pk = C.pack(sim, pages, no)
    assert _run(sim, pk, omit) == 0
    want = C.want(name, pages, omit)
    assert [w[0] for w in want] == [R.OK] * len(pages)
    C.check(pk, want)
    if name.startswith(C.STRICT):
        C.check(pk, C.strict_want(pages))


def _far_at_break(path, lo):
    """[(line, source state, target state)] of the far moves a path makes on a line's first frame"""
    out = []
    for (k0, t0, s0), (k1, t1, s1) in zip(path[:-1], path[1:]):
        if t1 == 0 and k1 > 0 and s1 // 2 >= 1 and s0 <= 2 * (s1 // 2) - 2 and not (s1 - s0 == 2 and s1 % 2 == 1):
            out.append((k1, s0, s1))
    return out


def test_the_scripted_cases_exercise_what_they_were_written_for():
    """on the checker's own path: the far moves at the line breaks start where the cases say, the absent runs are what
    the path omits, and the path starts above state 1 and ends below 2 n where a prefix or suffix is absent"""
    by = dict((c[0], c) for c in C.cases())
    _, _, omit, (a, b, c) = by["far on a first frame"]
    far = [_far_at_break(R.align_page_omit_closed(*pg, omit)[3], pg[2]) for pg in (a, b, c)]
    # the blank 2 lo_new - 2 can only TIE as a source: being in the blank 2 lo_new a frame earlier costs the same, and
    # the tie order (advance before far, the largest s' among far candidates) takes that -- the page holds the tie
    path = R.align_page_omit_closed(*a, omit)
    assert far[0] == [] and [s for _, _, s in path[3]] == [1, 1, 3, 3, 6, 7, 7, 9, 9] and 4 == 2 * a[2][1] - 2
    rival = [(k, t, 4 if (k, t) == (0, 4) else s) for k, t, s in path[3]]
    assert R.path_score(*a, omit, rival) == path[1]
    assert far[1] == [(1, 3, 11)] and 3 < 2 * b[2][1] - 2            # from a label several states below the window
    assert far[2] == [(1, 17, 43)] and 17 // 4 >= 1 and 17 < 2 * c[2][1]     # from lane 4 of the old layout (K = 4)
    for pg in by["equal characters across a break"][3]:
        st, score, frames, path = R.align_page_omit(*pg, by["equal characters across a break"][2])
        (k, s0, s1), = _far_at_break(path, pg[2])
        lab = pg[1]
        assert lab[s0 // 2] == lab[s1 // 2] and s1 - s0 == 4 and (frames[(s0 + 1) // 2 + 0] == -1).all()
    for K in C.KS:
        name = "absent runs K=%d" % K
        _, _, omit, pages = by[name]
        assert [max(PC.variant(h - l) for l, h in zip(pg[2], pg[3])) for pg in pages] == [K] * 3
        for pg, (st, score, frames) in zip(pages, C.want(name, pages, omit)):
            cs = np.asarray(pg[1])
            assert ((frames[:, 0] == R.OMITTED) == (cs >= 4)).all(), name        # the run and the filler, nothing else
            run = int((cs == 4).sum())
            far = _far_at_break(R.align_page_omit_closed(*pg, omit)[3], pg[2])
            assert [(k, s1 - s0) for k, s0, s1 in far] == ([(1, 2 * run + 2)] if run else []), name
    _, _, omit, pages = by["walk blocks"]
    for pg, T in zip(pages, (31, 32, 33)):
        assert len(pg[0][0]) == T and len(_far_at_break(R.align_page_omit_closed(*pg, omit)[3], pg[2])) == 1
    _, _, omit, pages = by["absent prefix and suffix"]
    for pg in pages:
        path = R.align_page_omit(*pg, omit)[3]
        assert path[0][2] == 15 and path[-1][2] == 19 and 2 * len(pg[1]) == 38
    _, _, omit, pages = by["more characters than frames"]
    assert all(len(pg[1]) > sum(len(P) for P in pg[0]) for pg in pages)
    assert any(name.startswith(C.STRICT) for name in by) and sum(len(c[3]) for n, c in by.items() if n.startswith(C.STRICT)) >= 15


def test_workspace_bytes(sim):
    T = np.asarray([3, 8, 9, 1], np.int32)
    f = lambda nl, K: sim.ta_forced_page_omit_workspace_bytes(nl, T.ctypes.data, K)       # noqa: E731
    # the move rows as ta_forced_page_workspace_bytes counts them, then ceil(T / (32 / K)) bit rows per line
    assert f(4, 2) == 256 * ((1 + 1 + 2 + 1) + (1 + 1 + 1 + 1)) and f(4, 4) == 256 * ((1 + 2 + 3 + 1) + (1 + 1 + 2 + 1))
    assert f(4, 8) == 256 * ((2 + 4 + 5 + 1) + (1 + 2 + 3 + 1)) and f(2, 16) == 256 * ((3 + 8) + (2 + 4))
    assert f(4, 32) == 256 * 3 * 21
    assert f(0, 2) == -1 and f(4, 3) == -1 and f(4, 64) == -1
    g = sim.ta_forced_page_omit_workspace_bytes
    assert g(1, np.asarray([5001], np.int32).ctypes.data, 2) == -1 and g(1, np.asarray([0], np.int32).ctypes.data, 2) == -1
    assert g(1, None, 2) == -1
    assert g(1, np.asarray([5000], np.int32).ctypes.data, 32) == 256 * 3 * 5000


def _three(rng):
    return [C._page(rng, (12, 11), 8, (0, 3), (4, 8), 6), C._page(rng, (4, 3, 5), 14, (0, 1, 8), (6, 9, 14), 6), C._wide(rng, 70)]


def test_a_page_refused_through_its_data_leaves_its_neighbours_alone(sim):
    pages = _three(np.random.default_rng(7))
    omit = 2 * UNIT
    want = [R.answer(*pg, omit) for pg in pages]
    assert [w[0] for w in want] == [R.OK] * 3

    def refused(status, **edit):
        pk = C.pack(sim, pages, 6)
        for name, (k, v) in edit.items():
            getattr(pk, name)[k] = v
        host = {h: getattr(C.pack(sim, pages, 6), h[:-5]) for h in C.HOST}            # the host's copies stay right
        assert _run(sim, pk, omit, **host) == 0
        w = list(want)
        w[1] = (status, None, None)
        C.check(pk, w)

    a = int(C.pack(sim, pages, 6).lab_off[1])
    refused(R.LABEL, labels=(a + 2, 6))
    refused(R.LABEL, labels=(a + 13, 0))
    refused(R.BOUNDS, lo=(2, 1))                          # lo_0 != 0
    refused(R.BOUNDS, hi=(4, 13))                         # hi_last != n
    refused(R.BOUNDS, lo=(3, 7))                          # lo_1 > hi_0: a character no window holds
    refused(R.BOUNDS, lo=(4, 0))                          # lo_2 < lo_1: not monotone
    refused(R.BOUNDS, hi=(3, 5))                          # hi_1 < hi_0
    refused(R.BOUNDS, T=(3, 0))
    refused(R.BOUNDS, T=(3, 5001))
    refused(R.BOUNDS, row_off=(2, -3))
    refused(R.BOUNDS, row_off=(4, 10 ** 9))
    refused(R.BOUNDS, ws_off=(2, 8))
    refused(R.BOUNDS, ws_off=(3, 10 ** 12))
    refused(R.BOUNDS, ws_off=(4, -16))
    # the device's windows ask for a variant that the host's copies did not launch: refused, not left without a status
    wide = C._page(np.random.default_rng(8), (15, 12), 73, (0, 68), (70, 73), 6)
    pk2 = C.pack(sim, [pages[0], wide], 6)
    narrow, early = pk2.hi.copy(), pk2.lo.copy()
    narrow[2], early[3] = 60, 58                          # the host's copy says K = 2, the device's 70 characters need K = 4
    assert _run(sim, pk2, omit, hi_host=narrow, lo_host=early) == 0
    assert pk2.status.tolist() == [R.OK, R.BOUNDS]
    # (the price is a launch argument, not data: no page can be refused through it past the host's check)
    pk = C.pack(sim, pages[:2], 6)
    assert _run(sim, pk, omit) == 0 and pk.status.tolist() == [R.OK, R.OK]


def test_host_side_refusals_touch_nothing(sim):
    pages = _three(np.random.default_rng(9))[:2]
    pk = C.pack(sim, pages, 6)
    omit = 2 * UNIT
    EINVAL, ELIMIT = -1, -4

    def arr(name, k, v):
        a = getattr(pk, name).copy()
        a[k] = v
        return a
    wide_hi, wide_lab = pk.hi.copy(), pk.lab_off.copy()
    wide_hi[:2] = 1024                                   # one window of 1024 characters: [0, 1024) on both lines of page 0
    wide_lab[1:] += 1016
    long_hi, long_lab = pk.hi.copy(), pk.lab_off.copy()
    long_hi[1] = (1 << 20) + 1                           # a page of 2^20 + 1 characters behind a narrow first window
    long_lab[1:] += (1 << 20) + 1 - 8
    # a page of more than 2^25 frames needs 6711 lines of 5000: every line but the first a copy of line 1
    many = 6711
    T_many = np.full(many + 3, 5000, np.int32)
    lf_many = np.asarray([0, many, many + 3], np.int64)
    lo_many = np.concatenate([[0], np.full(many - 1, pk.lo[1]), pk.lo[2:5]]).astype(np.int32)
    hi_many = np.concatenate([[pk.hi[0]], np.full(many - 1, pk.hi[1]), pk.hi[2:5]]).astype(np.int32)
    sim.sim_forced_page_omit_last_error.restype = ctypes.c_char_p
    last_error = sim.sim_forced_page_omit_last_error
    # every refusal with its text, word for word; where an input breaks two rules the text shows which is asked first
    refusals = [
        ("omit -1", EINVAL, "omit_q outside 0 .. TA_FORCED_OMIT_MAX", dict(omit_q=-1)), ("omit above the maximum", EINVAL, "omit_q outside 0 .. TA_FORCED_OMIT_MAX", dict(omit_q=(1 << 26) + 1)),
        ("2^20 + 1 characters", ELIMIT, "a page's text has more than 2^20 characters", dict(hi_host=long_hi, lab_off_host=long_lab, nlabels=1 << 22)),
        ("more than 2^25 frames", ELIMIT, "a page has more than 2^25 frames", dict(T_host=T_many, line_first_host=lf_many, lo_host=lo_many, hi_host=hi_many,
                                               nlines=many + 3, rows=1 << 40, workspace_bytes=1 << 40)),
        ("null probs", EINVAL, "null pointer argument", dict(probs=None)), ("null frames", EINVAL, "null pointer argument", dict(frames=None)),
        ("null workspace", EINVAL, "null pointer argument", dict(workspace=None)), ("null lo_host", EINVAL, "null pointer argument", dict(lo_host=None)),
        ("negative npages", EINVAL, "negative size", dict(npages=-1)), ("negative rows", EINVAL, "negative size", dict(rows=-1)),
        ("no = 1", EINVAL, "no outside 2 .. TA_TRAIN_MAX_CLASSES", dict(no=1)), ("no = 129", EINVAL, "no outside 2 .. TA_TRAIN_MAX_CLASSES", dict(no=129)),
        ("rows too few", EINVAL, "the lines' timesteps exceed rows", dict(rows=int(pk.T.sum()) - 1)),
        ("nlabels too few", EINVAL, "the pages' texts exceed nlabels", dict(nlabels=int(pk.lab_off[-1]) - 1)),
        ("workspace too small", EINVAL, "workspace smaller than the pages' ta_forced_page_omit_workspace_bytes", dict(workspace_bytes=256)),
        ("workspace misaligned", EINVAL, "workspace not 16-byte aligned", dict(workspace=pk.ws.ctypes.data + 4)),
        ("nlines wrong", EINVAL, "line_first does not run from 0 to nlines", dict(nlines=pk.nlines + 1)),
        ("a page without lines", EINVAL, "a page without lines", dict(line_first_host=np.asarray([0, 0, pk.nlines], np.int64))),
        ("a page without text", EINVAL, "a page without text", dict(lab_off_host=arr("lab_off", 1, int(pk.lab_off[0])))),
        ("T = 0", EINVAL, "a line without timesteps", dict(T_host=arr("T", 1, 0))), ("T > 5000", ELIMIT, "a line has more than TA_TRAIN_MAX_T timesteps", dict(T_host=arr("T", 1, 5001))),
        ("lo_0 != 0", EINVAL, "the first window does not start at the text's start", dict(lo_host=arr("lo", 0, 1))), ("hi_last != n", EINVAL, "the last window does not end at the text's end", dict(hi_host=arr("hi", 1, 7))),
        ("non-monotone lo", EINVAL, "windows must move forwards and leave no character out", dict(lo_host=arr("lo", 4, 0))),
        ("a gap between windows", EINVAL, "windows must move forwards and leave no character out", dict(lo_host=arr("lo", 1, 5))),
        ("hi decreases", EINVAL, "windows must move forwards and leave no character out", dict(hi_host=arr("hi", 3, 5))),
        ("width 1024", ELIMIT, "a window of more than TA_FORCED_MAX_TARGET characters", dict(hi_host=wide_hi, lab_off_host=wide_lab, nlabels=10 ** 6)),
        ("lo_0 = -1", EINVAL, "a window outside its page's text", dict(lo_host=arr("lo", 0, -1))),
        ("hi_0 > n", EINVAL, "a window outside its page's text", dict(hi_host=arr("hi", 0, 9))),
        ("hi_0 < lo_0", EINVAL, "a window outside its page's text", dict(hi_host=arr("hi", 0, -1))),
        # the frame cap is asked per page, before the lines are held against rows
        ("more than 2^25 frames and rows too few", ELIMIT, "a page has more than 2^25 frames",
         dict(T_host=T_many, line_first_host=lf_many, lo_host=lo_many, hi_host=hi_many, nlines=many + 3, rows=1,
              workspace_bytes=1 << 40)),
        ("T > 5000 and lo_0 != 0 on one line", ELIMIT, "a line has more than TA_TRAIN_MAX_T timesteps",
         dict(T_host=arr("T", 0, 5001), lo_host=arr("lo", 0, 1))),
    ]
    for what, code, text, over in refusals:
        assert _run(sim, pk, omit, **over) == code, what
        assert last_error().decode() == text, what
        assert (pk.frames == C.POISON32).all() and (pk.score == C.POISON64).all() and (pk.status == C.POISON32).all(), what
        assert (pk.ws == C.POISON_BYTE).all(), what
    assert _run(sim, pk, omit, npages=0) == 0 and (pk.status == C.POISON32).all()
    assert _run(sim, pk, omit) == 0 and pk.status.tolist() == [0, 0]
    C.check(pk, [R.answer(*pg, omit) for pg in pages])
