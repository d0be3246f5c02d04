"""The page-scope forced-alignment kernel without a GPU: tests/native/sim_forced_page.cpp compiles
csrc/ta_forced_page.hip ITSELF for the host (a wave = 64 coroutines that meet at every DPP move, ballot and hand-over of
LDS; tests/native/hipshim and sim_forced_shim.h) and every integer it writes must equal the checker
tests/forced_page_ref.py -- the cases of tests/forced_page_cases.py, which tests/test_forced_page_gpu.py drives through
the real kernel."""
import ctypes

import numpy as np
import pytest

import forced_cases as C0
import forced_page_cases as C
import forced_page_ref as R
import simlib


@pytest.fixture(scope="module")
def sim():
    deps = [simlib.CSRC + "ta_forced_page.hip", simlib.CSRC + "forced_page_common.h"] + C0.SIM_DEPS
    return C.bind(simlib.load("forced_page", deps, include=["hipshim"]))


def _run(lib, pk, **over):
    return C.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, **over)


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_host_build_of_the_kernel_equals_the_checker(sim, case):
    name, no, pages = case
    pk = C.pack(sim, pages, no)
    assert _run(sim, pk) == 0
    C.check(pk, C.want(name, pages))


def test_variant_and_workspace_bytes(sim):
    for w, K in ((0, 2), (63, 2), (64, 4), (127, 4), (128, 8), (255, 8), (256, 16), (511, 16), (512, 32), (1023, 32)):
        assert sim.ta_forced_page_variant(w) == K == C.variant(w)
    assert sim.ta_forced_page_variant(1024) == -1 and sim.ta_forced_page_variant(-1) == -1
    T = np.asarray([3, 8, 9, 1], np.int32)
    f = lambda nl, K: sim.ta_forced_page_workspace_bytes(nl, T.ctypes.data, K)       # noqa: E731
    assert f(4, 2) == 256 * (1 + 1 + 2 + 1) and f(4, 4) == 256 * (1 + 2 + 3 + 1) and f(4, 32) == 256 * 2 * 21
    assert f(2, 16) == 256 * (3 + 8) and f(0, 2) == -1 and f(4, 3) == -1 and f(4, 64) == -1
    assert sim.ta_forced_page_workspace_bytes(1, np.asarray([5001], np.int32).ctypes.data, 2) == -1
    assert sim.ta_forced_page_workspace_bytes(1, np.asarray([0], np.int32).ctypes.data, 2) == -1
    assert sim.ta_forced_page_workspace_bytes(1, None, 2) == -1


def _three(rng):
    return [C._page(rng, (12, 11), 8, (0, 3), (4, 8), 6), C._page(rng, (10, 9, 11), 9, (0, 1, 6), (5, 6, 9), 6),
            C._wide(rng, 70)]


def test_a_page_refused_through_its_data_leaves_its_neighbours_alone(sim):
    pages = _three(np.random.default_rng(7))
    want = [R.align_page(*pg)[:3] for pg in pages]
    assert [w[0] for w in want] == [R.OK] * 3

    def refused(status, **edit):
        pk = C.pack(sim, pages, 6)
        for name, (k, v) in edit.items():
            getattr(pk, name)[k] = v
        host = {h: getattr(C.pack(sim, pages, 6), h[:-5]) for h in C.HOST}            # the host's copies stay right
        assert _run(sim, pk, **host) == 0
        w = list(want)
        w[1] = (status, None, None)
        C.check(pk, w)

    a = int(C.pack(sim, pages, 6).lab_off[1])
    refused(R.LABEL, labels=(a + 2, 6))
    refused(R.LABEL, labels=(a + 8, 0))
    refused(R.BOUNDS, lo=(2, 1))                          # lo_0 != 0
    refused(R.BOUNDS, hi=(4, 8))                          # hi_last != n
    refused(R.BOUNDS, lo=(3, 6))                          # lo_1 > hi_0: a character no window holds
    refused(R.BOUNDS, lo=(4, 0))                          # lo_2 < lo_1: not monotone
    refused(R.BOUNDS, hi=(3, 4))                          # hi_1 < hi_0
    refused(R.BOUNDS, T=(3, 0))
    refused(R.BOUNDS, T=(3, 5001))
    refused(R.BOUNDS, row_off=(2, -3))
    refused(R.BOUNDS, row_off=(4, 10 ** 9))
    refused(R.BOUNDS, ws_off=(2, 8))
    refused(R.BOUNDS, ws_off=(3, 10 ** 12))
    refused(R.BOUNDS, ws_off=(4, -16))
    # the device's windows ask for a variant that the host's copies did not launch: refused, not left without a status
    pk = C.pack(sim, pages[:2], 6)
    wide = C._page(np.random.default_rng(8), (150, 12), 73, (0, 68), (70, 73), 6)
    pk2 = C.pack(sim, [pages[0], wide], 6)
    narrow, early = pk2.hi.copy(), pk2.lo.copy()
    narrow[2], early[3] = 60, 58                          # the host's copy says K = 2, the device's 70 characters need K = 4
    assert _run(sim, pk2, hi_host=narrow, lo_host=early) == 0
    assert pk2.status.tolist() == [R.OK, R.BOUNDS]
    assert _run(sim, pk) == 0 and pk.status.tolist() == [R.OK, R.OK]


def test_host_side_refusals_touch_nothing(sim):
    pages = _three(np.random.default_rng(9))[:2]
    pk = C.pack(sim, pages, 6)
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
    sim.sim_forced_page_last_error.restype = ctypes.c_char_p
    last_error = sim.sim_forced_page_last_error
    # every refusal with its text, word for word; where an input breaks two rules the text shows which is asked first
    refusals = [
        ("null probs", EINVAL, "null pointer argument", dict(probs=None)), ("null frames", EINVAL, "null pointer argument", dict(frames=None)),
        ("null workspace", EINVAL, "null pointer argument", dict(workspace=None)), ("null lo_host", EINVAL, "null pointer argument", dict(lo_host=None)),
        ("negative npages", EINVAL, "negative size", dict(npages=-1)), ("negative rows", EINVAL, "negative size", dict(rows=-1)),
        ("no = 1", EINVAL, "no outside 2 .. TA_TRAIN_MAX_CLASSES", dict(no=1)), ("no = 129", EINVAL, "no outside 2 .. TA_TRAIN_MAX_CLASSES", dict(no=129)),
        ("rows too few", EINVAL, "the lines' timesteps exceed rows", dict(rows=int(pk.T.sum()) - 1)),
        ("nlabels too few", EINVAL, "the pages' texts exceed nlabels", dict(nlabels=int(pk.lab_off[-1]) - 1)),
        ("workspace too small", EINVAL, "workspace smaller than the pages' ta_forced_page_workspace_bytes", dict(workspace_bytes=256)),
        ("workspace misaligned", EINVAL, "workspace not 16-byte aligned", dict(workspace=pk.ws.ctypes.data + 4)),
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
        assert (pk.frames == C.POISON32).all() and (pk.score == C.POISON64).all() and (pk.status == C.POISON32).all(), what
        assert (pk.ws == C.POISON_BYTE).all(), what
    assert _run(sim, pk, npages=0) == 0 and (pk.status == C.POISON32).all()
    assert _run(sim, pk) == 0 and pk.status.tolist() == [0, 0]
    C.check(pk, [R.align_page(*pg)[:3] for pg in pages])
