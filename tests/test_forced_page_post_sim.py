"""The page-scope posterior kernel without a GPU: tests/native/sim_forced_page_post.cpp compiles
csrc/ta_forced_page_post.hip ITSELF for the host (a wave = 64 coroutines that meet at every DPP move, ballot and hand-over
of LDS; tests/native/hipshim, sim_forced_shim.h and sim_forced_conf_shim.h; -ffp-contract=off as the library's build) and
every word it writes must equal the checker tests/forced_page_post_ref.py bit for bit -- the cases of
tests/forced_page_cases.py with the queries of tests/forced_page_post_cases.py, which tests/test_forced_page_post_gpu.py
drives through the real kernel."""
import ctypes

import numpy as np
import pytest

import forced_cases as C0
import forced_page_cases as PC
import forced_page_post_cases as C
import forced_page_post_ref as R
import forced_page_ref as PR
import simlib


@pytest.fixture(scope="module")
def sim():
    deps = [simlib.NAT + "sim_forced_conf_shim.h", simlib.CSRC + "ta_forced_page_post.hip", simlib.CSRC + "forced_page_two_fill.h", simlib.CSRC + "forced_page_common.h",
            simlib.CSRC + "forced_post_cells.h", simlib.CSRC + "forced_two_fill.h"] + C0.SIM_DEPS
    return C.bind(simlib.load("forced_page_post", deps, flags=["-ffp-contract=off"], include=["hipshim"]))


def _run(lib, pk, **over):
    return C.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, **over)


@pytest.mark.parametrize("which", C.SETS)
@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_host_build_of_the_kernel_equals_the_checker(sim, case, which):
    name, no, pages = case
    want = C.want(name, pages)[which]
    pk = C.pack(sim, pages, no, [(w["line"], w["frame"]) for w in want])
    assert _run(sim, pk) == 0
    C.check(pk, want)


def test_workspace_bytes(sim):
    f = sim.ta_forced_page_posterior_workspace_bytes
    # per character a forward row of 64 K doubles, then 64 K int32: 768 K n bytes
    assert f(1, 2) == 1536 and f(9, 2) == 13824 and f(70, 4) == 3072 * 70 and f(300, 8) == 6144 * 300
    assert f(1027, 32) == 24576 * 1027 and f(5, 16) == 12288 * 5 and f(1 << 29, 32) == 3 << 42
    for n, K in ((0, 2), (-1, 2), ((1 << 29) + 1, 2), (5, 0), (5, 3), (5, 64), (5, -2)):
        assert f(n, K) == -1


def _three(rng):
    return [PC._page(rng, (12, 11), 8, (0, 3), (4, 8), 6), PC._page(rng, (10, 9, 11), 9, (0, 1, 6), (5, 6, 9), 6),
            PC._wide(rng, 70)]


def _wants(rng, pages):
    return [C.answer(pg, *C.seeded_queries(rng, [len(P) for P in pg[0]], len(pg[1]), pg[2], pg[3])) for pg in pages]


def test_a_page_without_a_path_between_two_good_ones(sim):
    rng = np.random.default_rng(11)
    pages = _three(rng)
    pages[1] = PC._page(rng, (2, 1), 5, (0, 2), (4, 5), 6)              # five characters on three frames
    want = _wants(rng, pages)
    assert [w["status"] for w in want] == [PR.OK, PR.NOPATH, PR.OK]
    pk = C.pack(sim, pages, 6, [(w["line"], w["frame"]) for w in want])
    assert _run(sim, pk) == 0
    C.check(pk, want)


def test_a_page_refused_through_its_data_leaves_its_neighbours_alone(sim):
    rng = np.random.default_rng(7)
    pages = _three(rng)
    want = _wants(rng, pages)
    # page 1's lines have 10, 9 and 11 frames and the windows [0, 5), [1, 6), [6, 9); its queries are chosen by hand
    ql, qt = np.asarray([0, 0, 0, 0, 0, 1, 2, 2, 2], np.int32), np.asarray([0, 2, 2, 5, 9, 4, 0, 3, 10], np.int32)
    want[1] = C.answer(pages[1], ql, qt)
    queries = [(w["line"], w["frame"]) for w in want]

    def refused(status, **edit):
        pk = C.pack(sim, pages, 6, queries)
        for name, (k, v) in edit.items():
            getattr(pk, name)[k] = v
        host = {h: getattr(C.pack(sim, pages, 6, queries), h[:-5]) for h in C.HOST}      # the host's copies stay right
        assert _run(sim, pk, **host) == 0
        w = list(want)
        w[1] = C.refused(status)
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
    refused(PR.BOUNDS, pws_off=(1, 8))
    refused(PR.BOUNDS, pws_off=(1, 10 ** 12))
    refused(PR.BOUNDS, pws_off=(1, -16))

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
        R.query(*pages[1], np.asarray([0, 0, 0, 1, 0, 1, 2, 2, 2]), qt * 0)
    # the device's windows ask for a variant that the host's copies did not launch: refused, not left without a status
    wide = PC._page(np.random.default_rng(8), (150, 12), 73, (0, 68), (70, 73), 6)
    two = [pages[0], wide]
    w2 = _wants(rng, two)
    pk2 = C.pack(sim, two, 6, [(w["line"], w["frame"]) for w in w2])
    narrow, early = pk2.hi.copy(), pk2.lo.copy()
    narrow[2], early[3] = 60, 58                          # the host's copy says K = 2, the device's 70 characters need K = 4
    assert _run(sim, pk2, hi_host=narrow, lo_host=early) == 0
    C.check(pk2, [w2[0], C.refused(PR.BOUNDS)])
    # equal neighbours are allowed
    same = [(l.copy(), t.copy()) for l, t in queries]
    same[1][0][6:], same[1][1][6:] = 2, 4
    pk = C.pack(sim, pages, 6, same)
    assert _run(sim, pk) == 0
    w = list(want)
    w[1] = C.answer(pages[1], *same[1])
    C.check(pk, w)


def test_host_side_refusals_touch_nothing(sim):
    rng = np.random.default_rng(9)
    pages = _three(rng)[:2]
    want = _wants(rng, pages)
    pk = C.pack(sim, pages, 6, [(w["line"], w["frame"]) for w in want])
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
    sim.sim_forced_page_post_last_error.restype = ctypes.c_char_p
    last_error = sim.sim_forced_page_post_last_error
    null = "null pointer argument"
    # every refusal with its text, word for word: forced_check_pages', with the rule of this call's workspace
    refusals = [("null " + name, EINVAL, null, {name: None}) for name in
                ("probs", "query", "own_m", "own_x", "rival_m", "rival_x", "rival_state", "z_m", "z_x", "pstatus", "workspace", "lo_host")]
    refusals += [
        ("negative npages", EINVAL, "negative size", dict(npages=-1)), ("negative rows", EINVAL, "negative size", dict(rows=-1)),
        ("no = 1", EINVAL, "no outside 2 .. TA_TRAIN_MAX_CLASSES", dict(no=1)), ("no = 129", EINVAL, "no outside 2 .. TA_TRAIN_MAX_CLASSES", dict(no=129)),
        ("rows too few", EINVAL, "the lines' timesteps exceed rows", dict(rows=int(pk.T.sum()) - 1)),
        ("nlabels too few", EINVAL, "the pages' texts exceed nlabels", dict(nlabels=int(pk.lab_off[-1]) - 1)),
        ("workspace too small", EINVAL, "workspace smaller than the pages' ta_forced_page_posterior_workspace_bytes", dict(workspace_bytes=need - 1)),
        ("workspace misaligned", EINVAL, "workspace not 16-byte aligned", dict(workspace=pk.pws.ctypes.data + 4)),
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
    # more than 2^24 frames on one page: 3 356 lines of 5 000 frames; 2^24 frames exactly pass this check
    for nl, last, refused in ((3356, 5000, True), (3356, 2216, False)):
        T_big = np.full(nl, 5000, np.int32)
        T_big[-1] = last
        assert (int(T_big.sum()) > 1 << 24) == refused and int(T_big.sum()) >= 1 << 24
        big = dict(nlines=nl, npages=1, rows=1 << 23, T_host=T_big, lo_host=np.zeros(nl, np.int32),
                   hi_host=np.full(nl, 8, np.int32), line_first_host=np.asarray([0, nl], np.int64),
                   lab_off_host=np.asarray([int(pk.lab_off[0]), int(pk.lab_off[0]) + 8], np.int64))
        assert _run(sim, pk, **big) == (ELIMIT if refused else EINVAL)
        assert last_error().decode() == ("a page has more than 2^24 frames" if refused else "the lines' timesteps exceed rows")
        assert C.untouched(pk)
    assert _run(sim, pk, npages=0) == 0 and C.untouched(pk)
    assert _run(sim, pk) == 0
    C.check(pk, want)


def test_the_kernel_refuses_a_page_of_more_than_2_24_frames(sim):
    """the device's own count: the host's copies say lines of one frame, the device's T add up to 2^24 + 8 frames"""
    rng = np.random.default_rng(12)
    nl = 3356
    small = PC._page(rng, (9,), 3, (0,), (3,), 4)
    pk = C.pack(sim, [small], 4, [C.seeded_queries(rng, [9], 3, [0], [3])])
    # one block of 5 000 rows serves every line of the long page: the rows may overlap, the kernel never gets to read them
    T = np.full(nl, 5000, np.int32)
    T[-1] = (1 << 24) + 8 - 5000 * (nl - 1)
    row_off = np.zeros(nl, np.int64)
    probs = np.ascontiguousarray(PC.probs(rng, 5000, 4))
    lo, hi = np.zeros(nl, np.int32), np.full(nl, 3, np.int32)
    line_first = np.asarray([0, nl], np.int64)
    host_T = np.full(nl, 1, np.int32)
    over = dict(probs=probs.ctypes.data, row_off=row_off.ctypes.data, T=T.ctypes.data, lo=lo.ctypes.data, hi=hi.ctypes.data,
                line_first=line_first.ctypes.data, nlines=nl, rows=len(probs), T_host=host_T, lo_host=lo, hi_host=hi,
                line_first_host=line_first)
    assert _run(sim, pk, **over) == 0
    assert int(pk.pstatus[0]) == PR.BOUNDS
    pk.pstatus[0] = C.POISON32
    assert C.untouched(pk)
