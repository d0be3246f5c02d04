"""ta_confidence_pages without a GPU: tests/native/sim_refine_conf.cpp compiles csrc/ta_refine_conf.hip ITSELF for the
host (a wave = 64 coroutines that meet at every ballot / barrier; tests/native/hipshim) and every integer it writes must
equal the plain-Python checker tests/refine_conf_ref.py -- the cases of tests/refine_conf_cases.py, which
tests/test_forced_conf_lines_gpu.py drives through the real kernel.  Every output is poisoned and no offset is 0."""
import numpy as np
import pytest

import refine_conf_cases as C
import refine_conf_ref as R
import simlib


@pytest.fixture(scope="module")
def sim():
    deps = [simlib.HIPSHIM, simlib.CSRC + "ta_refine_conf.hip", simlib.HEADER]
    return C.bind(simlib.load("refine_conf", deps, include=["hipshim"]))


def _run(lib, pk, **over):
    return C.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, **over)


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_host_build_of_the_kernel_equals_the_checker(sim, case):
    name, pages = case
    pk = C.pack(pages, seed=len(name))
    assert _run(sim, pk) == 0
    C.compare(pk)


def test_the_cases_are_what_their_names_say():
    """the checker's own verdicts, and the values the named cases are about"""
    got = {}
    for name, pages in C.cases():
        pk = C.pack(pages, seed=len(name))
        got[name] = C.want(pk)
        assert got[name][0] == (R.OK, [C.NO, 7, -2, 9, C.NO, C.NO], [7, -2, C.NO])            # the front page
    NO = C.NO
    assert got["no refined line"][1] == (R.OK, [NO] * 9, [NO, NO])
    assert got["a syllable across a refined and an unrefined line"][1] == (
        R.OK, [50, 40, 30, 20, NO, NO, NO, NO, NO], [40, 20, NO])
    st, cc, sc = got["a syllable with no valued character"][1]
    assert st == R.OK and sc[:2] == [NO, NO] and sc[2] == min(cc[:4]) != NO
    assert got["an empty transcript"][1] == (R.OK, [], []) and got["a page without lines"][1] == (R.OK, [NO] * 5, [NO])
    assert got["a page off the array path"][1] == (R.OK, [NO] * 12, [])
    assert got["zero and negative values"][1] == (R.OK, [0, 5, -3, NO, -(1 << 40), 0, 0, NO + 1],
                                                  [0, -3, -3, NO, -(1 << 40), 0, NO + 1, NO + 1])
    assert got["an unrefined line with a refused slot"][1][0] == R.OK
    big = got["more than 64 lines, syllables and characters"]
    assert [a[0] for a in big] == [R.OK] * 3 and len(big[1][2]) > 64 and sum(c != NO for c in big[2][1]) > 64
    want = {"a syllable behind the page's characters": R.RANGE, "a syllable in front of the page's characters": R.RANGE,
            "a syllable whose range is turned round": R.RANGE, "a table row behind the page's characters": R.TABLE,
            "a table row in front of the page's characters": R.TABLE, "a refined line without a slot": R.SLOT,
            "a refined line the confidence skipped": R.STATUS, "a refined line the confidence refused": R.STATUS}
    for name, status in want.items():                     # each between two good pages
        assert [a[0] for a in got[name]] == [R.OK, R.OK, status, R.OK], name
        assert got[name][2][1:] == (None, None)


def test_count_limits_the_slots(sim):
    name, pages = [c for c in C.cases() if c[0] == "three pages"][0]
    full = C.want(C.pack(pages, seed=3))
    for count in (-1, 0, 1, 3):
        pk = C.pack(pages, seed=3, count=count)
        answer = C.want(pk)
        assert _run(sim, pk) == 0
        C.compare(pk, answer)
        for p, pg in enumerate(pk.pages):                 # a page that refines nothing needs no slot; any other is refused
            lf0, lf1 = int(pk.line_first[p]), int(pk.line_first[p + 1])
            ks = [int(pk.slot[q]) for q in range(lf0, lf1) if pk.refined[q]]
            assert answer[p][0] == (R.SLOT if any(k >= max(count, 0) for k in ks) else R.OK)
            if answer[p][0] == R.OK:
                assert answer[p] == full[p]
    pk = C.pack(pages, seed=3, count=1 << 40)             # more than the arrays hold: the poisoned slots stay unread
    assert _run(sim, pk) == 0
    C.compare(pk, full)


def test_a_page_whose_own_numbers_are_out_of_bounds_is_left_alone(sim):
    name, pages = [c for c in C.cases() if c[0] == "three pages"][0]
    for field, at, v, hit in (("t_off", 2, -1, (1, 2)), ("t_off", 3, 1 << 40, (2, 3)), ("line_first", 3, 1000, (2, 3)),
                              ("line_first", 2, -2, (1, 2)), ("syl_off", 2, 1 << 33, (1, 2)), ("syl_off", 4, -7, (3,))):
        pk = C.pack(pages, seed=1)
        answer = C.want(pk)
        getattr(pk, field)[at] = v
        assert _run(sim, pk) == 0
        getattr(pk, field)[at] = C.pack(pages, seed=1).__dict__[field][at]    # compare lays the answer out by the true offsets
        assert [int(pk.status[p]) for p in hit] == [R.BOUNDS] * len(hit), (field, at)
        C.compare(pk, answer, skip=hit)


def test_a_slot_whose_labels_leave_label_cap_refuses_its_page(sim):
    name, pages = [c for c in C.cases() if c[0] == "three pages"][0]
    pk = C.pack(pages, seed=2)
    answer = C.want(pk)
    k = int(pk.slot[int(pk.line_first[2])])                 # the page of one refined line
    for v in (-1, pk.label_cap - int(pk.L[k]) + 1, 1 << 50):
        was, pk.lab_off[k] = pk.lab_off[k], v
        for name in C.OUTPUTS:
            getattr(pk, name)[:] = C.POISON32 if name == "status" else C.POISON64
        assert _run(sim, pk) == 0
        pk.lab_off[k] = was
        assert pk.status[2] == R.TABLE
        C.compare(pk, answer, skip=(2,))
        a, b = int(pk.t_off[2]), int(pk.t_off[3])
        assert (pk.char_conf[a:b] == C.POISON64).all()


def test_host_side_refusals_touch_nothing(sim):
    name, pages = C.cases()[1]
    pk = C.pack(pages)
    EINVAL, ELIMIT = -1, -4
    for what, code, over in (("null confidence", EINVAL, dict(confidence=None)), ("null count", EINVAL, dict(count=None)),
                             ("null slot", EINVAL, dict(slot=None)), ("null syl_last", EINVAL, dict(syl_last=None)),
                             ("null char_conf", EINVAL, dict(char_conf=None)), ("null status", EINVAL, dict(status=None)),
                             ("negative nprob", EINVAL, dict(nprob=-1)), ("negative nslots", EINVAL, dict(nslots=-1)),
                             ("negative nsyl", EINVAL, dict(nsyl=-1)), ("negative t_len", EINVAL, dict(t_len=-1)),
                             ("negative label_cap", EINVAL, dict(label_cap=-1)),
                             ("too many lines", ELIMIT, dict(nlines=(1 << 24) + 1))):
        assert _run(sim, pk, **over) == code, what
        assert (pk.char_conf == C.POISON64).all() and (pk.syl_conf == C.POISON64).all() and (pk.status == C.POISON32).all()
    assert _run(sim, pk, nprob=0) == 0 and (pk.status == C.POISON32).all()
    assert _run(sim, pk) == 0
    C.compare(pk)
