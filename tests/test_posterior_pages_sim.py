"""ta_posterior_pages without a GPU: tests/native/sim_refine_post.cpp compiles csrc/ta_refine_conf.hip ITSELF for the
host (a wave = 64 coroutines that meet at every ballot / barrier; tests/native/hipshim) and every word it writes must
equal the plain-numpy checker tests/refine_post_ref.py bit for bit -- the cases of tests/refine_post_cases.py, which
tests/test_posterior_pages_gpu.py drives through the real kernel.  Every output is poisoned and no offset is 0."""
import numpy as np
import pytest

import refine_post_cases as C
import refine_post_ref as R
import simlib


@pytest.fixture(scope="module")
def sim():
    deps = [simlib.HIPSHIM, simlib.CSRC + "ta_refine_conf.hip", simlib.HEADER]
    return C.bind(simlib.load("refine_post", deps, include=["hipshim"]))


def _run(lib, pk, **over):
    return C.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, **over)


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64).tolist()


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
        st, cp, sp = got[name][0]                        # the front page: characters 1 .. 3 valued
        assert st == R.OK and np.isnan(cp).tolist() == [True, False, False, False, True, True]
        assert np.isnan(sp).tolist() == [False, False, True]
    nan = float("nan")
    st, cp, sp = got["no refined line"][1]
    assert st == R.OK and _bits(cp) == [C.NAN] * 9 and _bits(sp) == [C.NAN] * 2
    st, cp, sp = got["a syllable with no valued character"][1]
    assert st == R.OK and _bits(sp[:2]) == [C.NAN] * 2 and sp[2] == cp[:4].min()
    st, cp, sp = got["a syllable across two refined lines with different z"][1]
    assert st == R.OK and _bits(cp) == _bits([1.0, 0.5, 1.0, 0.5, 1.0, 0.125, 0.5, nan]) and _bits(sp) == _bits([0.5, 0.125, 0.5, nan])
    st, cp, sp = got["zero masses"][1]
    assert st == R.OK and _bits(cp) == _bits([0.0, 2.0 ** -2 / 1.5, 0.0, 0.0, nan, nan])
    assert _bits(sp) == _bits([0.0, 0.0, 2.0 ** -2 / 1.5, 0.0, nan])
    assert got["an empty transcript"][1][0] == R.OK and len(got["an empty transcript"][1][1]) == 0
    assert _bits(got["a page off the array path"][1][1]) == [C.NAN] * 12 and len(got["a page off the array path"][1][2]) == 0
    big = got["more than 64 lines, syllables and characters"]
    assert [a[0] for a in big] == [R.OK] * 3 and len(big[1][2]) > 64 and (~np.isnan(big[2][1])).sum() > 64
    want = {"a syllable behind the page's characters": R.RANGE, "a syllable in front of the page's characters": R.RANGE,
            "a syllable whose range is turned round": R.RANGE, "a table row behind the page's characters": R.TABLE,
            "a table row in front of the page's characters": R.TABLE, "a refined line without a slot": R.SLOT,
            "a refined line the confidence skipped": R.STATUS, "a refined line the confidence refused": R.STATUS}
    for name, status in want.items():                     # every status code, each between two good pages
        assert [a[0] for a in got[name]] == [R.OK, R.OK, status, R.OK], name
        assert got[name][2][1:] == (None, None)


def test_the_division_pages_on_the_host_build(sim):
    """the pairs tests/test_posterior_pages_gpu.py decides the device's division with, through the host's division here"""
    from text_alignment_amd import forced
    pages = C.division_pages()
    pk = C.pack(pages, seed=5)
    assert _run(sim, pk) == 0
    C.check_division(pk, pages, forced.posterior_values)


def test_count_limits_the_slots(sim):
    name, pages = [c for c in C.cases() if c[0] == "three pages"][0]
    full = C.want(C.pack(pages, seed=3))
    for count in (-1, 0, 1, 3):
        pk = C.pack(pages, seed=3, count=count)
        answer = C.want(pk)
        assert _run(sim, pk) == 0
        C.compare(pk, answer)
        assert {a[0] for a in answer} <= {R.OK, R.SLOT}
    pk = C.pack(pages, seed=3, count=1 << 40)             # more than the arrays hold: the poisoned slots stay unread
    assert _run(sim, pk) == 0
    C.compare(pk, full)


def test_a_page_whose_own_numbers_are_out_of_bounds_is_left_alone(sim):
    name, pages = [c for c in C.cases() if c[0] == "three pages"][0]
    for field, at, v, hit in (("t_off", 2, -1, (1, 2)), ("t_off", 3, 1 << 40, (2, 3)), ("line_first", 3, 1000, (2, 3)),
                              ("line_first", 2, -2, (1, 2)), ("syl_off", 2, 1 << 33, (1, 2)), ("syl_off", 4, -7, (3,))):
        pk = C.pack(pages, seed=1)
        answer, was = C.want(pk), getattr(pk, field)[at]
        getattr(pk, field)[at] = v
        assert _run(sim, pk) == 0
        getattr(pk, field)[at] = was                      # compare lays the answer out by the true offsets
        assert [int(pk.status[p]) for p in hit] == [R.BOUNDS] * len(hit), (field, at)
        C.compare(pk, answer, skip=hit)


def test_a_slot_whose_labels_leave_label_cap_refuses_its_page(sim):
    name, pages = [c for c in C.cases() if c[0] == "three pages"][0]
    pk = C.pack(pages, seed=2)
    answer = C.want(pk)
    k = int(pk.slot[int(pk.line_first[2])])                 # the page of one refined line
    for v in (-1, pk.label_cap - int(pk.L[k]) + 1, 1 << 50):
        was, pk.lab_off[k] = pk.lab_off[k], v
        pk.char_post.view(np.int64)[:], pk.syl_post.view(np.int64)[:], pk.status[:] = C.POISON64, C.POISON64, C.POISON32
        assert _run(sim, pk) == 0
        pk.lab_off[k] = was
        assert pk.status[2] == R.TABLE
        C.compare(pk, answer, skip=(2,))
        a, b = int(pk.t_off[2]), int(pk.t_off[3])
        assert (pk.char_post.view(np.int64)[a:b] == C.POISON64).all()


def test_host_side_refusals_touch_nothing(sim):
    name, pages = C.cases()[1]
    pk = C.pack(pages)
    EINVAL, ELIMIT = -1, -4

    def untouched():
        return bool((pk.char_post.view(np.int64) == C.POISON64).all() and (pk.syl_post.view(np.int64) == C.POISON64).all() and
                    (pk.status == C.POISON32).all())
    for what, code, over in ([("null " + n, EINVAL, {n: None}) for n in ("own_m", "own_x", "z_m", "z_x", "count", "slot",
                                                                         "syl_last", "char_post", "syl_post", "status")] +
                             [("negative " + n, EINVAL, {n: -1}) for n in ("nprob", "nslots", "nsyl", "t_len", "label_cap",
                                                                           "nlines")] +
                             [("too many lines", ELIMIT, dict(nlines=(1 << 24) + 1))]):
        assert _run(sim, pk, **over) == code, what
        assert untouched(), what
    assert _run(sim, pk, nprob=0) == 0 and untouched()
    assert _run(sim, pk) == 0
    C.compare(pk)
