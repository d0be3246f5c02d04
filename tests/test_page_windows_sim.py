"""The page-scope window kernel without a GPU: tests/native/sim_page_windows.cpp compiles csrc/ta_page_windows.hip ITSELF
for the host (a wave = 64 coroutines that meet at every wave-wide operation) and every word it writes must equal
forced.page_scope_eligibility / forced.page_windows -- the cases of tests/page_windows_cases.py, which
tests/test_page_windows_gpu.py drives through the real kernel."""
import ctypes

import numpy as np
import pytest

import forced_cases as C0
import page_windows_cases as C
import simlib

BAD_OFFSETS = (("t_off", 2, 3), ("line_first", 2, 10 ** 6), ("t_off", 2, 10 ** 9), ("line_first", 2, -1), ("t_off", 2, -5))
DEPS = [simlib.CSRC + "ta_page_windows.hip", simlib.NAT + "sim_forced_omit_shim.h"] + C0.SIM_DEPS


@pytest.fixture(scope="module")
def sim():
    return C.bind(simlib.load("page_windows", DEPS, include=["hipshim"]))


def _run(lib, pk, m, **over):
    return C.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, m, **over)


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_host_build_of_the_kernel_equals_the_host_rule(sim, case):
    name, margin, pages = case
    pk = C.pack(pages)
    assert _run(sim, pk, margin) == 0
    C.check(pk, C.want(pk.pages, margin))


def test_the_cases_cover_every_reason_and_both_edges():
    """what the case list claims, asserted on the expected answers alone"""
    by_name = {name: C.want(pages, margin) for name, margin, pages in C.cases()}
    assert [r for r, _ in by_name["each reason alone"]] == [1, 2, 3, 4, 5, 5, 6]
    assert [r for r, _ in by_name["adjacent reasons together"]] == [1, 2, 3, 4, 5, 1, 3]
    assert [r for r, _ in by_name["widths 1023 and 1024"]] == [0, 5, 0]
    assert [r for r, _ in by_name["widths 1023 and 1024 through the margin"]] == [0, 5]
    lo, hi = by_name["widths 1023 and 1024"][0][1]
    assert int((hi - lo).max()) == C.MAX_TARGET
    lo, hi = by_name["widths 1023 and 1024 through the margin"][0][1]
    assert int((hi - lo).max()) == C.MAX_TARGET
    assert [r for r, _ in by_name["n against the frames"]] == [0, 6]
    reasons = [r for name, w in by_name.items() if name.startswith("random") for r, _ in w]
    assert len(reasons) == 300 and {0, 1, 2, 3, 5, 6} <= set(reasons)


def test_three_pages_in_one_launch_and_a_page_out_of_bounds_between_good_ones(sim):
    rows, n = C.chain(70, L=2, gap=1)
    pages = [C.page(C.EXAMPLE, 37, T=[40, 40, 40, 19]), C.page(rows, n), C.page(C.EXAMPLE, 37, T=[9, 9, 9, 9])]
    pk = C.pack(pages)
    assert pk.line_first[1] > 0 and pk.t_off[1] > 0
    assert _run(sim, pk, 16) == 0
    C.check(pk, C.want(pk.pages, 16))
    # offsets that decrease or leave the arrays.  t_off[2] = 3 refuses page 1 alone, between two good ones: page 2 then owns
    # the characters its own numbers say (reading overlaps, writing does not); an offset outside the arrays refuses both
    # pages it belongs to, between pages 0 and 3
    for name, k, v in BAD_OFFSETS:
        pk = C.pack(pages)
        getattr(pk, name)[k] = v
        assert _run(sim, pk, 16) == 0
        bad = [p for p in range(pk.npages)
               if not (0 <= pk.line_first[p] <= pk.line_first[p + 1] <= pk.nlines and 0 <= pk.t_off[p] <= pk.t_off[p + 1] <= pk.t_len)]
        assert bad == ([1] if v == 3 else [1, 2])
        wanted = []
        for p in range(pk.npages):
            a, b, c, d = int(pk.line_first[p]), int(pk.line_first[p + 1]), int(pk.t_off[p]), int(pk.t_off[p + 1])
            if p in bad:
                assert int(pk.reason[p]) == C.BOUNDS, (name, k, v, p)
                continue
            pg = dict(plain=bool(pk.plain[p]), status=int(pk.h_status[p]), classes=pk.t_class[c:d], rows=pk.table[a:b], T=pk.T[a:b])
            wanted.append((p, C.want([pg], 16)[0]))
        assert len(wanted) >= 2
        touched = np.zeros(pk.nlines, bool)
        for p, (reason, win) in wanted:
            a, b = int(pk.line_first[p]), int(pk.line_first[p + 1])
            assert int(pk.reason[p]) == reason, (name, k, v, p)
            if reason == 0:
                assert np.array_equal(pk.lo[a:b], win[0]) and np.array_equal(pk.hi[a:b], win[1]), (name, k, v, p)
                touched[a:b] = True
        assert (pk.lo[~touched] == C.POISON32).all() and (pk.hi[~touched] == C.POISON32).all(), (name, k, v)


def test_host_side_refusals_touch_nothing(sim):
    pk = C.pack([C.page(C.EXAMPLE, 37, T=[40, 40, 40, 19])])
    sim.sim_page_windows_last_error.restype = ctypes.c_char_p
    EINVAL = -1
    refusals = [("null pointer argument", dict(table=None)), ("null pointer argument", dict(h_status=None)),
                ("null pointer argument", dict(line_first=None)), ("null pointer argument", dict(t_off=None)),
                ("null pointer argument", dict(t_class=None)), ("null pointer argument", dict(T=None)),
                ("null pointer argument", dict(plain=None)), ("null pointer argument", dict(lo=None)),
                ("null pointer argument", dict(hi=None)), ("null pointer argument", dict(reason=None)),
                ("negative size", dict(npages=-1)), ("negative size", dict(nlines=-1)), ("negative size", dict(t_len=-1)),
                ("negative margin", dict(margin=-1))]
    for text, over in refusals:
        assert _run(sim, pk, 16, **over) == EINVAL, over
        assert sim.sim_page_windows_last_error().decode() == text, over
        assert (pk.lo == C.POISON32).all() and (pk.hi == C.POISON32).all() and (pk.reason == C.POISON32).all(), over
    assert _run(sim, pk, 16, npages=0) == 0 and (pk.reason == C.POISON32).all() and (pk.lo == C.POISON32).all()
    assert _run(sim, pk, 16, npages=0, table=None, reason=None) == 0
    assert _run(sim, pk, 16) == 0
    C.check(pk, C.want(pk.pages, 16))

