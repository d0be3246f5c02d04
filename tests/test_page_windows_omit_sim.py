"""The page-scope window kernel for the lattice with omission without a GPU: tests/native/sim_page_windows_omit.cpp compiles
csrc/ta_page_windows_omit.hip ITSELF for the host (page_windows.h's kernel with kOmit = true) and every word it writes must
equal forced.page_scope_eligibility(..., omit=True) -- the pages of tests/page_windows_cases.py and the limit pages of
tests/page_windows_omit_cases.py, which tests/test_page_windows_omit_gpu.py drives through the real kernel.

The issue asked for the page of 2^20 characters to have ONE line; such a page has the window [0, n) and is PAGE_WINDOWS under
either rule, so the limit pages here have 1026 lines whose windows are 1023 characters wide (page_windows_omit_cases)."""
import ctypes

import numpy as np
import pytest

import forced_cases as C0
import page_windows_cases as C
import page_windows_omit_cases as O
import simlib

DEPS = [simlib.CSRC + "ta_page_windows_omit.hip", simlib.CSRC + "page_windows.h", simlib.CSRC + "forced_page_common.h",
        simlib.NAT + "sim_forced_omit_shim.h"] + C0.SIM_DEPS
FRAMES = 6


@pytest.fixture(scope="module")
def sim():
    return O.bind(simlib.load("page_windows_omit", DEPS, include=["hipshim"]))


def _run(lib, pk, m, **over):
    return O.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, m, **over)


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_host_build_of_the_kernel_equals_the_host_rule(sim, case):
    name, margin, pages = case
    pk = C.pack(pages)
    assert _run(sim, pk, margin) == 0
    wanted = O.want(pk.pages, margin)
    strict = C.want(pk.pages, margin)
    for (r, w), (rs, ws) in zip(wanted, strict):         # FRAMES under the strict rule: reason 0 here, with windows
        assert r != FRAMES and (r == rs or (rs == FRAMES and r == 0 and w is not None))
    C.check(pk, wanted)                                  # (poison stays in lo / hi of every page with a reason)


def test_the_cases_hold_pages_the_strict_rule_calls_frames():
    strict = [r for name, margin, pages in C.cases() for r, _ in C.want(pages, margin)]
    omit = [r for name, margin, pages in C.cases() for r, _ in O.want(pages, margin)]
    assert strict.count(FRAMES) >= 3 and FRAMES not in omit
    assert [o for s, o in zip(strict, omit) if s == FRAMES] == [0] * strict.count(FRAMES)


@pytest.mark.parametrize("case", O.limit_cases(), ids=lambda c: c[0])
def test_the_limits_of_the_lattice_with_omission(sim, case):
    name, margin, pages, reasons = case
    pk = C.pack(pages)
    wanted = O.want(pk.pages, margin)
    assert [r for r, _ in wanted] == [0] + reasons        # (the page in front)
    assert _run(sim, pk, margin) == 0
    C.check(pk, wanted)


def test_host_side_refusals_touch_nothing(sim):
    pk = C.pack([C.page(C.EXAMPLE, 37, T=[9, 9, 9, 9])])
    sim.sim_page_windows_omit_last_error.restype = ctypes.c_char_p
    EINVAL = -1
    null = "null pointer argument"
    refusals = [(null, dict(table=None)), (null, dict(h_status=None)), (null, dict(line_first=None)), (null, dict(t_off=None)),
                (null, dict(t_class=None)), (null, dict(T=None)), (null, dict(plain=None)), (null, dict(lo=None)),
                (null, dict(hi=None)), (null, dict(reason=None)),
                ("negative size", dict(npages=-1)), ("negative size", dict(nlines=-1)), ("negative size", dict(t_len=-1)),
                ("negative margin", dict(margin=-1))]
    for text, over in refusals:
        assert _run(sim, pk, 16, **over) == EINVAL, over
        assert sim.sim_page_windows_omit_last_error().decode() == text, over
        assert (pk.lo == C.POISON32).all() and (pk.hi == C.POISON32).all() and (pk.reason == C.POISON32).all(), over
    assert _run(sim, pk, 16, npages=0) == 0 and (pk.reason == C.POISON32).all() and (pk.lo == C.POISON32).all()
    assert _run(sim, pk, 16) == 0
    assert pk.reason.tolist() == [0, 0]                  # 37 characters on 36 frames
    C.check(pk, O.want(pk.pages, 16))


def test_a_page_out_of_bounds_between_good_ones(sim):
    pages = [C.page(C.EXAMPLE, 37, T=[9, 9, 9, 9]), C.page(*C.chain(70, L=2, gap=1)), C.page(C.EXAMPLE, 37, T=[9, 9, 9, 9])]
    pk = C.pack(pages)
    pk.t_off[2] = 3                                       # page 1's text ends before it starts
    assert _run(sim, pk, 16) == 0
    assert pk.reason.tolist() == [0, C.BOUNDS, 0, 0]
    a, b = int(pk.line_first[1]), int(pk.line_first[2])
    assert (pk.lo[a:b] == C.POISON32).all() and (pk.hi[a:b] == C.POISON32).all()


def test_the_reasons_are_the_headers():
    from text_alignment_amd import _abi, forced
    assert _abi.CONSTANTS["TA_PAGE_SCOPE_TOO_LONG"] == 8 == forced.PAGE_TOO_LONG
    assert _abi.CONSTANTS["TA_PAGE_SCOPE_ALL_OMITTED"] == 9 == forced.PAGE_ALL_OMITTED
