"""ta_refine_columns without a GPU: tests/native/sim_refine.cpp compiles csrc/ta_refine.hip ITSELF for the host (a wave =
64 coroutines that meet at every ballot / barrier; tests/native/hipshim) and every integer it writes must equal the
plain-Python checker tests/refine_ref.py -- the cases of tests/refine_cases.py, which tests/test_refine_gpu.py drives
through the real kernel.  Every output is poisoned and no offset is 0."""
import numpy as np
import pytest

import refine_cases as C
import refine_ref as R
import simlib


@pytest.fixture(scope="module")
def sim():
    deps = [simlib.HIPSHIM, simlib.CSRC + "ta_refine.hip", simlib.HEADER]
    return C.bind(simlib.load("refine", deps, include=["hipshim"]))


def _run(lib, pk, **over):
    return C.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, **over)


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_host_build_of_the_kernel_equals_the_checker(sim, case):
    name, chunk = case
    pk = C.pack(chunk, seed=len(name))
    assert _run(sim, pk) == 0
    C.compare(pk)


def test_the_cases_are_what_their_names_say():
    """the checker's own verdicts: which case refines what, which page gets which status"""
    got = {}
    for name, chunk in C.cases():
        pk = C.pack(chunk, seed=len(name))
        per_page, refined, _ = C.want(pk)
        own = refined[int(pk.line_first[1]):]
        got[name] = ([st for st, _, _ in per_page][1:], own.tolist(), refined[0])
    assert all(g[2] == 1 for name, g in got.items() if name != "count -1")       # the front page's line
    assert got["count -1"] == ([0], [0] * 4, 0)
    assert got["no line refined"][1] == [0] * 4 and got["every line refined"][1] == [1] * 4
    assert got["only the first line"][1] == [1, 0, 0, 0] and got["only the last line"][1] == [0, 0, 0, 1]
    assert got["L = 1"][1] == [1, 1, 0] and got["an expanded abbreviation"][1] == [0, 1]
    assert got["a page that is not plain"] == ([0, 0], [0, 0, 0, 1, 1], 1)
    assert got["a slot the forced alignment refused"][1] == [1, 1, 0, 0]
    assert got["count below the slots"][1] == [1, 1, 0, 0]
    assert got["a page the harvest refused"][0] == [0, R.HARVEST, 0]
    assert got["kept characters in front of the run"] == ([0, R.CONTAIN, 0], [1, 1, 0, 0, 1, 1], 1)
    assert got["kept characters behind the run"][0] == [R.CONTAIN, 0]
    assert got["a slot whose L is not the table's"][0] == [R.CONTAIN, 0]
    assert got["a refined line without OCR characters"][0] == [R.CONTAIN]
    assert got["o_line decreases"][0] == [R.COLUMNS, 0] and got["a column code above 2"][0] == [R.COLUMNS, 0]
    assert sum(sum(g[1]) for g in got.values()) > 60


def test_a_page_whose_own_numbers_are_out_of_bounds_is_left_alone(sim):
    name, chunk = [c for c in C.cases() if c[0] == "three pages"][0]
    for field, p, v in (("ops_len", 2, -1), ("ops_len", 2, 10 ** 6), ("ops_off", 2, -4), ("t_off", 3, 1 << 40),
                        ("line_first", 4, 1000)):
        pk, was = C.pack(chunk, seed=1), C.pack(chunk, seed=1)
        answer = C.want(pk)
        getattr(pk, field)[p] = v
        assert _run(sim, pk) == 0
        hit = [q for q in range(pk.nprob) if (q == 2 and field in ("ops_len", "ops_off")) or (field == "t_off" and q in (2, 3))
               or (field == "line_first" and q == 3)]
        for q in range(pk.nprob):
            r0 = int(was.ops_off[q])
            if q in hit:
                assert pk.status[q] == R.BOUNDS and pk.ops_new_len[q] == -1 and pk.idx_new_len[q] == -1
                lf0, lf1 = int(was.line_first[q]), int(was.line_first[q + 1])
                assert (pk.refined[lf0:lf1] == C.POISON32).all() and (pk.slot[lf0:lf1] == C.POISON32).all()
                assert (pk.ops_new[r0:int(was.ops_off[q + 1])] == C.POISON8).all()
            else:
                st, ops, idx = answer[0][q]
                assert pk.status[q] == st and pk.ops_new_len[q] == len(ops)
                assert np.array_equal(pk.ops_new[r0:r0 + len(ops)], ops) and np.array_equal(pk.idx_new[r0:r0 + len(idx)], idx)


def test_host_side_refusals_touch_nothing(sim):
    name, chunk = C.cases()[3]
    pk = C.pack(chunk)
    EINVAL, ELIMIT = -1, -4
    for what, code, over in (("null ops", EINVAL, dict(ops=None)), ("null idx", EINVAL, dict(idx=None)),
                             ("null count", EINVAL, dict(count=None)), ("null plain", EINVAL, dict(plain=None)),
                             ("null status", EINVAL, dict(status=None)), ("null slot", EINVAL, dict(slot=None)),
                             ("negative nprob", EINVAL, dict(nprob=-1)), ("negative nslots", EINVAL, dict(nslots=-1)),
                             ("negative box_base", EINVAL, dict(box_base=-1)), ("negative ops_bytes", EINVAL, dict(ops_bytes=-1)),
                             ("too many lines", ELIMIT, dict(nlines=(1 << 24) + 1)),
                             ("box rows beyond 32 bits", ELIMIT, dict(box_base=2 ** 31 - 5))):
        assert _run(sim, pk, **over) == code, what
        for out in C.OUTPUTS:
            a = getattr(pk, out)
            assert (a == (C.POISON8 if a.dtype == np.uint8 else C.POISON32)).all(), what
    assert _run(sim, pk, nprob=0) == 0 and (pk.status == C.POISON32).all()
    assert _run(sim, pk) == 0
    C.compare(pk)
