"""ta_refine_columns_omit without a GPU: tests/native/sim_refine.cpp compiles csrc/ta_refine.hip ITSELF for the host (a
wave = 64 coroutines that meet at every ballot / barrier; tests/native/hipshim), so it exports the second instantiation as
well, and every integer that writes must equal the plain-Python checker tests/refine_omit_ref.py -- the cases of
tests/refine_omit_cases.py, which tests/test_refine_omit_columns_gpu.py drives through the real kernel.  Every output is
poisoned, no offset is 0, and a row of frames the kernel has no business reading would pass for a present character."""
import numpy as np
import pytest

import refine_cases as RC
import refine_omit_cases as C
import refine_omit_ref as R
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
    """the checker's own verdicts: what each case refines, counts and leaves alone"""
    got = {}
    for name, chunk in C.cases():
        pk = C.pack(chunk, seed=len(name))
        per_page, refined, _, omitted = C.want(pk)
        a = int(pk.line_first[1])
        got[name] = ([st for st, _, _ in per_page][1:], refined[a:].tolist(), omitted[a:].tolist(), per_page, pk)
        assert refined[0] == 1 and omitted[0] == 0 or name.endswith("count -1")              # the front page's line
    assert got["the first and the last omitted"][1:3] == ([1, 1], [2, 2])
    assert got["nothing omitted"][1:3] == ([1, 1], [0, 0])
    assert got["L = 1 present and L = 1 omitted"][1:3] == ([1, 0, 0], [0, 1, -1])
    assert got["L = 1 omitted and L = 1 present"][1:3] == ([0, 1, 0], [1, 0, -1])
    st, ref, gone, per_page, pk = got["a line with every character omitted between refined neighbours"]
    assert (st, ref, gone) == ([0], [1, 0, 1], [0, 5, 0])
    assert per_page[1][1].tolist() == [0, 0, 0] + [1] + [0, 2, 0, 1, 0, 2, 0] + [0, 0, 0]   # line 1's run as it was
    st, ref, gone, per_page, pk = got["every line with every character omitted"]
    assert (ref, gone) == ([0, 0, 0], [3, 5, 3]) and np.array_equal(per_page[1][1], pk.pages[1]["ops"])
    assert got["all but one omitted"][1:3] == ([1, 1, 1], [2, 4, 2])
    st, ref, gone, per_page, pk = got["omitted in columns 63 and 64"]
    assert np.flatnonzero(per_page[1][1]).tolist() == [63, 64, 127, 128]
    for L in (64, 65, 1023):
        st, ref, gone, _, _ = got["L = %d scattered" % L]
        assert ref == [1] and 0 < gone[0] < L
    assert got["a slot the forced alignment refused carries live frames"][1] == [1, 1, 0, 0]
    assert got["a slot the forced alignment refused carries live frames"][2][2:] == [-1, -1]
    assert got["a negative first field that is not -1"][2] == [2, 1] and got["the most negative first field"][2] == [2, 1]
    st, ref, gone, _, _ = got["an object-path page"]
    assert ref[:3] == [0, 0, 0] and min(gone[:3]) >= 0 and sum(gone[:3]) > 0 and ref[3:] == [1, 1]
    st, ref, gone, _, _ = got["a page the harvest refused"]
    assert st == [0, R.HARVEST, 0] and gone[2:5] == [-1] * 3 and min(gone[:2] + gone[5:]) >= 0
    st, ref, gone, _, _ = got["a CONTAIN page"]
    assert st == [0, R.CONTAIN, 0] and gone[2:4] == [-1, -1] and ref[2:4] == [0, 0] and min(gone[:2] + gone[4:]) >= 0
    assert got["kept characters in front of the run of a line with every character omitted"][:3] == ([0], [1, 0], [0, 5])
    assert got["a slot whose L is not the table's, every character omitted"][:3] == ([R.CONTAIN], [0, 0], [-1, -1])
    assert got["refine_cases: count -1"][2] == [-1] * 4


@pytest.mark.parametrize("case", RC.cases(), ids=lambda c: c[0])
def test_with_every_character_present_it_is_ta_refine_columns(sim, case):
    name, chunk = case
    pk = C.pack(chunk, seed=len(name))                   # no "gone", no "scatter": every character present
    strict = RC.pack(chunk, seed=len(name))
    assert _run(sim, pk) == 0
    assert RC.call(sim, strict, lambda name: getattr(strict, name).ctypes.data) == 0
    for out in RC.OUTPUTS:
        assert np.array_equal(getattr(pk, out), getattr(strict, out)), out
    per_page, _, slot, omitted = C.want(pk)
    assert all(g in (0, -1) for g in omitted.tolist()) and all(omitted[l] == 0 for l in np.flatnonzero(slot >= 0))


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_the_checkers_columns_are_those_of_the_host_rule(case):
    """per page the checker's ops equal forced.refine_columns(..., present=...)'s -- what refine_pages forms its columns
    with -- and its idx agree once the device's numbering (box_base + lab_off[k] + i) is mapped to that function's
    compact one (the line's first row on, the present characters in order)"""
    from text_alignment_amd import forced
    name, chunk = case
    pk = C.pack(chunk, seed=len(name))
    per_page, refined, slot, _ = C.want(pk)
    compact, next_row = {}, pk.box_base
    for p, pg in enumerate(pk.pages):
        st, ops, idx = per_page[p]
        if st != R.OK:
            continue
        lines, masks = [], []
        for l in range(int(pk.line_first[p]), int(pk.line_first[p + 1])):
            if refined[l]:
                k = int(slot[l])
                here = pk.present[k]
                lines.append((l, int(pk.table[l, 1]), int(pk.L[k]), next_row))
                masks.append(here)
                for r, i in enumerate(np.flatnonzero(here)):
                    compact[pk.box_base + int(pk.lab_off[k]) + int(i)] = next_row + r
                next_row += int(here.sum())
        o_line = pk.o_line[pk.o_off[p]:pk.o_off[p + 1]]
        h_ops, h_idx = forced.refine_columns(pg["ops"], pg["idx"], o_line, lines, present=masks)
        assert np.array_equal(h_ops, ops)
        assert [compact[v] if v >= pk.box_base else v for v in idx.tolist()] == h_idx.tolist()


def test_a_page_whose_own_numbers_are_out_of_bounds_is_left_alone(sim):
    name, chunk = [c for c in C.cases() if c[0] == "refine_cases: three pages"][0]
    pk, was = C.pack(chunk, seed=1), C.pack(chunk, seed=1)
    answer = C.want(pk)
    pk.ops_len[2] = 10 ** 6
    assert _run(sim, pk) == 0
    lf0, lf1 = int(was.line_first[2]), int(was.line_first[3])
    assert pk.status[2] == R.BOUNDS and pk.ops_new_len[2] == -1 and (pk.omitted[lf0:lf1] == C.POISON32).all()
    assert np.array_equal(np.delete(pk.omitted[:pk.nlines], np.r_[lf0:lf1]), np.delete(answer[3], np.r_[lf0:lf1]))
    for q in (0, 1, 3):
        r0, (st, ops, idx) = int(pk.ops_off[q]), answer[0][q]
        assert pk.status[q] == st and np.array_equal(pk.ops_new[r0:r0 + len(ops)], ops)
        assert np.array_equal(pk.idx_new[r0:r0 + len(idx)], idx)


def test_host_side_refusals_touch_nothing(sim):
    name, chunk = C.cases()[0]
    pk = C.pack(chunk)
    EINVAL, ELIMIT = -1, -4
    for what, code, over in (("null ops", EINVAL, dict(ops=None)), ("null frames", EINVAL, dict(frames=None)),
                             ("null omitted", EINVAL, dict(omitted=None)), ("null status", EINVAL, dict(status=None)),
                             ("negative nprob", EINVAL, dict(nprob=-1)), ("negative label_cap", EINVAL, dict(label_cap=-1)),
                             ("negative box_base", EINVAL, dict(box_base=-1)),
                             ("too many lines", ELIMIT, dict(nlines=(1 << 24) + 1)),
                             ("box rows beyond 32 bits", ELIMIT, dict(box_base=2 ** 31 - 5))):
        assert _run(sim, pk, **over) == code, what
        for out in C.OUTPUTS:
            a = getattr(pk, out)
            assert (a == (C.POISON8 if a.dtype == np.uint8 else C.POISON32)).all(), what
    assert _run(sim, pk, nprob=0) == 0 and (pk.status == C.POISON32).all() and (pk.omitted == C.POISON32).all()
    assert _run(sim, pk) == 0
    C.compare(pk)
