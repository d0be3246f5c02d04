"""ta_forced_align_lines without a GPU: the host build of csrc/ta_forced.hip (tests/native/sim_forced.cpp, as
tests/test_forced_sim.py makes it) run through the entry whose line list lies "on the device" -- the cases of
tests/forced_cases.py in the layout of tests/forced_lines_cases.py -- and every integer held against tests/forced_ref.py."""
import numpy as np
import pytest

import forced_cases as C
import forced_lines_cases as LC
import forced_ref as R
import simlib


@pytest.fixture(scope="module")
def sim():
    return LC.bind(simlib.load("forced", [simlib.CSRC + "ta_forced.hip"] + C.SIM_DEPS, include=["hipshim"]))


def _run(lib, pk, **over):
    return LC.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, **over)


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_the_indexed_entry_equals_the_checker(sim, case):
    """acc_line a permutation with holes, caps equal to and above L, slots behind count -- and in the variant cases lines
    that need two different K in one call (each holds the largest text of its K and the smallest of the next)"""
    name, no, lines = case
    pk = LC.pack(sim, lines, no, seed=len(name))
    assert _run(sim, pk) == 0
    frames, score = C.want(name, lines)
    n = len(lines)
    assert pk.status[:n].tolist() == [R.OK] * n
    assert (pk.status[n:] == LC.POISON32).all() and (pk.score[n:] == LC.POISON64).all()
    assert np.array_equal(C.gather(pk, pk.frames), frames)
    assert np.array_equal(pk.score[:n], score)


def _three(rng):
    return [(C.probs(rng, 30, 6), C.text(rng, 7, 6)), (C.probs(rng, 21, 6), C.text(rng, 5, 6)),
            (C.probs(rng, 140, 6), C.text(rng, 66, 6))]


def test_a_slot_refused_through_its_data_leaves_its_neighbours_alone(sim):
    rng = np.random.default_rng(15)
    lines = _three(rng)
    frames, score = R.align_batch(lines)
    keep = np.r_[0:7, 12:78]

    def check(pk, status, ran=False):
        assert ran or _run(sim, pk) == 0
        assert pk.status[:3].tolist() == [R.OK, status, R.OK]
        got = C.gather(pk, pk.frames)
        assert np.array_equal(got[keep], frames[keep]) and (got[7:12] == LC.POISON32).all()
        assert pk.score[1] == LC.POISON64 and np.array_equal(pk.score[[0, 2]], score[[0, 2]])
    # the device's L = 5 over a cap of 4: the text would fit its line (2 L + 1 = 11 <= 21) and its workspace piece
    check(LC.pack(sim, lines, 6, cap_edit={1: 4}), R.BOUNDS)
    # a cap above L that the device's L still exceeds
    check(LC.pack(sim, lines, 6, cap_edit={1: 8}, L_dev={1: 9}), R.BOUNDS)
    check(LC.pack(sim, lines, 6, L_dev={1: 0}), R.BOUNDS)
    check(LC.pack(sim, lines, 6, labels_edit={1: (2, 6)}), R.LABEL)
    # a cap above L that the device's L stays within: aligned (the checker's answer for the shorter text)
    pk = LC.pack(sim, lines, 6, cap_edit={1: 8}, L_dev={1: 4})
    assert _run(sim, pk) == 0 and pk.status[:3].tolist() == [R.OK] * 3
    _, fr, _ = R.align(lines[1][0], lines[1][1][:4])
    o = int(pk.lab_off[1])
    assert np.array_equal(pk.frames[o:o + 4], fr) and (pk.frames[o + 4] == LC.POISON32).all()
    # acc_line outside the chunk's lines, offsets outside their arrays: nothing is read through them
    for name, k, v in (("acc_line", 1, -1), ("acc_line", 1, 6), ("acc_line", 1, 1 << 30), ("lab_off", 1, -1),
                       ("lab_off", 1, 10 ** 9)):
        pk = LC.pack(sim, lines, 6)
        assert pk.nlines_all == 6
        was = getattr(pk, name)[k]
        getattr(pk, name)[k] = v
        assert _run(sim, pk) == 0
        getattr(pk, name)[k] = was                       # gather looks the lines' rows up where they were
        check(pk, R.BOUNDS, ran=True)
    for name, v in (("row_off_all", -3), ("row_off_all", 10 ** 9), ("ws_off_all", 8), ("ws_off_all", 10 ** 12), ("ws_off_all", -16)):
        pk = LC.pack(sim, lines, 6)
        getattr(pk, name)[pk.slot_line[1]] = v
        check(pk, R.BOUNDS)


def test_count_limits_the_slots_and_a_negative_count_touches_nothing(sim):
    rng = np.random.default_rng(16)
    lines = _three(rng)
    frames, score = R.align_batch(lines)
    pk = LC.pack(sim, lines, 6, count=2)                 # three slots given, two filled
    assert _run(sim, pk) == 0
    assert pk.status[:2].tolist() == [R.OK, R.OK] and (pk.status[2:] == LC.POISON32).all()
    got = C.gather(pk, pk.frames)
    assert np.array_equal(got[:12], frames[:12]) and (got[12:] == LC.POISON32).all()
    assert np.array_equal(pk.score[:2], score[:2]) and (pk.score[2:] == LC.POISON64).all()
    pk = LC.pack(sim, lines, 6, count=0)
    assert _run(sim, pk) == 0 and LC.untouched(pk)
    for count in (-1, -(1 << 40)):
        pk = LC.pack(sim, lines, 6, count=count)
        assert _run(sim, pk) == 0 and LC.untouched(pk)
    pk = LC.pack(sim, lines, 6, count=1 << 40)           # more than the slots the call covers: the covered ones run
    pk.acc_line[3:], pk.L[3:], pk.lab_off[3:] = -1, 1, 0
    assert _run(sim, pk) == 0 and pk.status.tolist() == [R.OK] * 3 + [R.BOUNDS] * 2


def test_host_side_refusals_touch_nothing(sim):
    rng = np.random.default_rng(17)
    lines = _three(rng)[:2]
    pk = LC.pack(sim, lines, 6)
    for what, code, over in LC.refusals(pk):
        if over == "misalign":
            over = dict(workspace=pk.ws.ctypes.data + 4)
        assert _run(sim, pk, **over) == code, what
        assert LC.untouched(pk), what
    assert _run(sim, pk, nslots=0) == 0 and LC.untouched(pk)
    assert _run(sim, pk, nlines_all=0, nslots=0) == 0 and LC.untouched(pk)
    # no line can receive a text: nothing to launch
    assert _run(sim, pk, Lcap_host=np.zeros(pk.nlines_all, np.int32)) == 0 and LC.untouched(pk)
    assert _run(sim, pk) == 0 and pk.status[:2].tolist() == [0, 0]
    assert np.array_equal(C.gather(pk, pk.frames), R.align_batch(lines)[0])


def test_workspace_bytes_never_decrease_with_the_text(sim):
    """a line's piece is sized by its cap: it must hold every shorter text, across the variants' boundaries as well"""
    f = sim.ta_forced_workspace_bytes
    edges = sorted({L for _, lmax, lnext in C.EDGES for L in (lmax, lnext) if L is not None})
    for T in (3, 9, 127, 129, 257, 1025, 2047, 2048, 2049, 4999, 5000):
        got = [f(T, L) for L in range(1, min((T - 1) // 2, R.MAX_TARGET) + 1)]
        assert min(got) > 0 and all(a <= b for a, b in zip(got, got[1:])), T
    for L in edges:                                      # right at a boundary, at the shortest line that takes the text
        for T in (2 * L + 1, 2 * L + 3, 5000):
            assert 0 < f(T, L - 1) <= f(T, L) and (L == R.MAX_TARGET or f(max(T, 2 * L + 3), L) <= f(max(T, 2 * L + 3), L + 1))
