"""ta_forced_align_omit_lines without a GPU: the host build of csrc/ta_forced_omit.hip (tests/native/sim_forced_omit.cpp,
as tests/test_forced_omit_sim.py makes it -- it includes the .hip itself, so it exports the slot entry as well) run through
the entry whose line list lies "on the device" -- EVERY case of tests/forced_omit_cases.py in the layout of
tests/forced_omit_lines_cases.py -- and every integer held against tests/forced_omit_ref.py."""
import numpy as np
import pytest

import forced_cases as C0
import forced_omit_cases as OC
import forced_omit_lines_cases as LC
import forced_omit_ref as R
import forced_ref as R0
import simlib

UNIT = OC.UNIT


@pytest.fixture(scope="module")
def sim():
    deps = [simlib.NAT + "sim_forced_omit_shim.h", simlib.CSRC + "ta_forced_omit.hip"] + C0.SIM_DEPS
    return LC.bind(simlib.load("forced_omit", deps, include=["hipshim"]))


def _run(lib, pk, omit, **over):
    return LC.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, omit, **over)


@pytest.mark.parametrize("case", OC.cases(), ids=lambda c: c[0])
def test_the_indexed_entry_equals_the_checker(sim, case):
    """acc_line a permutation with holes, caps equal to and above L, slots behind count"""
    name, no, omit, lines = case
    pk = LC.pack(sim, lines, no, seed=len(name))
    assert _run(sim, pk, omit) == 0
    frames, score = OC.want(name, lines, omit)
    n = len(lines)
    assert pk.status[:n].tolist() == [R0.OK] * n
    assert (pk.status[n:] == LC.POISON32).all() and (pk.score[n:] == LC.POISON64).all()
    assert np.array_equal(C0.gather(pk, pk.frames), frames)
    assert np.array_equal(pk.score[:n], score)
    if name == OC.STRICT:
        strict_frames, strict_score = R0.align_batch(lines)
        assert np.array_equal(frames, strict_frames) and np.array_equal(score, strict_score)


def _three(rng):
    return [(C0.probs(rng, 30, 6), C0.text(rng, 7, 6)), (C0.probs(rng, 21, 6), C0.text(rng, 5, 6)),
            (C0.probs(rng, 140, 6), C0.text(rng, 66, 6))]


def test_a_slot_refused_through_its_data_leaves_its_neighbours_alone(sim):
    rng = np.random.default_rng(15)
    omit = 2 * UNIT
    lines = _three(rng)
    frames, score = R.align_batch(lines, omit)
    keep = np.r_[0:7, 12:78]

    def check(pk, status, ran=False):
        assert ran or _run(sim, pk, omit) == 0
        assert pk.status[:3].tolist() == [R0.OK, status, R0.OK]
        got = C0.gather(pk, pk.frames)
        assert np.array_equal(got[keep], frames[keep]) and (got[7:12] == LC.POISON32).all()
        assert pk.score[1] == LC.POISON64 and np.array_equal(pk.score[[0, 2]], score[[0, 2]])
    # the device's L = 5 over a cap of 4: the text would fit its line (2 L + 1 = 11 <= 21) and its workspace piece
    check(LC.pack(sim, lines, 6, cap_edit={1: 4}), R0.BOUNDS)
    # a cap above L that the device's L still exceeds
    check(LC.pack(sim, lines, 6, cap_edit={1: 8}, L_dev={1: 9}), R0.BOUNDS)
    check(LC.pack(sim, lines, 6, L_dev={1: 0}), R0.BOUNDS)
    check(LC.pack(sim, lines, 6, labels_edit={1: (2, 6)}), R0.LABEL)
    check(LC.pack(sim, lines, 6, labels_edit={1: (0, 0)}), R0.LABEL)
    # a cap above L that the device's L stays within: aligned (the checker's answer for the shorter text)
    pk = LC.pack(sim, lines, 6, cap_edit={1: 8}, L_dev={1: 4})
    assert _run(sim, pk, omit) == 0 and pk.status[:3].tolist() == [R0.OK] * 3
    _, fr, _ = R.align_closed(lines[1][0], lines[1][1][:4], omit)
    o = int(pk.lab_off[1])
    assert np.array_equal(pk.frames[o:o + 4], fr) and (pk.frames[o + 4] == LC.POISON32).all()
    # acc_line outside the chunk's lines, offsets outside their arrays: nothing is read through them
    for name, k, v in (("acc_line", 1, -1), ("acc_line", 1, 6), ("acc_line", 1, 1 << 30), ("lab_off", 1, -1),
                       ("lab_off", 1, 10 ** 9)):
        pk = LC.pack(sim, lines, 6)
        assert pk.nlines_all == 6
        was = getattr(pk, name)[k]
        getattr(pk, name)[k] = v
        assert _run(sim, pk, omit) == 0
        getattr(pk, name)[k] = was                       # gather looks the lines' rows up where they were
        check(pk, R0.BOUNDS, ran=True)
    for name, v in (("row_off_all", -3), ("row_off_all", 10 ** 9), ("ws_off_all", 8), ("ws_off_all", 10 ** 12), ("ws_off_all", -16)):
        pk = LC.pack(sim, lines, 6)
        getattr(pk, name)[pk.slot_line[1]] = v
        check(pk, R0.BOUNDS)


def test_count_limits_the_slots_and_a_negative_count_touches_nothing(sim):
    rng = np.random.default_rng(16)
    omit = 2 * UNIT
    lines = _three(rng)
    frames, score = R.align_batch(lines, omit)
    pk = LC.pack(sim, lines, 6, count=2)                 # three slots given, two filled
    assert _run(sim, pk, omit) == 0
    assert pk.status[:2].tolist() == [R0.OK, R0.OK] and (pk.status[2:] == LC.POISON32).all()
    got = C0.gather(pk, pk.frames)
    assert np.array_equal(got[:12], frames[:12]) and (got[12:] == LC.POISON32).all()
    assert np.array_equal(pk.score[:2], score[:2]) and (pk.score[2:] == LC.POISON64).all()
    pk = LC.pack(sim, lines, 6, count=0)
    assert _run(sim, pk, omit) == 0 and LC.untouched(pk)
    for count in (-1, -(1 << 40)):
        pk = LC.pack(sim, lines, 6, count=count)
        assert _run(sim, pk, omit) == 0 and LC.untouched(pk)
    pk = LC.pack(sim, lines, 6, count=1 << 40)           # more than the slots the call covers: the covered ones run
    pk.acc_line[3:], pk.L[3:], pk.lab_off[3:] = -1, 1, 0
    assert _run(sim, pk, omit) == 0 and pk.status.tolist() == [R0.OK] * 3 + [R0.BOUNDS] * 2


def test_host_side_refusals_touch_nothing(sim):
    rng = np.random.default_rng(17)
    omit = 2 * UNIT
    lines = _three(rng)[:2]
    pk = LC.pack(sim, lines, 6)
    for what, code, over in LC.refusals(pk):
        if over == "misalign":
            over = dict(workspace=pk.ws.ctypes.data + 4)
        assert _run(sim, pk, omit, **over) == code, what
        assert LC.untouched(pk), what
    assert _run(sim, pk, omit, nslots=0) == 0 and LC.untouched(pk)
    assert _run(sim, pk, omit, nlines_all=0, nslots=0) == 0 and LC.untouched(pk)
    # no line can receive a text: nothing to launch
    assert _run(sim, pk, omit, Lcap_host=np.zeros(pk.nlines_all, np.int32)) == 0 and LC.untouched(pk)
    # the device's omit price is the host's argument: the kernel holds it to its range as well, and the good call runs
    assert _run(sim, pk, omit) == 0 and pk.status[:2].tolist() == [0, 0]
    assert np.array_equal(C0.gather(pk, pk.frames), R.align_batch(lines, omit)[0])


def test_workspace_bytes_never_decrease_with_the_text(sim):
    """a line's piece is sized by its cap: it must hold every shorter text, across the variants' boundaries as well"""
    f = sim.ta_forced_omit_workspace_bytes
    edges = sorted({L for _, lmax, lnext in C0.EDGES for L in (lmax, lnext) if L is not None})
    for T in (3, 9, 127, 129, 257, 1025, 2047, 2048, 2049, 4999, 5000):
        got = [f(T, L) for L in range(1, min((T - 1) // 2, R0.MAX_TARGET) + 1)]
        assert min(got) > 0 and all(a <= b for a, b in zip(got, got[1:])), T
    for L in edges:                                      # right at a boundary, at the shortest line that takes the text
        for T in (2 * L + 1, 2 * L + 3, 5000):
            assert 0 < f(T, L - 1) <= f(T, L) and (L == R0.MAX_TARGET or f(max(T, 2 * L + 3), L) <= f(max(T, 2 * L + 3), L + 1))
