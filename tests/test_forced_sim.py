"""The forced-alignment kernel without a GPU: tests/native/sim_forced.cpp compiles csrc/ta_forced.hip ITSELF for the host
(a wave = 64 coroutines that meet at every DPP move, ballot and hand-over of LDS; tests/native/hipshim and
sim_forced_shim.h) and every integer it writes must equal the checker tests/forced_ref.py -- the cases of
tests/forced_cases.py, which tests/test_forced_gpu.py drives through the real kernel."""
import numpy as np
import pytest

import forced_cases as C
import forced_ref as R
import simlib


@pytest.fixture(scope="module")
def sim():
    return C.bind(simlib.load("forced", [simlib.CSRC + "ta_forced.hip"] + C.SIM_DEPS, include=["hipshim"]))


def _run(lib, pk, **over):
    return C.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, **over)


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_host_build_of_the_kernel_equals_the_checker(sim, case):
    name, no, lines = case
    pk = C.pack(sim, lines, no)
    assert _run(sim, pk) == 0
    frames, score = C.want(name, lines)
    assert pk.status.tolist() == [R.OK] * len(lines)
    assert np.array_equal(C.gather(pk, pk.frames), frames)
    assert np.array_equal(pk.score, score)


def test_workspace_bytes(sim):
    f = sim.ta_forced_workspace_bytes
    assert f(3, 1) == 256 and f(8, 1) == 256 and f(9, 1) == 512           # K = 2: eight steps per word
    assert f(129, 64) == 256 * 33 and f(2047, 1023) == 256 * 2 * 2047      # K = 4: four per word; K = 32: two words per step
    for T, L in ((0, 1), (2, 1), (5, 0), (5001, 5), (4000, 1024), (-1, -1)):
        assert f(T, L) == -1


def test_a_line_refused_through_its_data_leaves_its_neighbours_alone(sim):
    rng = np.random.default_rng(5)
    lines = [(C.probs(rng, 30, 6), C.text(rng, 7, 6)), (C.probs(rng, 21, 6), C.text(rng, 5, 6)),
             (C.probs(rng, 140, 6), C.text(rng, 66, 6))]
    frames, score = R.align_batch(lines)
    keep = np.r_[0:7, 12:78]
    for edit, status in ((dict(labels_edit={1: (2, 6)}), R.LABEL), (dict(labels_edit={1: (0, 0)}), R.LABEL),
                         (dict(L_dev={1: 11}), R.BOUNDS),        # 2 L + 1 = 23 > T on the device alone
                         (dict(L_dev={1: 0}), R.BOUNDS)):
        pk = C.pack(sim, lines, 6, **edit)
        assert _run(sim, pk) == 0
        assert pk.status.tolist() == [R.OK, status, R.OK]
        got = C.gather(pk, pk.frames)
        assert np.array_equal(got[keep], frames[keep]) and (got[7:12] == C.POISON32).all()
        assert pk.score[1] == C.POISON64 and np.array_equal(pk.score[[0, 2]], score[[0, 2]])
    # the device's L asks for a variant that the host's copies did not launch: refused, not left without a status
    pk = C.pack(sim, lines[:2], 6, L_dev={1: 5})
    pk.T[1], pk.L[1] = 21, 5
    pk2 = C.pack(sim, [lines[2], lines[0]], 6, L_dev={1: 7})
    assert _run(sim, pk2, L_host=np.asarray([66, 7], np.int32)) == 0 and pk2.status.tolist() == [R.OK, R.OK]
    big = (C.probs(rng, 140, 6), C.text(rng, 66, 6))
    pk3 = C.pack(sim, [lines[0], big], 6)
    pk3.L_host[1] = 60                                   # the host's copy says K = 2, the device's L = 66 needs K = 4
    assert _run(sim, pk3) == 0 and pk3.status.tolist() == [R.OK, R.BOUNDS]
    # offsets outside the arrays: nothing is read through them
    for name, k, v in (("row_off", 0, -3), ("row_off", 2, 10 ** 9), ("lab_off", 1, -1), ("lab_off", 1, 10 ** 9),
                       ("ws_off", 0, 8), ("ws_off", 2, 10 ** 12), ("ws_off", 1, -16)):
        pk = C.pack(sim, lines, 6)
        getattr(pk, name)[k] = v
        assert _run(sim, pk) == 0
        want = [R.OK] * 3
        want[k] = R.BOUNDS
        assert pk.status.tolist() == want, (name, v)


def test_host_side_refusals_touch_nothing(sim):
    rng = np.random.default_rng(6)
    lines = [(C.probs(rng, 30, 6), C.text(rng, 7, 6)), (C.probs(rng, 21, 6), C.text(rng, 5, 6))]
    pk = C.pack(sim, lines, 6)
    for what, code, over in C.refusals(pk):
        if over == "misalign":
            over = dict(workspace=pk.ws.ctypes.data + 4)
        assert _run(sim, pk, **over) == code, what
        assert (pk.frames == C.POISON32).all() and (pk.score == C.POISON64).all() and (pk.status == C.POISON32).all(), what
        assert (pk.ws == C.POISON_BYTE).all(), what
    assert _run(sim, pk, nlines=0) == 0 and (pk.status == C.POISON32).all()
    assert _run(sim, pk) == 0 and pk.status.tolist() == [0, 0]
    assert np.array_equal(C.gather(pk, pk.frames), R.align_batch(lines)[0])
