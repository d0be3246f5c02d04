"""The omission-tolerant forced-alignment kernel without a GPU: tests/native/sim_forced_omit.cpp compiles
csrc/ta_forced_omit.hip ITSELF for the host (a wave = 64 coroutines that meet at every DPP move, ballot and hand-over of
LDS; tests/native/hipshim, sim_forced_shim.h and sim_forced_omit_shim.h, which states the DPP controls of the max-scan)
and every integer it writes must equal the checker tests/forced_omit_ref.py -- the cases of tests/forced_omit_cases.py,
which tests/test_forced_omit_gpu.py drives through the real kernel."""
import numpy as np
import pytest

import forced_cases as C0
import forced_omit_cases as C
import forced_omit_ref as R
import forced_ref as R0
import simlib

UNIT = C.UNIT


@pytest.fixture(scope="module")
def sim():
    deps = [simlib.NAT + "sim_forced_omit_shim.h", simlib.CSRC + "ta_forced_omit.hip"] + C0.SIM_DEPS
    return C.bind(simlib.load("forced_omit", deps, include=["hipshim"]))


def _run(lib, pk, omit, **over):
    return C.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, omit, **over)


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_host_build_of_the_kernel_equals_the_checker(sim, case):
    name, no, omit, lines = case
    pk = C.pack(sim, lines, no)
    assert _run(sim, pk, omit) == 0
    frames, score = C.want(name, lines, omit)
    assert pk.status.tolist() == [R0.OK] * len(lines)
    assert np.array_equal(C.gather(pk, pk.frames), frames)
    assert np.array_equal(pk.score, score)
    if name == C.STRICT:
        strict_frames, strict_score = R0.align_batch(lines)
        assert np.array_equal(frames, strict_frames) and np.array_equal(score, strict_score)


def test_the_absent_runs_are_what_the_path_omits():
    """the far-move cases do what they were built for: the checker's path leaves out the absent run and nothing else"""
    cases = dict((c[0], c) for c in C.cases())
    for name, at, run in (("absent run 70", 4, 70), ("absent run 200", 6, 200), ("absent run 600", 3, 600)):
        _, _, omit, lines = cases[name]
        frames, _ = C.want(name, lines, omit)
        gone = np.flatnonzero(frames[:, 0] == R.OMITTED)
        assert set(range(at, at + run)) <= set(gone.tolist()) and len(gone) <= run + 4, name
        assert (frames[gone] == R.OMITTED).all()
        path = R.align_closed(lines[0][0], lines[0][1], omit)[2]
        assert np.diff(path).max() >= 2 * run, name      # ONE far move over the whole run: across many lanes
    _, _, omit, lines = cases["far between equal labels"]
    frames, _ = C.want("far between equal labels", lines, omit)
    assert (frames.reshape(len(lines), 3, 3)[:, 1] == R.OMITTED).all() and (frames.reshape(len(lines), 3, 3)[:, ::2] >= 0).all()


def test_workspace_bytes(sim):
    f = sim.ta_forced_omit_workspace_bytes
    # the moves as ta_forced_align's, then a bit per state and timestep: 32 / K steps per word and lane
    assert f(3, 1) == 512 and f(8, 1) == 512 and f(9, 1) == 768 and f(16, 1) == 768 and f(17, 1) == 256 * 5
    assert f(129, 64) == 256 * (33 + 17) and f(2047, 1023) == 256 * 3 * 2047
    for T, L in ((0, 1), (2, 1), (5, 0), (5001, 5), (4000, 1024), (-1, -1)):
        assert f(T, L) == -1
    for T in (2047, 3000, 5000):                         # never decreasing in L
        sizes = [f(T, L) for L in range(1, min((T - 1) // 2, 1023) + 1)]
        assert all(b % 256 == 0 and b > 0 for b in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))


def test_a_line_refused_through_its_data_leaves_its_neighbours_alone(sim):
    rng = np.random.default_rng(5)
    omit = 2 * UNIT
    lines = [(C0.probs(rng, 30, 6), C0.text(rng, 7, 6)), (C0.probs(rng, 21, 6), C0.text(rng, 5, 6)),
             (C0.probs(rng, 140, 6), C0.text(rng, 66, 6))]
    frames, score = R.align_batch(lines, omit)
    keep = np.r_[0:7, 12:78]
    for edit, status in ((dict(labels_edit={1: (2, 6)}), R0.LABEL), (dict(labels_edit={1: (0, 0)}), R0.LABEL),
                         (dict(L_dev={1: 11}), R0.BOUNDS),       # 2 L + 1 = 23 > T on the device alone
                         (dict(L_dev={1: 0}), R0.BOUNDS)):
        pk = C.pack(sim, lines, 6, **edit)
        assert _run(sim, pk, omit) == 0
        assert pk.status.tolist() == [R0.OK, status, R0.OK]
        got = C.gather(pk, pk.frames)
        assert np.array_equal(got[keep], frames[keep]) and (got[7:12] == C.POISON32).all()
        assert pk.score[1] == C.POISON64 and np.array_equal(pk.score[[0, 2]], score[[0, 2]])
    # the device's L asks for a variant that the host's copies did not launch: refused, not left without a status
    big = (C0.probs(rng, 140, 6), C0.text(rng, 66, 6))
    pk3 = C.pack(sim, [lines[0], big], 6)
    pk3.L_host[1] = 60                                   # the host's copy says K = 2, the device's L = 66 needs K = 4
    assert _run(sim, pk3, omit) == 0 and pk3.status.tolist() == [R0.OK, R0.BOUNDS]
    # offsets outside the arrays: nothing is read through them
    for name, k, v in (("row_off", 0, -3), ("row_off", 2, 10 ** 9), ("lab_off", 1, -1), ("lab_off", 1, 10 ** 9),
                       ("ws_off", 0, 8), ("ws_off", 2, 10 ** 12), ("ws_off", 1, -16)):
        pk = C.pack(sim, lines, 6)
        getattr(pk, name)[k] = v
        assert _run(sim, pk, omit) == 0
        want = [R0.OK] * 3
        want[k] = R0.BOUNDS
        assert pk.status.tolist() == want, (name, v)


def test_host_side_refusals_touch_nothing(sim):
    rng = np.random.default_rng(6)
    omit = 2 * UNIT
    lines = [(C0.probs(rng, 30, 6), C0.text(rng, 7, 6)), (C0.probs(rng, 21, 6), C0.text(rng, 5, 6))]
    pk = C.pack(sim, lines, 6)
    for what, code, over in C.refusals(pk):
        if over == "misalign":
            over = dict(workspace=pk.ws.ctypes.data + 4)
        assert _run(sim, pk, omit, **over) == code, what
        assert (pk.frames == C.POISON32).all() and (pk.score == C.POISON64).all() and (pk.status == C.POISON32).all(), what
        assert (pk.ws == C.POISON_BYTE).all(), what
    assert _run(sim, pk, omit, nlines=0) == 0 and (pk.status == C.POISON32).all()
    assert _run(sim, pk, omit) == 0 and pk.status.tolist() == [0, 0]
    assert np.array_equal(C.gather(pk, pk.frames), R.align_batch(lines, omit)[0])
