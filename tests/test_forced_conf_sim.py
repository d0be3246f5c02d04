"""The confidence kernel without a GPU: tests/native/sim_forced_conf.cpp compiles csrc/ta_forced_conf.hip ITSELF for the
host (a wave = 64 coroutines that meet at every DPP move, ballot and hand-over of LDS; tests/native/hipshim,
sim_forced_shim.h and sim_forced_conf_shim.h, which states the DPP control of the move from the right lane) and every
integer it writes must equal the checker tests/forced_conf_ref.py -- the cases of tests/forced_conf_cases.py, which
tests/test_forced_conf_gpu.py drives through the real kernel."""
import numpy as np
import pytest

import forced_cases as C0
import forced_conf_cases as C
import forced_conf_ref as R
import forced_ref as R0
import simlib


@pytest.fixture(scope="module")
def sim():
    deps = [simlib.NAT + "sim_forced_conf_shim.h", simlib.CSRC + "ta_forced_conf.hip"] + C0.SIM_DEPS
    return C.bind(simlib.load("forced_conf", deps, include=["hipshim"]))


def _run(lib, pk, **over):
    return C.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, **over)


def _untouched(pk):
    return ((pk.confidence == C.POISON64).all() and (pk.rival == C.POISON32).all() and (pk.status == C.POISON32).all() and
            (pk.ws == C.POISON_BYTE).all())


@pytest.mark.parametrize("which", C.SETS)
@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_host_build_of_the_kernel_equals_the_checker(sim, case, which):
    name, no, lines = case
    tqs, conf, rival = C.want(name, lines)[which]
    pk = C.pack(sim, lines, no, tqs)
    assert _run(sim, pk) == 0
    assert pk.status.tolist() == [R0.OK] * len(lines)
    assert np.array_equal(C.gather(pk, pk.confidence, C.POISON64), conf)
    assert np.array_equal(C.gather(pk, pk.rival, C.POISON32), rival)
    piece = np.zeros(pk.ws_bytes, dtype=bool)            # the workspace outside every line's piece stays poison
    for o, t, l in zip(pk.ws_off, pk.T_host, pk.L_host):
        piece[o:o + sim.ta_forced_confidence_workspace_bytes(int(t), int(l))] = True
    assert (pk.ws[~piece] == C.POISON_BYTE).all()


def test_workspace_bytes(sim):
    f = sim.ta_forced_confidence_workspace_bytes
    # a forward row of 64 K int64 per character: 512 K L bytes
    assert f(3, 1) == 1024 and f(5000, 1) == 1024 and f(127, 63) == 1024 * 63 and f(129, 64) == 2048 * 64
    assert f(255, 127) == 2048 * 127 and f(257, 128) == 4096 * 128 and f(1025, 512) == 16384 * 512
    assert f(2047, 1023) == 16384 * 1023
    for T, L in ((0, 1), (2, 1), (5, 0), (5001, 5), (4000, 1024), (-1, -1)):
        assert f(T, L) == -1


def _three(rng):
    return [(C0.probs(rng, 30, 6), C0.text(rng, 7, 6)), (C0.probs(rng, 21, 6), C0.text(rng, 5, 6)),
            (C0.probs(rng, 140, 6), C0.text(rng, 66, 6))]


def test_a_line_refused_through_its_data_leaves_its_neighbours_alone(sim):
    rng = np.random.default_rng(5)
    lines = _three(rng)
    tqs = [C.seeded_queries(rng, len(P), len(cs)) for P, cs in lines]
    conf, rival = R.query_batch(lines, tqs)
    keep = np.r_[0:7, 12:78]

    def check(pk, status):
        assert _run(sim, pk) == 0
        assert pk.status.tolist() == [R0.OK, status, R0.OK]
        for got, want, poison in ((pk.confidence, conf, C.POISON64), (pk.rival, rival, C.POISON32)):
            got = C.gather(pk, got, poison)
            assert np.array_equal(got[keep], want[keep]) and (got[7:12] == poison).all()
    for edit, status in ((dict(labels_edit={1: (2, 6)}), R0.LABEL), (dict(labels_edit={1: (0, 0)}), R0.LABEL),
                         (dict(L_dev={1: 11}), R0.BOUNDS),       # 2 L + 1 = 23 > T on the device alone
                         (dict(L_dev={1: 0}), R0.BOUNDS)):
        check(C.pack(sim, lines, 6, tqs, **edit), status)
    # a query that leaves 0 .. T - 1, and queries that decrease: TA_FORCED_QUERY, nothing else of the line is touched
    for mine in ([-1, 3, 9, 9, 20], [0, 3, 9, 9, 21], [0, 3, 5000, 5000, 5000], [0, 3, 9, 8, 20], [5, 4, 10, 10, 20],
                 [20, 20, 20, 20, 0]):
        pk = C.pack(sim, lines, 6, [tqs[0], np.asarray(mine, np.int32), tqs[2]])
        check(pk, R.QUERY)
        a = int(pk.ws_off[1])
        assert (pk.ws[a:a + sim.ta_forced_confidence_workspace_bytes(21, 5)] == C.POISON_BYTE).all()
    equal = [tq.copy() for tq in tqs]
    equal[1][:] = 10                                     # equal neighbours are allowed
    pk = C.pack(sim, lines, 6, equal)
    assert _run(sim, pk) == 0 and pk.status.tolist() == [0, 0, 0]
    assert np.array_equal(C.gather(pk, pk.confidence, C.POISON64)[7:12], R.query(lines[1][0], lines[1][1], equal[1])[0])
    # the device's L asks for a variant that the host's copies did not launch: refused, not left without a status
    pk3 = C.pack(sim, [lines[0], lines[2]], 6, [tqs[0], tqs[2]])
    pk3.L_host[1] = 60                                   # the host's copy says K = 2, the device's L = 66 needs K = 4
    assert _run(sim, pk3) == 0 and pk3.status.tolist() == [R0.OK, R0.BOUNDS]
    # offsets outside the arrays: nothing is read through them
    for name, k, v in (("row_off", 0, -3), ("row_off", 2, 10 ** 9), ("lab_off", 1, -1), ("lab_off", 1, 10 ** 9),
                       ("ws_off", 0, 8), ("ws_off", 2, 10 ** 12), ("ws_off", 1, -16)):
        pk = C.pack(sim, lines, 6, tqs)
        getattr(pk, name)[k] = v
        assert _run(sim, pk) == 0
        want = [R0.OK] * 3
        want[k] = R0.BOUNDS
        assert pk.status.tolist() == want, (name, v)


def test_host_side_refusals_touch_nothing(sim):
    rng = np.random.default_rng(6)
    lines = _three(rng)[:2]
    tqs = [C.seeded_queries(rng, len(P), len(cs)) for P, cs in lines]
    pk = C.pack(sim, lines, 6, tqs)
    for what, code, over in C0.refusals(pk) + [("null t_query", -1, dict(t_query=None)), ("null rival", -1, dict(rival=None))]:
        if over == "misalign":
            over = dict(workspace=pk.ws.ctypes.data + 4)
        assert _run(sim, pk, **over) == code, what
        assert _untouched(pk), what
    assert _run(sim, pk, nlines=0) == 0 and _untouched(pk)
    assert _run(sim, pk) == 0 and pk.status.tolist() == [0, 0]
    conf, rival = R.query_batch(lines, tqs)
    assert np.array_equal(C.gather(pk, pk.confidence, C.POISON64), conf)
    assert np.array_equal(C.gather(pk, pk.rival, C.POISON32), rival)
