"""The confidence kernel of the lattice with omission without a GPU: tests/native/sim_forced_omit_conf.cpp compiles
csrc/ta_forced_omit_conf.hip ITSELF for the host (a wave = 64 coroutines that meet at every DPP move, lane read, ballot
and hand-over of LDS; tests/native/hipshim, sim_forced_shim.h and sim_forced_omit_conf_shim.h, which states what each DPP
control of the two max-scans does) and every integer it writes must equal the checker tests/forced_omit_conf_ref.py -- the
cases of tests/forced_omit_conf_cases.py, which tests/test_forced_omit_conf_gpu.py drives through the real kernel."""
import os
import subprocess

import numpy as np
import pytest

import forced_cases as C0
import forced_omit_conf_cases as C
import forced_omit_conf_ref as R
import forced_ref as R0
import simlib
from conftest import REPO

DEPS = [simlib.NAT + "sim_forced_omit_conf_shim.h", simlib.CSRC + "ta_forced_omit_conf.hip"] + C0.SIM_DEPS


@pytest.fixture(scope="module")
def sim():
    return C.bind(simlib.load("forced_omit_conf", DEPS, include=["hipshim"]))


def _run(lib, pk, omit, **over):
    return C.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, omit, **over)


def _untouched(pk):
    return ((pk.confidence == C.POISON64).all() and (pk.rival == C.POISON32).all() and (pk.status == C.POISON32).all() and
            (pk.ws == C.POISON_BYTE).all())


@pytest.mark.parametrize("which", C.SETS)
@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_host_build_of_the_kernel_equals_the_checker(sim, case, which):
    name, no, omit, lines = case
    qs, conf, rival = C.want(name, lines, omit)[which]
    pk = C.pack(sim, lines, no, qs)
    assert _run(sim, pk, omit) == 0
    assert pk.status.tolist() == [R0.OK] * len(lines)
    assert np.array_equal(C.gather(pk, pk.confidence, C.POISON64), conf)
    assert np.array_equal(C.gather(pk, pk.rival, C.POISON32), rival)
    assert (pk.ws[~C.pieces(sim, pk)] == C.POISON_BYTE).all()    # the workspace outside every line's piece stays poison


def test_the_cases_hold_what_they_are_there_for():
    """the absent-run cases hold omitted and present characters at their price of 4 bits; the seeded set holds every query
    count, and the prices and the chunk edges are all there"""
    kinds, names = set(), set()
    n_absent = 0
    for name, no, omit, lines in C.cases():
        names.add(name)
        kinds |= {C.nq_kind(name, k) for k in range(len(lines))}
        if name.startswith(C.ABSENT_AT_4_BITS):
            assert omit == 4 * C.UNIT
            n_absent += 1
            for f in C.line_frames(name, lines, omit):
                assert (f[:, 0] < 0).any() and (f[:, 0] >= 0).any(), name
    assert n_absent >= 10 and kinds == set(C.NQ_KINDS)
    assert {"price %d" % o for o in C.OMITS} | {"price %d constant" % o for o in C.OMITS} | {"chunk edges", "variant L=1023"} <= names
    assert {len(P) for P, _ in dict((c[0], c[3]) for c in C.cases())["chunk edges"]} == {7, 8, 9, 15, 16, 17, 23, 24}


def test_workspace_bytes(sim):
    f = sim.ta_forced_omit_confidence_workspace_bytes
    # a forward row of 64 K int64 per query: 512 K nq bytes
    assert f(3, 1, 0) == 0 and f(3, 1, 1) == 1024 and f(3, 1, 2) == 2048 and f(5000, 1, 2) == 2048
    assert f(127, 63, 126) == 1024 * 126 and f(129, 64, 128) == 2048 * 128 and f(129, 64, 1) == 2048
    assert f(255, 127, 5) == 2048 * 5 and f(257, 128, 256) == 4096 * 256 and f(1025, 512, 7) == 16384 * 7
    assert f(511, 255, 3) == 4096 * 3 and f(513, 256, 3) == 8192 * 3 and f(1023, 511, 3) == 8192 * 3
    assert f(2047, 1023, 2046) == 16384 * 2046
    for T, L, nq in ((0, 1, 0), (2, 1, 1), (5, 0, 0), (5001, 5, 1), (4000, 1024, 1), (-1, -1, -1), (9, 3, -1), (9, 3, 7),
                     (2047, 1023, 2047)):
        assert f(T, L, nq) == -1


def test_a_line_refused_through_its_data_leaves_its_neighbours_alone(sim):
    rng = np.random.default_rng(5)
    omit = 3 * C.UNIT
    lines = C.three(rng)
    qs = C.three_queries(rng, lines)
    want = [R.query_list(R.tables_closed(P, cs, omit)[2], *q) for (P, cs), q in zip(lines, qs)]
    conf, rival = np.concatenate([c for c, _ in want]), np.concatenate([r for _, r in want])
    a, b = len(qs[0][0]), len(qs[0][0]) + len(qs[1][0])

    def check(pk, status, mine=None):
        assert _run(sim, pk, omit) == 0
        assert pk.status.tolist() == [R0.OK, status, R0.OK]
        n1 = int(pk.nq_host[1])
        for got, want, poison in ((pk.confidence, conf, C.POISON64), (pk.rival, rival, C.POISON32)):
            got = C.gather(pk, got, poison)
            assert np.array_equal(got[:a], want[:a]) and np.array_equal(got[a + n1:], want[b:]) and (got[a:a + n1] == poison).all()
        o = int(pk.ws_off[1])                            # the refused line's piece stays poison too
        assert (pk.ws[o:o + 1024 * n1] == C.POISON_BYTE).all()
    for edit, status in ((dict(labels_edit={1: (2, 6)}), R0.LABEL), (dict(labels_edit={1: (0, 0)}), R0.LABEL),
                         (dict(L_dev={1: 11}), R0.BOUNDS),       # 2 L + 1 = 23 > T on the device alone
                         (dict(L_dev={1: 0}), R0.BOUNDS),
                         (dict(nq_dev={1: -1}), R.QUERY), (dict(nq_dev={1: 11}), R.QUERY), (dict(nq_dev={1: 1 << 30}), R.QUERY),
                         (dict(nq_dev={1: 10}), R.QUERY)):        # within 0 .. 2 L: the queries behind its own are the gap's -7
        check(C.pack(sim, lines, 6, qs, **edit), status)
    # a frame that leaves 0 .. T - 1, frames that decrease, a character that leaves 0 .. L - 1: TA_FORCED_QUERY
    good_c = qs[1][0]
    for frames, chars in (([-1, 3, 9, 9, 20], good_c), ([0, 3, 9, 9, 21], good_c), ([0, 3, 5000, 5000, 5000], good_c),
                          ([0, 3, 9, 8, 20], good_c), ([5, 4, 10, 10, 20], good_c), ([20, 20, 20, 20, 0], good_c),
                          (qs[1][1], [0, 1, 5, 2, 3]), (qs[1][1], [-1, 1, 4, 2, 3]), (qs[1][1], [0, 1, 4, 2, 1 << 20])):
        mine = (np.asarray(chars, np.int32), np.asarray(frames, np.int32))
        check(C.pack(sim, lines, 6, [qs[0], mine, qs[2]]), R.QUERY)
    equal = list(qs)
    equal[1] = (np.asarray([4, 4, 0, 4, 2], np.int32), np.full(5, 10, np.int32))   # equal frames, a character three times
    pk = C.pack(sim, lines, 6, equal)
    assert _run(sim, pk, omit) == 0 and pk.status.tolist() == [0, 0, 0]
    assert np.array_equal(C.gather(pk, pk.confidence, C.POISON64)[a:b],
                          R.query_list(R.tables_closed(lines[1][0], lines[1][1], omit)[2], *equal[1])[0])
    # the device's L asks for a variant that the host's copies did not launch: refused, not left without a status
    pk3 = C.pack(sim, [lines[0], lines[2]], 6, [qs[0], qs[2]])
    pk3.L_host[1] = 60                                   # the host's copy says K = 2, the device's L = 66 needs K = 4
    assert _run(sim, pk3, omit) == 0 and pk3.status.tolist() == [R0.OK, R0.BOUNDS]
    # offsets outside the arrays: nothing is read through them
    for name, k, v in (("row_off", 0, -3), ("row_off", 2, 10 ** 9), ("lab_off", 1, -1), ("lab_off", 1, 10 ** 9),
                       ("ws_off", 0, 8), ("ws_off", 2, 10 ** 12), ("ws_off", 1, -16), ("q_off", 0, -1), ("q_off", 2, 10 ** 12),
                       ("q_off", 1, 10 ** 9)):
        pk = C.pack(sim, lines, 6, qs)
        getattr(pk, name)[k] = v
        assert _run(sim, pk, omit) == 0
        want = [R0.OK] * 3
        want[k] = R0.BOUNDS
        assert pk.status.tolist() == want, (name, v)


def test_host_side_refusals_touch_nothing(sim):
    rng = np.random.default_rng(6)
    omit = 2 * C.UNIT
    lines = C.three(rng)[:2]
    qs = C.three_queries(rng, lines)
    pk = C.pack(sim, lines, 6, qs)
    for what, code, over in C.refusals(pk):
        if over == "misalign":
            over = dict(workspace=pk.ws.ctypes.data + 4)
        assert _run(sim, pk, omit, **over) == code, what
        assert _untouched(pk), what
    assert _run(sim, pk, omit, nlines=0) == 0 and _untouched(pk)
    assert _run(sim, pk, omit) == 0 and pk.status.tolist() == [0, 0]
    want = [R.query_list(R.tables_closed(P, cs, omit)[2], *q) for (P, cs), q in zip(lines, qs)]
    assert np.array_equal(C.gather(pk, pk.confidence, C.POISON64), np.concatenate([c for c, _ in want]))
    assert np.array_equal(C.gather(pk, pk.rival, C.POISON32), np.concatenate([r for _, r in want]))


def test_stand_alone_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the new entry's host build as a program with its own main, every variant K once, under the host sanitizers"""
    exe = str(tmp_path / "sim_forced_omit_conf_main")
    native = os.path.join(REPO, simlib.NAT)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DSIM_FORCED_OMIT_CONF_MAIN", "-I", os.path.join(native, "hipshim"), "-o", exe,
                           os.path.join(native, "sim_forced_omit_conf.cpp")])
    got = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert got.returncode == 0, got.stdout + got.stderr
    assert "confidence of the first queries" in got.stdout and "ERROR" not in got.stderr
