"""The posterior kernel without a GPU: tests/native/sim_forced_post.cpp compiles csrc/ta_forced_post.hip ITSELF for the
host (a wave = 64 coroutines that meet at every DPP move, ballot and hand-over of LDS; tests/native/hipshim,
sim_forced_shim.h and sim_forced_conf_shim.h; -ffp-contract=off as the library's build) and every word it writes must
equal the checker tests/forced_post_ref.py BIT FOR BIT -- the float64 outputs are compared through their int64 view.  The
cases are tests/forced_post_cases.py's, which tests/test_forced_post_gpu.py drives through the real kernel."""
import numpy as np
import pytest

import forced_cases as C0
import forced_post_cases as C
import forced_post_ref as R
import forced_ref as R0
import simlib


@pytest.fixture(scope="module")
def sim():
    deps = [simlib.NAT + "sim_forced_conf_shim.h", simlib.CSRC + "ta_forced_post.hip"] + C0.SIM_DEPS
    return C.bind(simlib.load("forced_post", deps, flags=["-ffp-contract=off"], include=["hipshim"]))


def _run(lib, pk, **over):
    return C.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, **over)


def _got(pk):
    return lambda name: getattr(pk, name)


@pytest.mark.parametrize("which", C.SETS)
@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_host_build_of_the_kernel_equals_the_checker_bit_for_bit(sim, case, which):
    name, no, lines = case
    tqs, wanted = C.want(name, lines)[which]
    pk = C.pack(sim, lines, no, tqs)
    assert _run(sim, pk) == 0
    assert pk.status.tolist() == [R0.OK] * len(lines)
    assert C.differing(pk, _got(pk), wanted) == []
    piece = np.zeros(pk.ws_bytes, dtype=bool)            # the workspace outside every line's piece stays poison
    for o, t, l in zip(pk.ws_off, pk.T_host, pk.L_host):
        piece[o:o + sim.ta_forced_posterior_workspace_bytes(int(t), int(l))] = True
    assert (pk.ws[~piece] == C.POISON_BYTE).all()


def test_workspace_bytes(sim):
    f = sim.ta_forced_posterior_workspace_bytes
    # per character a forward row of 64 K doubles and 64 K int32 exponents: 768 K L bytes
    assert f(3, 1) == 1536 and f(5000, 1) == 1536 and f(127, 63) == 1536 * 63 and f(129, 64) == 3072 * 64
    assert f(255, 127) == 3072 * 127 and f(257, 128) == 6144 * 128 and f(1025, 512) == 24576 * 512
    assert f(2047, 1023) == 24576 * 1023
    for T, L in ((0, 1), (2, 1), (5, 0), (5001, 5), (4000, 1024), (-1, -1)):
        assert f(T, L) == -1
    sizes = [f(5000, L) for L in range(1, 1024)]         # never decreasing in L, rows of 256 bytes
    assert all(a < b for a, b in zip(sizes[:-1], sizes[1:])) and all(s % 256 == 0 for s in sizes)


def _three(rng):
    return [(C0.probs(rng, 30, 6), C0.text(rng, 7, 6)), (C0.probs(rng, 21, 6), C0.text(rng, 5, 6)),
            (C0.probs(rng, 140, 6), C0.text(rng, 66, 6))]


def test_a_line_refused_through_its_data_leaves_its_neighbours_alone(sim):
    rng = np.random.default_rng(5)
    lines = _three(rng)
    tqs = [C.seeded_queries(rng, len(P), len(cs)) for P, cs in lines]
    wanted = R.query_batch(lines, tqs)
    keep = np.r_[0:7, 12:78]

    def check(pk, status):
        assert _run(sim, pk) == 0
        assert pk.status.tolist() == [R0.OK, status, R0.OK]
        for name in C.PER_LABEL:
            got = C.gather(pk, getattr(pk, name))
            assert np.array_equal(got[keep], C.words(wanted[name])[keep]) and (got[7:12] == C.poison_of(got)).all(), name
        for name in C.PER_LINE:
            got = C.words(getattr(pk, name))
            assert np.array_equal(got[[0, 2]], C.words(wanted[name])[[0, 2]]) and got[1] == C.poison_of(got), name
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
        assert (pk.ws[a:a + sim.ta_forced_posterior_workspace_bytes(21, 5)] == C.POISON_BYTE).all()
    same = [tq.copy() for tq in tqs]
    same[1][:] = 10                                      # equal neighbours are allowed
    pk = C.pack(sim, lines, 6, same)
    assert _run(sim, pk) == 0 and pk.status.tolist() == [0, 0, 0]
    assert C.differing(pk, _got(pk), R.query_batch(lines, same)) == []
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
    more = [("null t_query", -1, dict(t_query=None))] + [("null " + n, -1, {n: None}) for n in C.OUTPUTS]
    for what, code, over in C0.refusals(pk) + more:
        if over == "misalign":
            over = dict(workspace=pk.ws.ctypes.data + 4)
        assert _run(sim, pk, **over) == code, what
        assert C.untouched(_got(pk)), what
    assert _run(sim, pk, nlines=0) == 0 and C.untouched(_got(pk))
    assert _run(sim, pk) == 0 and pk.status.tolist() == [0, 0]
    assert C.differing(pk, _got(pk), R.query_batch(lines, tqs)) == []
