"""The span fill without a GPU: tests/native/sim_span.cpp replays the kernel's strips, lanes, skewed steps, hand-off row
and reductions on the host with the SAME nw_span.h the kernel compiles (carrier, cell, free column-0 boundary, lane step,
last-column maximum), and every result must equal the checker tests/span_ref.py -- the shapes of tests/test_span_gpu.py,
scaled to what the simulator runs in seconds."""
import ctypes

import numpy as np
import pytest

import span_cases as C
import span_ref as R
import simlib


@pytest.fixture(scope="module")
def sim():
    lib = simlib.load("span", [simlib.CSRC + "nw_span.h", simlib.CSRC + "nw_cell.h"])
    lib.sim_span.restype = ctypes.c_int
    lib.sim_span.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                             ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.sim_span_roundtrip.restype = ctypes.c_int
    lib.sim_span_roundtrip.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def _sim(lib, t, o, system, R_=4, W=1):
    t = np.ascontiguousarray(t, dtype=np.int32)
    o = np.ascontiguousarray(o, dtype=np.int32)
    p = np.ascontiguousarray(system, dtype=np.int32)
    out = np.full(3, -77, dtype=np.int32)
    tt = np.concatenate([t, [9999]]).astype(np.int32)      # never empty buffers
    oo = np.concatenate([o, [9998]]).astype(np.int32)
    assert lib.sim_span(tt.ctypes.data, len(t), oo.ctypes.data, len(o), p.ctypes.data, R_, W, out.ctypes.data) == 0
    return tuple(int(v) for v in out)


def test_carrier_is_exact_at_the_ends_of_its_fields(sim):
    out = np.zeros(2, dtype=np.int32)
    for score in (-(1 << 23) + 1, -1, 0, 1, (1 << 23) - 1):
        for origin in (0, 1, (1 << 28) - 1):
            for add in (0, -7, 1 << 22, -(1 << 22)):
                sim.sim_span_roundtrip(score, origin, add, out.ctypes.data)
                assert tuple(out) == (score + add, origin), (score, origin, add)


def test_small_cases_every_system_and_strip_height(sim):
    for seed in range(420):
        t, o, system = C.small_case(seed)
        want = R.span_origins(t, o, system)
        assert _sim(sim, t, o, system, R_=(4, 2, 1)[seed % 3], W=1 + seed % 4) == want, (seed, t, o, system)


@pytest.mark.parametrize("alphabet", [2, 25])
def test_strip_and_group_edges(sim, alphabet):
    """row counts around the 64-lane strip (R = 1: strips of 64 rows; R = 4: 256), column counts around the 64-step
    start-up and the steady loop, several strips per wave so that the hand-off row is overwritten in place"""
    rng = np.random.RandomState(70 + alphabet)
    k = 0
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 513):
        for m in (0, 1, 2, 63, 64, 65, 300):
            if n * m > 60000 and (n + m) % 3:
                continue
            t = rng.randint(0, alphabet, size=n)
            o = rng.randint(0, alphabet, size=m)
            if n > m + 10 and m > 0 and k % 2:             # a planted span, exact or with a few substitutions
                a = int(rng.randint(0, n - m))
                o = t[a:a + m].copy()
                o[rng.randint(0, m, size=m // 8)] = rng.randint(0, alphabet)
            system = C.SYSTEMS[k % len(C.SYSTEMS)]
            want = R.span_numpy(t, o, system)
            r_ = (4, 1, 2)[k % 3]
            assert _sim(sim, t, o, system, R_=r_, W=(1, 2, 8, 3)[k % 4]) == want, (n, m, r_, system)
            k += 1
    assert k > 40


def test_a_wave_takes_a_second_strip(sim):
    """more than W strips (R = 1: 64 rows each): a wave's best joins that of its earlier strips, and a tie between two
    strips goes to the SMALLER i1 whichever wave holds it"""
    rng = np.random.RandomState(5)
    word = rng.randint(0, 4, size=40)
    t = np.concatenate([rng.randint(4, 8, size=100), word, rng.randint(4, 8, size=300), word, rng.randint(4, 8, size=200)])
    for W in (1, 2, 3, 8):
        for system in (C.SYSTEMS[0], C.SYSTEMS[3]):
            want = R.span_numpy(t, word, system)
            if system is C.SYSTEMS[0]:
                assert want[:2] == (100, 140)               # both copies score the same: the first one
            assert _sim(sim, t, word, system, R_=1, W=W) == want
            assert _sim(sim, t, word, system, R_=4, W=W) == want
    t = rng.randint(0, 3, size=1500)
    o = rng.randint(0, 3, size=90)
    for W in (2, 8):
        assert _sim(sim, t, o, C.SYSTEMS[1], R_=1, W=W) == R.span_numpy(t, o, C.SYSTEMS[1])


def test_noisy_planted_text(sim):
    tr, ocr, _ = C.planted(1003, 400, 170, 300, 0.75)
    t, o = C.codes(tr, ocr)
    for system in C.SYSTEMS:
        assert _sim(sim, t, o, system, R_=4, W=2) == R.span_numpy(t, o, system)
