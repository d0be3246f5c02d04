"""CPU check of the gaussians' tap loop: tests/native/sim_corr1d.cpp compiles the same csrc/corr1d.h as the kernels
of ta_lineest.hip and ta_distort.hip and runs ring_taps<NO> along a line under both border rules.  The integer
decisions of the normaliser hang on the last bit of these sums, so the result must equal scipy's correlate1d BIT FOR
BIT: same products, same order of additions, no contraction."""
import ctypes

import numpy as np
import pytest
from scipy import ndimage

import simlib


SIGMAS = [0.3, 1.0, 2.5, 10, 30]            # radii 1, 4, 10, 40, 120
LENGTHS = [1, 2, 3, 7, 33, 64, 257]         # reach not a multiple of NO, reach several times n


@pytest.fixture(scope="module")
def sim():
    lib = simlib.load("corr1d", [simlib.CSRC + "corr1d.h"], flags=["-ffp-contract=off"])
    lib.sim_corr1d.restype = ctypes.c_int
    lib.sim_corr1d.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                               ctypes.c_int, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def cases():
    """(x, weights, radius, scipy's result under 'constant' and under 'reflect'), computed once"""
    from text_alignment_amd import lineest_gpu
    rng = np.random.default_rng(31)
    out = []
    for sigma in SIGMAS:
        w, rad = lineest_gpu._gauss_weights(sigma)
        w = np.ascontiguousarray(w, dtype=np.float64)
        assert len(w) == 2 * rad + 1 and np.array_equal(w, w[::-1])
        for n in LENGTHS:
            x = rng.standard_normal(n)
            want = [ndimage.correlate1d(x, w, mode=mode) for mode in ("constant", "reflect")]
            out.append((x, w, rad, want))
    assert sorted({c[2] for c in out}) == [1, 4, 10, 40, 120]
    return out


@pytest.mark.parametrize("no", [1, 4, 5, 7, 8, 9])
def test_ring_taps_equal_scipy_bit_for_bit(sim, cases, no):
    for x, w, rad, want in cases:
        for mode in (0, 1):
            got = np.full(len(x), np.nan)
            assert sim.sim_corr1d(no, x.ctypes.data, len(x), w.ctypes.data, rad, mode, got.ctypes.data) == 0
            assert got.tobytes() == want[mode].tobytes(), (no, len(x), rad, ("constant", "reflect")[mode],
                                                            float(np.abs(got - want[mode]).max()))

