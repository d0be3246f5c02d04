"""The banded fill's data flow on the CPU (tests/native/sim_nw_band.cpp): phase 1 runs only the groups band_groups()
names, from the sentinel state, with the sentinel tail in a strip's last row -- and the unchanged phase 2 must never
restart from or re-fill with anything phase 1 did not write (the replay fails with a negative code if it does).  Where
the certificate passes the alignment equals the oracle's; where the oracle's path leaves the band it must not pass."""
import ctypes

import numpy as np
import pytest

import simlib
from oracle import nw_oracle
from tools.synth import synth_pair_ids

DEFAULT = [8, -4, -7, -7, -3, 0]
FLOWS = [32, 1064, 2064]        # nw_trace2_kernel (32-lane window), nw_trace2w_kernel, nw_trace2h_kernel (half-strips)


@pytest.fixture(scope="module")
def sim():
    lib = simlib.load("nw_band", [simlib.NAT + "sim_nw.cpp", simlib.CSRC + "nw_cell.h", simlib.CSRC + "nw_band.h"])
    lib.sim_nw2_band.restype = ctypes.c_int
    lib.sim_nw2_band.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                 ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
    return lib


def _run(lib, t, o, params, w, flow):
    t = np.ascontiguousarray(t, dtype=np.int32)
    o = np.ascontiguousarray(o, dtype=np.int32)
    p = np.asarray(params, dtype=np.int32)
    ops = np.zeros(len(t) + len(o) + 1, dtype=np.uint8)
    ln = ctypes.c_int(0)
    info = np.zeros(3, dtype=np.int32)
    rc = lib.sim_nw2_band(t.ctypes.data, len(t), o.ctypes.data, len(o), p.ctypes.data, w, flow, ops.ctypes.data,
                          ctypes.byref(ln), info.ctypes.data)
    assert rc == 0, (rc, len(t), len(o), w, flow)
    return bool(info[0]), int(info[1]), int(info[2]), ops[:ln.value]


def _excursion(ops):
    """(min, max) of j - i along an alignment"""
    d = np.concatenate([[0], np.cumsum((ops != 1).astype(np.int64) - (ops != 2).astype(np.int64))])
    return int(d.min()), int(d.max())


def _path_score(t, o, ops, s):
    sc, i, j, prev = 0, 0, 0, None
    for op in ops.tolist():
        if op == 0:
            sc += s[0] if t[i] == o[j] else s[1]; i += 1; j += 1
        elif op == 1:
            sc += s[4] + (s[2] if prev != 1 else 0); i += 1
        else:
            sc += s[5] + (s[3] if prev != 2 else 0); j += 1
        prev = op
    return sc


def _check(lib, t, o, params, w, flow, must_certify=None):
    n, m = len(t), len(o)
    want = nw_oracle.align_ids(t, o, params)
    ok, v0, U, got = _run(lib, t, o, params, w, flow)
    lo, hi = min(0, m - n) - w, max(0, m - n) + w
    dmin, dmax = _excursion(want)
    inside = lo <= dmin and dmax <= hi
    if ok:
        assert inside, (n, m, w, "certified although the oracle's path leaves the band", dmin, dmax)
        assert got.tolist() == want.tolist(), (n, m, w, flow)
    if not inside:
        assert not ok
    if must_certify is not None:
        assert ok == must_certify, (n, m, w, v0, U)
    return ok, v0, U


@pytest.mark.parametrize("flow", FLOWS)
def test_banded_replay_certified(sim, flow):
    for (n, m, seed), widths in [((1100, 1100, 11), (488, 400)), ((1300, 900, 12), (488,)),
                                 ((900, 1300, 13), (488,)), ((1537, 1601, 14), (700,)), ((2049, 2048, 15), (910,))]:
        t, o = synth_pair_ids(n, m, seed)
        for w in widths:
            ok, v0, U = _check(sim, t, o, DEFAULT, w, flow, must_certify=True)
            # v0 is the smallest of the last cell's three values, all exact where certified: the oracle's path is worth
            # one of them, and they lie within a gap open + extend and a substitution of each other
            assert 0 <= _path_score(t, o, nw_oracle.align_ids(t, o, DEFAULT), DEFAULT) - v0 <= 40


@pytest.mark.parametrize("flow", FLOWS)
def test_banded_replay_uncertified(sim, flow):
    # the rule's own width for 1300 x 900 alone: the 400 unmatched rows cost more than the bound allows for
    t, o = synth_pair_ids(1300, 900, 12)
    _check(sim, t, o, DEFAULT, 355, flow, must_certify=False)
    # bands far narrower than the rule's: the path stays inside, but the bound cannot show it
    t, o = synth_pair_ids(1100, 1100, 11)
    for w in (64, 200):
        _check(sim, t, o, DEFAULT, w, flow, must_certify=False)
    # unrelated strings score low
    rng = np.random.default_rng(5)
    _check(sim, rng.integers(0, 27, 1100), rng.integers(0, 27, 1100), DEFAULT, 488, flow, must_certify=False)
    # a path that leaves the band: t = X k + C, o = C + Y k
    C = rng.integers(0, 20, 900)
    for k in (186, 256, 326):
        t = np.concatenate([np.full(k, 25), C]); o = np.concatenate([C, np.full(k, 26)])
        _check(sim, t, o, DEFAULT, 256, flow)


@pytest.mark.parametrize("flow", [2064])
def test_banded_replay_other_systems_and_edges(sim, flow):
    """sizes around strip, half-strip and checkpoint-interval borders (the walk's start probes the unit above when
    n - 1 is a multiple of the unit), other scoring systems with non-positive gap opens"""
    for n, m, seed in [(1025, 1030, 1), (1153, 1100, 2), (1281, 1281, 3), (1024, 1088, 4), (1280, 1217, 5), (1101, 1024, 6)]:
        t, o = synth_pair_ids(n, m, seed)
        for params in (DEFAULT, [10, -5, -7, -7, -7, -7], [5, -10, -2, -7, 0, -5], [11, -4, -2, -2, 0, 0]):
            for w in (80, 300):
                _check(sim, t, o, params, w, flow)
