"""The chained span search without a GPU: tests/native/sim_span_chain.cpp replays ta_nw_span_chain's three kernels on the
host with the SAME nw_span.h they compile -- the fill's chained boundary, lane step and last-column store, the carry's
tiles, the walk's reduction -- and every output must equal the checker tests/span_chain_ref.py, integer for integer.
R = the fill's rows per lane (strips of 64 R rows), W = the waves of the carry's and the walk's workgroup (tiles of
256 W rows); the chained fill itself keeps no per-wave state, so W does not enter it."""
import ctypes

import numpy as np
import pytest

import span_cases as C
import span_chain_ref as CH
import simlib
from test_span_chain import repeated_passage

DEFAULT = [8, -12, -6, -6, -2, -2]


@pytest.fixture(scope="module")
def sim():
    lib = simlib.load("span_chain", [simlib.CSRC + "nw_span.h", simlib.CSRC + "nw_cell.h"])
    lib.sim_span_chain.restype = ctypes.c_int
    lib.sim_span_chain.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                   ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                   ctypes.c_void_p]
    return lib


def _sim(lib, t, pages, system, floor, R_=4, W=4):
    tt = np.concatenate([np.asarray(t, dtype=np.int32), [9999]]).astype(np.int32)          # never empty buffers
    oo = np.concatenate([np.asarray(o, dtype=np.int32) for o in pages] + [[9998]]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(o) for o in pages])]).astype(np.int64)
    p = np.ascontiguousarray(system, dtype=np.int32)
    out = np.full((len(pages), 3), -77, dtype=np.int32)
    total = np.full(1, -77, dtype=np.int64)
    assert lib.sim_span_chain(tt.ctypes.data, len(t), oo.ctypes.data, off.ctypes.data, len(pages), p.ctypes.data,
                              int(floor), R_, W, out.ctypes.data, total.ctypes.data) == 0
    return [tuple(int(v) for v in row) for row in out], int(total[0])


def _bound(t, pages, system):
    return (len(t) + max(len(o) for o in pages) + 2) * (3 * max(abs(v) for v in system) + 2)


def test_small_chains_every_system(sim):
    from test_span_chain import _random_chain
    for seed in range(300):
        t, pages, system = _random_chain(seed)
        if seed % 2:
            system = C.SYSTEMS[seed % len(C.SYSTEMS)]
        for floor in (_bound(t, pages, system), 3):
            want = CH.chain_plain(t, pages, system, floor)[:2]
            assert _sim(sim, t, pages, system, floor, R_=(4, 2, 1)[seed % 3], W=1 + seed % 4) == want, (seed, floor)


def test_strip_tile_and_group_edges(sim):
    """row counts around one strip (64 R rows) and around the carry's tile (256 W rows), column counts around the 64-step
    start-up, chains of 1, 2 and 5 pages with an empty page inside"""
    rng = np.random.RandomState(77)
    ms = (0, 1, 63, 64, 65, 300)
    k = 0
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 513):
        for P in (1, 2, 5):
            for rep in range(2):
                r_, w_ = (4, 1, 2)[k % 3], (1, 2, 3, 8)[k % 4]
                t = rng.randint(0, 4, size=n)
                pages = []
                for p in range(P):
                    m = ms[(k + p * 5 + rep * 3) % len(ms)]
                    o = rng.randint(0, 4, size=m)
                    if 0 < m < n and (k + p) % 2:                # a planted page, a few substitutions
                        a = int(rng.randint(0, n - m))
                        o = t[a:a + m].copy()
                        o[rng.randint(0, m, size=m // 8)] = rng.randint(0, 4)
                    pages.append(o)
                system = C.SYSTEMS[k % len(C.SYSTEMS)]
                for floor in (_bound(t, pages, system), 5):
                    want = CH.chain_numpy(t, pages, system, floor)[:2]
                    assert _sim(sim, t, pages, system, floor, R_=r_, W=w_) == want, (n, P, r_, w_, system, floor)
                k += 1
    assert k == 54


def test_every_r_and_w_on_one_chain(sim):
    rng = np.random.RandomState(78)
    t = rng.randint(0, 3, size=513)
    pages = [t[10:74].copy(), rng.randint(0, 3, size=0), t[200:263].copy(), rng.randint(0, 3, size=65), t[400:401].copy()]
    for system in (C.SYSTEMS[0], C.SYSTEMS[3]):
        want = CH.chain_numpy(t, pages, system, _bound(t, pages, system))[:2]
        for r_ in (1, 2, 4):
            for w_ in (1, 2, 3, 8):
                assert _sim(sim, t, pages, system, _bound(t, pages, system), R_=r_, W=w_) == want, (r_, w_)


def test_repeated_passage(sim):
    t, pages = repeated_passage()
    got = _sim(sim, t, pages, DEFAULT, _bound(t, pages, DEFAULT))
    assert [s[:2] for s in got[0]] == [(70, 130), (130, 190), (190, 230)]
    assert got == CH.chain_numpy(t, pages, DEFAULT, _bound(t, pages, DEFAULT))[:2]
