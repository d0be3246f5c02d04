"""CPU check of what the labelling and skew-search kernels of csrc/ta_preproc.hip share: tests/native/sim_pp.cpp compiles
the same csrc/pp_cc.h as the kernels and (1) labels a page over runs in the run labeller's steps -- segments of 64 with
the carry, tables in raster order, join to the row above through the search, lock-free union, roots -- for ink and for
paper, held against scipy.ndimage.label with the 3 x 3 structure: raster-first pixel, area and box of every component;
(2) computes the row every point of a decimated page lands on under the skew search's angles, which must equal the
float64 expression of oracle/preproc_ref.py (rotation_angle_projections, score) exactly."""
import ctypes

import numpy as np
import pytest
from scipy import ndimage

import simlib


# the 64 and the 8 x 64 borders of the kernels' row loops, the band border at row 32
SHAPES = [(1, 1), (1, 64), (1, 65), (3, 63), (7, 128), (33, 129), (40, 513), (70, 1025)]
DENSITIES = [0.05, 0.5, 0.95]


@pytest.fixture(scope="module")
def sim():
    lib = simlib.load("pp", [simlib.CSRC + "pp_cc.h", simlib.CSRC + "corr1d.h"], flags=["-ffp-contract=off"])
    lib.sim_pp_label.restype = ctypes.c_int
    lib.sim_pp_label.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    lib.sim_pp_skew_rows.restype = None
    lib.sim_pp_skew_rows.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    return lib


def scipy_table(mask):
    """{first pixel in raster order, area, x0, y0, x1, y1} of every 8-connected component, by first pixel"""
    lab, n = ndimage.label(mask, structure=np.ones((3, 3), bool))
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    _, first = np.unique(flat[idx], return_index=True)
    area = np.bincount(flat, minlength=n + 1)[1:]
    rows = [(int(idx[first[k]]), int(area[k]), sl[1].start, sl[0].start, sl[1].stop - 1, sl[0].stop - 1)
            for k, sl in enumerate(ndimage.find_objects(lab))]
    return np.array(sorted(rows), dtype=np.int32).reshape(-1, 6)


def _pages():
    rng = np.random.default_rng(64)
    pages = [("%dx%d at %.2f" % (h, w, d), rng.random((h, w)) < d) for h, w in SHAPES for d in DENSITIES]
    pages.append(("checkerboard", (np.add.outer(np.arange(40), np.arange(131)) % 2) == 0))
    diag = np.zeros((70, 200), bool)                        # pixels that touch only at corners: one diagonal alone, two that cross
    k = np.arange(70)
    diag[k, 10 + k] = True; diag[k, 150 - k] = True; diag[k, 120 + k] = True
    pages.append(("diagonals", diag))
    pages.append(("all ink", np.ones((35, 70), bool)))
    pages.append(("empty", np.zeros((35, 70), bool)))
    return pages


def test_labelling_over_runs_equals_scipy(sim):
    for name, mask in _pages():
        plane = np.ascontiguousarray(mask, dtype=np.uint8)
        h, w = plane.shape
        for want in (1, 0):                                  # the runs of ink, and of paper (the hole filling)
            expect = scipy_table(mask if want else ~mask)
            cap = h * ((w + 1) // 2)                         # a row has at most ceil(w / 2) runs
            recs = np.full((cap, 6), -7, np.int32)
            count = sim.sim_pp_label(plane.ctypes.data, h, w, want, recs.ctypes.data, cap)
            assert count == len(expect), (name, want, count, len(expect))
            assert np.array_equal(recs[:count], expect), (name, want)
    assert len(scipy_table(_pages()[-3][1])) == 2           # the diagonals: 209 pixels, no two share an edge, two components


def test_skew_rows_equal_the_host_expression(sim):
    hs, ws = 300, 200
    ys, xs = (a.ravel().astype(np.int32) for a in np.mgrid[0:hs, 0:ws])
    cy, cx = (hs - 1) / 2.0, (ws - 1) / 2.0
    dy, dx = ys - cy, xs - cx
    for ang in np.arange(-6.0, 6.0 + 1e-9, 0.75):
        a = np.deg2rad(ang)
        want = np.rint(cy + dy * np.cos(a) - dx * np.sin(a)).astype(np.int64)      # oracle/preproc_ref.py, score()
        got = np.full(ys.size, -99, np.int64)
        sim.sim_pp_skew_rows(ys.ctypes.data, xs.ctypes.data, ys.size, hs, ws, float(np.cos(a)), float(np.sin(a)), got.ctypes.data)
        assert np.array_equal(got, want), (ang, int(np.count_nonzero(got != want)))
