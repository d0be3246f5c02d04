"""The strips that tests/test_distort_sim.py (the host build of csrc/ta_distort.hip) and tests/test_distort_edges_gpu.py
(the real kernels) share, the checker's answers for them (tests/distort_ref.py), computed once per process, and the one
comparison both files make: check_case.

A case is (name, strip, sigma, distort): a 2-D uint8 strip, the smoothing sigma and the maximal displacement.  The random
strips are seeded by their kind and size, so a case added or taken out leaves the others as they were.  Cases are grouped
by (sigma, distort) -- a call of ta_line_distort has one of each -- and case k of a group draws its noise with the key
SEED and the counter FIRST + k: the key and counter of the third Philox known answer (tests/test_distort.py), both with
a non-zero high word.

Every case is there for a branch of the kernels, stated below as a sentence and as a predicate over the SOURCE's
constants and its own choice of the column tile (tests/native/sim_distort.cpp: sim_distort_constants,
sim_distort_col_tile), which tests/test_distort_sim.py evaluates: a constant or a fit test that changes fails there,
loudly, instead of moving a case off its edge.  The kernel facts behind them:
  column pass   a tile of ct columns, the largest power of two <= kDsColTile with (h + 2 radius) ct <= kDsColCells; the
                grid has min(tiles, kDsGridTiles) of them per line, a strip with more is swept
  row pass      5 / 7 / kDsRowMaxNO outputs per lane for w <= kDsRowW5 / <= kDsRowW7 / beyond; a tile = kDsThreads lanes'
                outputs, staged with `radius` elements each side in kDsRowCells doubles; max_h workgroups per line
  resampling    cval = the strip's maximum, from ds_imax_kernel
"""
import collections
import zlib

import numpy as np

import distort_ref as R

SEED, FIRST = 0x299f31d0a4093822, 0x0370734413198a2e
FIELD_BOUND = 1e-9              # x distort: the bound of tests/test_distort_gpu.py, independent of the code under test
NEAR = 1e-6                     # a pixel is excluded where the checker's v, sy or sx is this close to a decision
EXCLUDED_SHARE = 1e-3           # of all cases' pixels, at most

# the last is the source's function (h, radius) -> columns per tile of the column pass, the others its integers
Constants = collections.namedtuple(
    "Constants", "threads col_cells col_tile row_w5 row_w7 row_max_no row_cells grid_tiles max_h max_radius col_tile_of")


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _strip(kind, h, w):
    """grey: ink 0..89 of density 0.3 on paper 235..255 (steep everywhere: a displaced sample shows); bilevel: 0 / 255,
    as the page cutter saves them; levels 0..90: nothing above 89 but the LAST pixel, which is 90 -- cval is not 255 and
    the maximum sits in the last lane's share of the strip"""
    rng = _rng("%s %dx%d" % (kind, h, w))
    if kind == "grey":
        s = np.where(rng.random((h, w)) < 0.3, rng.integers(0, 90, size=(h, w)), rng.integers(235, 256, size=(h, w)))
    elif kind == "bilevel":
        s = np.where(rng.random((h, w)) < 0.3, 0, 255)
    elif kind == "levels 0..90":
        s = rng.integers(0, 90, size=(h, w))
        s[h - 1, w - 1] = 90
    elif kind == "all 255":
        s = np.full((h, w), 255)
    elif kind == "all 0":
        s = np.zeros((h, w))
    else:
        raise ValueError(kind)
    s = s.astype(np.uint8)
    s.setflags(write=False)
    return s


def radius(sigma):
    return int(4.0 * float(sigma) + 0.5)


def col_tile(K, h, rad):
    """columns per tile of the column pass: what the source chooses"""
    return int(K.col_tile_of(h, rad))


def col_tiles(K, h, w, rad):
    ct = col_tile(K, h, rad)
    return (w + ct - 1) // ct


def col_full(K, h, rad):
    """the extended columns of a tile fill the column kernel's LDS array to its last element"""
    return (h + 2 * rad) * col_tile(K, h, rad) == K.col_cells


def row_no(K, w):
    """outputs per lane of the row pass"""
    return 5 if w <= K.row_w5 else 7 if w <= K.row_w7 else K.row_max_no


def row_tiles(K, w):
    tile = K.threads * row_no(K, w)
    return (w + tile - 1) // tile


def row_span(K, w, rad):
    """doubles of LDS a row tile is staged in"""
    return K.threads * row_no(K, w) + 2 * rad


# (kind, h, w, what the case is there for, predicate(K, h, w, rad)) per (sigma, distort), in the order of the batch
_GROUPS = [
    ((10.0, 3.0), [
        ("grey", 16, 70, "64-column tile, LDS exactly full, a partial second tile",
         lambda K, h, w, r: col_tile(K, h, r) == K.col_tile and col_full(K, h, r) and K.col_tile < w < 2 * K.col_tile),
        ("grey", 17, 70, "32-column tile: one row more than fits 64 columns",
         lambda K, h, w, r: col_tile(K, h, r) == 32 and col_tile(K, h - 1, r) == 64),
        ("grey", 112, 40, "32-column tile, LDS exactly full", lambda K, h, w, r: col_tile(K, h, r) == 32 and col_full(K, h, r)),
        ("bilevel", 113, 40, "16-column tile", lambda K, h, w, r: col_tile(K, h, r) == 16 and col_tile(K, h - 1, r) == 32),
        ("grey", 304, 20, "16-column tile, LDS exactly full", lambda K, h, w, r: col_tile(K, h, r) == 16 and col_full(K, h, r)),
        ("grey", 305, 20, "8-column tile; sets the row grid of its batch",
         lambda K, h, w, r: col_tile(K, h, r) == 8 and col_tile(K, h - 1, r) == 16),
        ("grey", 512, 9, "TA_DISTORT_MAX_H", lambda K, h, w, r: h == K.max_h),
        ("grey", 2, 1280, "row pass: the widest strip with 5 outputs per lane, every lane full",
         lambda K, h, w, r: w == K.row_w5 and row_no(K, w) == 5 and row_tiles(K, w) == 1),
        ("grey", 2, 1281, "row pass: the narrowest strip with 7 outputs per lane",
         lambda K, h, w, r: w == K.row_w5 + 1 and row_no(K, w) == 7),
        ("grey", 2, 1792, "row pass: the widest strip with 7 outputs per lane, every lane full",
         lambda K, h, w, r: w == K.row_w7 and row_no(K, w) == 7 and row_tiles(K, w) == 1),
        ("grey", 3, 2304, "row pass: one full tile of 9 outputs per lane",
         lambda K, h, w, r: w == K.threads * K.row_max_no and row_no(K, w) == K.row_max_no and row_tiles(K, w) == 1),
        ("grey", 2, 2305, "row pass: a second tile of one element; sets the tile count of its batch",
         lambda K, h, w, r: w == K.threads * K.row_max_no + 1 and row_tiles(K, w) == 2),
        ("bilevel", 2, 4700, "row pass: three tiles", lambda K, h, w, r: row_tiles(K, w) == 3),
        ("grey", 1, 1, "one pixel", lambda K, h, w, r: h == 1 and w == 1),
        ("grey", 5, 1, "one column", lambda K, h, w, r: w == 1 and h > 1),
        ("grey", 1, 2, "one row of two columns", lambda K, h, w, r: h == 1 and w == 2),
        ("levels 0..90", 40, 300, "cval is not 255; the maximum is the last pixel", None),
        ("all 255", 40, 300, "a constant strip", None),
        ("all 0", 12, 50, "a constant strip with cval 0", None),
    ]),
    ((2.5, 3.0), [
        ("grey", 76, 70, "64-column tile at radius 10, LDS exactly full",
         lambda K, h, w, r: r == 10 and col_tile(K, h, r) == K.col_tile and col_full(K, h, r)),
        ("grey", 77, 70, "32-column tile at radius 10", lambda K, h, w, r: col_tile(K, h, r) == 32),
    ]),
    ((0.1, 3.0), [("grey", 7, 50, "radius 0: the tap loop does not run", lambda K, h, w, r: r == 0)]),
    # (0.37, not the 0.13 that has radius 1 as well: there the one tap pair weighs 1.4e-13 and no bound could tell it lost)
    ((0.37, 3.0), [("grey", 7, 50, "radius 1: the tap loop runs once", lambda K, h, w, r: r == 1)]),
    ((32.0, 3.0), [("grey", 512, 5, "8-column tile, LDS exactly full, at TA_DISTORT_MAX_H",
                    lambda K, h, w, r: col_tile(K, h, r) == 8 and col_full(K, h, r))]),
    ((33.0, 3.0), [("grey", 512, 5, "4-column tile", lambda K, h, w, r: col_tile(K, h, r) == 4)]),
    ((130.0, 3.0), [("grey", 512, 5, "2-column tile", lambda K, h, w, r: col_tile(K, h, r) == 2)]),
    ((512.0, 0.75), [
        ("grey", 512, 3, "one-column tile; the extended column is the longest there is",
         lambda K, h, w, r: r == K.max_radius and h == K.max_h and col_tile(K, h, r) == 1 and h + 2 * r <= K.col_cells),
        ("grey", 2, 1793, "row pass at TA_DISTORT_MAX_RADIUS: the widest LDS span, one tile",
         lambda K, h, w, r: r == K.max_radius and row_tiles(K, w) == 1 and row_span(K, w, r) == K.row_cells - K.row_max_no),
        ("grey", 2, 4100, "more one-column tiles than the grid has: the column kernel's second sweep; a second row tile "
                          "at the largest radius",
         lambda K, h, w, r: col_tile(K, h, r) == 1 and K.grid_tiles < col_tiles(K, h, w, r) < 2 * K.grid_tiles
         and row_tiles(K, w) == 2 and r == K.max_radius),
    ]),
    ((10.0, 0.25), [("grey", 17, 70, "a small displacement", None), ("levels 0..90", 40, 300, "a small displacement", None)]),
    ((10.0, 40.0), [("grey", 17, 70, "nearly every pixel samples outside", None),
                    ("levels 0..90", 40, 300, "nearly every pixel samples outside: cval", None)]),
]

Case = collections.namedtuple("Case", "name strip sigma distort counter why claim")
_CASES = []
for (_sigma, _distort), _members in _GROUPS:
    for _k, (_kind, _h, _w, _why, _claim) in enumerate(_members):
        _CASES.append(Case("%dx%d %s, sigma %g, distort %g" % (_h, _w, _kind, _sigma, _distort), _strip(_kind, _h, _w),
                           _sigma, _distort, (FIRST + _k) % 2 ** 64, _why, _claim))
assert len({c.name for c in _CASES}) == len(_CASES)
_BY_NAME = {c.name: c for c in _CASES}


def cases():
    """[(name, strip, sigma, distort)]"""
    return [(c.name, c.strip, c.sigma, c.distort) for c in _CASES]


def case(name):
    """the whole record: name, strip, sigma, distort, counter, why, claim"""
    return _BY_NAME[name]


def groups():
    """[((sigma, distort), [name])]: the cases of one call, in the order of their counters FIRST, FIRST + 1, ..."""
    out = collections.OrderedDict()
    for c in _CASES:
        out.setdefault((c.sigma, c.distort), []).append(c.name)
    return list(out.items())


def claims(K):
    """[(name, sentence, holds)] of the cases that are there for a branch of the kernels, under the constants K"""
    return [(c.name, c.why, bool(c.claim(K, c.strip.shape[0], c.strip.shape[1], radius(c.sigma))))
            for c in _CASES if c.claim is not None]


Want = collections.namedtuple("Want", "out v d excluded")
_WANT = {}


def want(name):
    """the checker's output, unrounded values and fields of a case, and the pixels no comparison may rest on -- all of it
    from the checker's own values, computed once per process, read-only"""
    if name not in _WANT:
        c = _BY_NAME[name]
        out, v, d = R.distort_strip(c.strip, c.distort, c.sigma, SEED, c.counter)
        h, w = c.strip.shape
        sy = np.arange(h, dtype=np.float64)[:, None] + d[0]
        sx = np.arange(w, dtype=np.float64)[None, :] + d[1]
        # floor(v + 0.5) flips where v is a half-integer; inside / cval flips where the sample lies ON the rectangle's
        # border: the pixel where |F| peaks has |D| = distort to the last bit, so with a whole-numbered distort it lands
        # exactly on a row or column, and `distort` rows from an edge exactly on the border
        excluded = np.abs(v - np.floor(v) - 0.5) < NEAR
        excluded |= (np.abs(sy) < NEAR) | (np.abs(sy - (h - 1)) < NEAR) | (np.abs(sx) < NEAR) | (np.abs(sx - (w - 1)) < NEAR)
        for a in (out, v, d, excluded):
            a.setflags(write=False)
        _WANT[name] = Want(out, v, d, excluded)
    return _WANT[name]


def excluded_share():
    """(excluded pixels, pixels) over all cases"""
    return (sum(int(want(c.name).excluded.sum()) for c in _CASES), sum(c.strip.size for c in _CASES))


def check_case(name, out, fields):
    """what both test files assert of one case; returns the largest field error as a fraction of distort"""
    c, wt = _BY_NAME[name], want(name)
    out, fields = np.asarray(out), np.asarray(fields)
    assert out.shape == c.strip.shape and out.dtype == np.uint8, (name, out.shape, out.dtype)
    assert fields.shape == (2,) + c.strip.shape and fields.dtype == np.float64, (name, fields.shape, fields.dtype)
    assert np.isfinite(fields).all(), (name, "a field value was not written")
    err = float(np.abs(fields - wt.d).max())
    print("%s: max |D - D_ref| = %.3g (%.3g x distort); %d of %d pixels excluded"
          % (name, err, err / c.distort, int(wt.excluded.sum()), out.size))
    assert err <= FIELD_BOUND * c.distort, (name, "fields", err)
    for k in range(2):
        peak = float(np.abs(fields[k]).max())
        assert abs(peak - c.distort) <= 1e-12, (name, "peak of field %d" % k, peak)
    keep = ~wt.excluded
    wrong = int((out[keep] != wt.out[keep]).sum())
    assert wrong == 0, (name, "pixels", wrong, np.argwhere((out != wt.out) & keep)[:8].tolist())
    return err / c.distort


def _smooth_axis_short(a, sigma, axis):
    """R.smooth_axis with the outermost tap pair lost"""
    wts, rad = R.gauss_weights(sigma)
    n = a.shape[axis]
    idx = np.arange(n)
    out = np.take(a, idx, axis=axis) * wts[rad]
    for k in range(rad - 1, 0, -1):
        out = out + (np.take(a, R.reflect(idx - k, n), axis=axis) + np.take(a, R.reflect(idx + k, n), axis=axis)) * wts[rad - k]
    return out


def lost_tap_effect(name, axis):
    """the largest change of a field value of this case, as a fraction of distort, when the gaussian along `axis` loses
    its outermost tap pair: on the checker alone"""
    c = _BY_NAME[name]
    h, w = c.strip.shape
    worst = 0.0
    for k, n in enumerate(R.noise(h, w, SEED, c.counter)):
        if axis == 0:
            f = R.smooth_axis(_smooth_axis_short(n, c.sigma, 0), c.sigma, 1)
        else:
            f = _smooth_axis_short(R.smooth_axis(n, c.sigma, 0), c.sigma, 1)
        worst = max(worst, float(np.abs(f * (c.distort / np.abs(f).max()) - want(name).d[k]).max()))
    return worst / c.distort
