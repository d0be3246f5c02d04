"""The strips that tests/test_lineest_sim.py (the host build of csrc/ta_lineest.hip) and tests/test_lineest_gpu.py (the
real kernels) share, and the checker's answers for them (oracle/lineest_ref.py: scipy.ndimage in float64), computed once
per process.

A case is (name, pixels): a 2-D uint8 strip; the random ones are seeded by their own names, so a case added or taken out
leaves the others as they were.  ACCEPTED cases go through the checker with an output width >= 1; REFUSED ones make it
raise ValueError because their output width int(48 / (2 r) * w) is 0.

The kernel facts behind the geometry cases (random ink of density 0.3, black on white):
  row pass      sigma = h, radius 4 h, reach = min(4 h, w - 1); the LDS kernel while reach <= 640, 5 / 7 / 9 outputs per
                lane for w <= 1280 / <= 1792 / beyond, a tile = 256 lanes' outputs
  column pass   radius 2 h, reach = h - 1; the LDS kernel while h <= 96, four rows per lane, four waves
  centre line   radius int(1.2 h + 0.5), 'reflect'
  box filter    sizes int(0.5 h) and w, eight steps per chunk; a size <= 1 is a copy
"""
import zlib

import numpy as np

TARGET_HEIGHT, PAD = 48, 16


def strip(rng, h, w, wobble=0.0):
    """word-like ink blobs around a (possibly curved) baseline, grey-level antialiasing"""
    yy = np.arange(h)[:, None]
    base = h / 2.0 + wobble * np.sin(np.arange(w) / 97.0)[None, :]
    dens = 0.6 * np.exp(-0.5 * ((yy - base) / (h / 7.0)) ** 2)
    ink = rng.random((h, w)) < dens
    gaps = np.zeros(w, bool)
    x = int(rng.integers(5, 40))
    while x < w:
        g = int(rng.integers(8, 30))
        gaps[x:x + g] = True
        x += g + int(rng.integers(40, 120))
    ink[:, gaps] = False
    grey = np.where(ink, rng.integers(0, 90, size=(h, w)), rng.integers(235, 256, size=(h, w)))
    return grey.astype(np.uint8)


def word_strips():
    """the eleven strips tests/test_lineest_gpu.py began with.  The last two shapes take the kernels without an LDS tile:
    97 rows is the shortest strip of the tall-column gaussian, 161 x 643 (reach 642 > 640) a small one of the wide-row
    gaussian"""
    rng = np.random.default_rng(5)
    shapes = [(44, 1216), (61, 900), (70, 1500), (33, 300), (96, 700), (20, 120), (52, 2000), (45, 64),
              (97, 65), (161, 643)]
    strips = [strip(rng, h, w, wobble=(3.0 if k % 2 else 0.0)) for k, (h, w) in enumerate(shapes)]
    strips.append(np.where(strips[0] < 128, 0, 255).astype(np.uint8))        # bilevel, as the page cutter saves them
    return strips


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def scatter(name, h, w, density=0.3):
    """random ink, black on white"""
    return np.where(_rng(name).random((h, w)) < density, 0, 255).astype(np.uint8)


def _white(h, w):
    return np.full((h, w), 255, np.uint8)


def one_pixel(h, w, i, j):
    s = _white(h, w)
    s[i, j] = 0
    return s


# widths at the row kernel's switches of outputs per lane; 2305: the first strip with a second tile, of one column
ROW_SWITCH = [(30, 1280), (30, 1281), (30, 1792), (30, 1793), (30, 2304), (30, 2305)]
BENCH_WIDTH = [(60, 4400)]                      # the benchmark's pages: a nearly full second tile
# 160 x 1800: reach 640 and nine outputs per lane fill the row kernel's LDS array to its last element; 161 x 641: taller
# than 160 and still reach 640; 161 x 642: reach 641, the plain row kernel's smallest
HAND_OVER = [(160, 1800), (160, 641), (161, 641), (161, 642)]
# reach below the outputs per lane, partial groups of rows and of columns, the box filter's copy branch and its chunks
SMALL = [(1, 50), (2, 40), (3, 3), (4, 9), (5, 7), (8, 2), (8, 4), (8, 6), (12, 9), (9, 8), (10, 10), (17, 63),
         (16, 64), (95, 65), (98, 70), (99, 130)]
REFLECTED = [(40, 3), (40, 7)]                  # the centre line's reflect loop folds many times
ONE_COLUMN = [(8, 1, 5), (40, 1, 17)]           # (h, 1, row of the single ink pixel): r = 1, width 24


def _content():
    h, w = 40, 200
    out = []
    s = _white(h, w); s[0] = scatter("row 0", 1, w)[0]
    out.append(("ink in row 0 only", s))
    s = _white(h, w); s[h - 1] = scatter("row h-1", 1, w)[0]
    out.append(("ink in row h-1 only", s))
    out.append(("single ink pixel", one_pixel(h, w, 17, 90)))                # r = 1: 24-fold upsampling, 4 832 rows
    s = _white(h, w); s[:3] = scatter("top band", 3, w, 0.6); s[-3:] = scatter("bottom band", 3, w, 0.6)
    out.append(("bands at both edges", s))                                   # r > h
    s = _white(50, 400); s[(np.arange(400) * 49) // 399, np.arange(400)] = 0
    out.append(("diagonal 50x400", s))                                       # a steep baseline
    s = _white(h, w); s[:, 0] = scatter("column 0", h, 1, 0.5)[:, 0]
    out.append(("ink in column 0 only", s))
    s = _white(h, w); s[:, -1] = scatter("last column", h, 1, 0.5)[:, 0]
    out.append(("ink in the last column only", s))
    out.append(("white ink on black", 255 - scatter("inverted", h, w)))
    rng = _rng("grey band")
    s = np.where(rng.random((h, w)) < 0.3, rng.integers(100, 131, size=(h, w)), rng.integers(150, 181, size=(h, w)))
    s[0, 0], s[h - 1, w - 1] = 180, 100
    out.append(("values 100..180", s.astype(np.uint8)))                      # cval != 1, tmax != 1
    out.append(("bilevel", np.where(strip(_rng("bilevel"), h, w, wobble=2.0) < 128, 0, 255).astype(np.uint8)))
    return out


_CASES = {}


def accepted():
    """[(name, pixels)]: the word strips first, then geometry, then content"""
    if "accepted" not in _CASES:
        out = [("word strip %d (%dx%d)" % (k, s.shape[0], s.shape[1]), s) for k, s in enumerate(word_strips())]
        for h, w in ROW_SWITCH + BENCH_WIDTH + HAND_OVER + SMALL + REFLECTED:
            name = "scatter %dx%d" % (h, w)
            out.append((name, scatter(name, h, w)))
        for h, w, i in ONE_COLUMN:
            out.append(("one pixel %dx%d" % (h, w), one_pixel(h, w, i, 0)))
        out += _content()
        assert len({name for name, _ in out}) == len(out)
        _CASES["accepted"] = out
    return _CASES["accepted"]


def refused():
    """[(name, pixels)]: the checker raises ValueError for these, their output width being 0"""
    if "refused" not in _CASES:
        _CASES["refused"] = [(name, scatter(name, h, w)) for name, h, w in (("refused 60x1", 60, 1), ("refused 60x2", 60, 2))]
    return _CASES["refused"]


def by_name(name):
    return dict(accepted())[name]


class Want(object):
    """the checker's answers for one strip: arg (the per-column arg-max before it is smoothed), center, r, the output width
    wout and the rows of prepare_raw_strip, [wout + 32, 48] float64"""
    __slots__ = ("arg", "center", "r", "wout", "rows")


_WANT = {}


def want(name):
    """computed once per process; the stored arrays are read-only"""
    if name not in _WANT:
        from oracle import lineest_ref
        norm = lineest_ref.CenterNormalizer()
        rows = lineest_ref.prepare_raw_strip(by_name(name), norm)
        wt = Want()
        wt.arg, wt.center = np.asarray(norm.arg, np.int64), np.asarray(norm.center, np.int64)
        wt.r, wt.wout, wt.rows = int(norm.r), rows.shape[0] - 2 * PAD, rows
        for a in (wt.arg, wt.center, wt.rows):
            a.setflags(write=False)
        _WANT[name] = wt
    return _WANT[name]


def want_planes(name):
    """(smoothed, box-filtered): the two float64 images that CenterNormalizer.measure adds up before its arg-max, stated
    again here because the checker keeps neither"""
    from scipy.ndimage import gaussian_filter, uniform_filter
    line = by_name(name) / 255.0
    temp = np.amax(line) - line
    temp = temp * 1.0 / np.amax(temp)
    h, w = temp.shape
    smoothed = gaussian_filter(temp, (h * 0.5, h * 1.0), mode='constant')
    return smoothed, uniform_filter(smoothed, (h * 0.5, w), mode='constant')


def check_strip(name, arg, center, r, wout, rows, bound=2e-6):
    """what both test files assert of one strip: the integer decisions exactly, the rows to float32 rounding"""
    wt = want(name)
    assert np.array_equal(np.asarray(arg), wt.arg), (name, "arg")
    assert np.array_equal(np.asarray(center), wt.center), (name, "center")
    assert int(r) == wt.r, (name, "r", int(r), wt.r)
    assert int(wout) == wt.wout, (name, "width", int(wout), wt.wout)
    rows = np.asarray(rows)
    assert rows.shape == wt.rows.shape and rows.dtype == np.float32, (name, rows.shape, wt.rows.shape)
    assert np.isfinite(rows).all(), name
    err = float(np.abs(rows - wt.rows.astype(np.float32)).max())
    assert err <= bound, (name, "rows", err)
