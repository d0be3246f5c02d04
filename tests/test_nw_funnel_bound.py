"""The funnel's certificate (csrc/nw_band.h), without a GPU.  On small problems, against
exhaustive forward + backward tables of the reference's recurrence (test_nw_band_bound's), for every scoring system of
the reference's grid search and the default one, and regions that hold a run of columns per row with ends that do not
decrease from row to row -- random ones, under which nothing certifies on unrelated strings, and, on related strings,
the optimal paths' cells widened by 0 to 4 columns and funnels around the corner diagonals, under which thousands of
(region, system) cases certify:

* the exit bound X^ -- the maximum of Db(c) + a+ + Suf(c') over the cells c of the region or the boundary and their
  neighbours c' outside it, Db from the BANDED tables, a+ and Suf from the library -- is at least what any complete path
  through a cell outside the region scores;
* banded values never exceed the true ones;
* wherever v0 > X^ (v0 the smallest of the banded M, X, Y of the last cell), the walk over the banded tables is the walk
  over the full ones.

And the plan's closed-form spots: the funnel's ranges at the headline shape, the decline cases, n != m both ways."""
import numpy as np
import pytest

from test_nw_band_bound import NEG, SYSTEMS, _tables
from tools.nw_configs import DEFAULT_SYS

SHAPES = [(5, 17), (13, 24), (16, 16), (24, 24), (23, 9), (24, 2)]


def _banded_forward(n, m, eq, inside):
    """test_nw_band_bound._tables' forward recurrence with every cell outside the region left at NEG"""
    S = len(SYSTEMS)
    mat, mis, gox, goy, gex, gey = (SYSTEMS[:, k] for k in range(6))
    F = np.full((3, n + 1, m + 1, S), NEG, dtype=np.int64)
    for i in range(n + 1):
        F[0, i, 0] = -i; F[2, i, 0] = -i
    for j in range(m + 1):
        F[0, 0, j] = -j; F[1, 0, j] = -j
    F[2, 0, 0] = NEG
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            if not inside[i, j]:
                continue
            F[0, i, j] = F[:, i - 1, j - 1].max(axis=0) + np.where(eq[i - 1, j - 1], mat, mis)
            F[2, i, j] = np.maximum(np.maximum(F[0, i, j - 1] + goy + gey, F[1, i, j - 1] + goy + gey), F[2, i, j - 1] + gey)
            F[1, i, j] = np.maximum(np.maximum(F[0, i - 1, j] + gox + gex, F[1, i - 1, j] + gex), F[2, i - 1, j] + gox + gex)
    return np.maximum(F, NEG)                                     # (NEG + a few steps stays "none")


def _from_rows(n, m, lo, hi):
    """inside[i, j] for rows 1..n from columns lo[i - 1]..hi[i - 1], made non-decreasing, the last cell inside"""
    lo, hi = np.clip(lo, 1, m), np.clip(hi, 1, m)
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    lo, hi = np.maximum.accumulate(lo), np.maximum.accumulate(hi)
    hi[-1] = m
    inside = np.zeros((n + 1, m + 1), dtype=bool)
    for i in range(1, n + 1):
        inside[i, lo[i - 1]:hi[i - 1] + 1] = True
    return inside


def _regions(n, m, rng, count):
    """random regions: a run of columns per row, ends that do not decrease from row to row"""
    for _ in range(count):
        lo, hi = np.sort(rng.integers(1, m + 1, size=n)), np.sort(rng.integers(1, m + 1, size=n))
        if rng.integers(0, 2):
            lo[: rng.integers(1, n + 1)] = 1                      # starts at the boundary column, like a strip with gl = 0
        yield _from_rows(n, m, lo, hi)


def _regions_that_can_certify(n, m, T, rng):
    """Regions a good alignment stays inside, so that the certificate has a chance: the cells on optimal paths of one
    system (the default and two drawn ones) widened by d columns on either side -- d = 0: the region's border IS the
    path's, the last rows' three predecessors inside or not as the path has it -- and funnels around the diagonals
    through the table's corners whose widths shrink with the rows left, down to a floor."""
    S = len(SYSTEMS)
    rows = np.arange(1, n + 1)
    for k in [S - 1] + rng.integers(0, S - 1, size=2).tolist():
        opt = T[1:, 1:, k] == T[n, m, k]                          # interior cells on an optimal path of system k
        cols = [np.nonzero(r)[0] + 1 for r in opt]
        lo = np.array([c[0] if c.size else 1 for c in cols])
        hi = np.array([c[-1] if c.size else 1 for c in cols])
        for d in (0, 1, 2, 4):
            yield _from_rows(n, m, lo - d, hi + d)
        yield _from_rows(n, m, lo - 1, hi + 3)                    # lopsided, both ways
        yield _from_rows(n, m, lo - 3, hi + 1)
    for floor, slope in ((1, 2), (2, 2), (2, 4), (4, 3)):
        wide = floor + (n - rows) // slope
        yield _from_rows(n, m, rows + min(0, m - n) - wide, rows + max(0, m - n) + wide)
        yield _from_rows(n, m, np.where(rows <= n // 2, 1, rows + min(0, m - n) - wide), rows + max(0, m - n) + wide)


def _pairs(n, m, rng):
    """an unrelated pair (nothing should certify, the bound must still hold) and two related ones: the shorter string
    inside the longer one among inserted letters, with a substitution here and there"""
    yield rng.integers(0, 3, size=n), rng.integers(0, 3, size=m)
    for subs in (0, 2):
        short = rng.integers(0, 4, size=min(n, m))
        long_ = np.insert(short, np.sort(rng.integers(0, short.size + 1, size=abs(n - m))), rng.integers(0, 4, size=abs(n - m)))
        short = short.copy()
        at = rng.integers(0, short.size, size=min(subs, short.size))
        short[at] = (short[at] + 1) % 4
        yield (long_, short) if n >= m else (short, long_)


def _walk(F, k, eq, n, m):
    """the reference's walk on tables F[:, :, :, k]: from (n, m) in the state of its largest value (first maximum: M, X,
    Y), each step to the first predecessor state that reproduces the value"""
    mat, mis, gox, goy, gex, gey = (int(v) for v in SYSTEMS[k])
    i, j = n, m
    st = int(np.argmax(F[:, n, m, k]))
    ops = []
    while i > 0 and j > 0:
        ops.append(st)
        v = F[st, i, j, k]
        if st == 0:
            prev = [F[q, i - 1, j - 1, k] + (mat if eq[i - 1, j - 1] else mis) for q in range(3)]
            i -= 1; j -= 1
        elif st == 1:
            prev = [F[0, i - 1, j, k] + gox + gex, F[1, i - 1, j, k] + gex, F[2, i - 1, j, k] + gox + gex]
            i -= 1
        else:
            prev = [F[0, i, j - 1, k] + goy + gey, F[1, i, j - 1, k] + goy + gey, F[2, i, j - 1, k] + gey]
            j -= 1
        if i == 0 or j == 0:
            break
        hits = [q for q in range(3) if prev[q] == v]
        assert hits, "no predecessor reproduces the value"
        st = hits[0]
    return ops, (i, j)


# (region, system) cases that must certify per shape: over the six shapes ten times the 60 cases of the experiment the
# design rests on -- unrelated strings under arbitrary regions certify none, and the exactness half of the test would
# then pass without having compared a single walk
CERTIFIED_FLOOR = 100


@pytest.mark.parametrize("n,m", SHAPES)
def test_exit_bound_covers_every_path_that_leaves_the_region(native, n, m):
    rng = np.random.default_rng(77000 + 100 * n + m)
    S = len(SYSTEMS)
    prm = np.ascontiguousarray(SYSTEMS, dtype=np.int32)
    suf = np.zeros((n + 2, m + 2, S), dtype=np.int64)                                 # Suf(i, j), library's
    ap = np.zeros(S, dtype=np.int64)
    for k in range(S):
        a_out = np.zeros(1, dtype=np.int32)
        for rn in range(n + 1):
            for rm in range(m + 1):
                suf[n - rn, m - rm, k] = native.lib.ta_nw2_funnel_suf(rn, rm, prm[k].ctypes.data, a_out.ctypes.data)
        ap[k] = a_out[0]
    certified = walked = 0
    for t, o in _pairs(n, m, rng):
        assert len(t) == n and len(o) == m
        eq2 = t[:, None] == o[None, :]
        eq = eq2[:, :, None]
        F, B = _tables(n, m, eq)
        T = np.where((F > NEG // 2) & (B > NEG // 2), F + B, NEG).max(axis=0)      # best complete path through a cell
        # Suf bounds the true remainder from every interior cell in every state
        assert (B[:, 1:, 1:] <= suf[None, 1:n + 1, 1:m + 1]).all()
        for inside in list(_regions(n, m, rng, 4)) + list(_regions_that_can_certify(n, m, T, rng)):
            Fb = _banded_forward(n, m, eq, inside)
            assert (Fb <= F).all()                                        # banded <= true
            Db = Fb.max(axis=0)
            in_or_bnd = inside.copy(); in_or_bnd[0, :] = True; in_or_bnd[:, 0] = True
            outside = ~in_or_bnd
            xhat = np.full(S, NEG, dtype=np.int64)
            for di, dj in ((0, 1), (1, 0), (1, 1)):
                src = in_or_bnd[:n + 1 - di, :m + 1 - dj] & outside[di:, dj:]
                if src.any():
                    cand = Db[:n + 1 - di, :m + 1 - dj][src] + ap + suf[di:n + 1, dj:m + 1][src]
                    xhat = np.maximum(xhat, cand.max(axis=0))
            if outside.any():
                worst = T[outside].max(axis=0)
                bad = np.nonzero(worst > xhat)[0]
                assert bad.size == 0, (n, m, SYSTEMS[bad[0]].tolist(), int(worst[bad[0]]), int(xhat[bad[0]]))
            else:
                continue                                                  # (the whole table: nothing to certify)
            v0 = Fb[:, n, m].min(axis=0)
            ok = np.nonzero(v0 > xhat)[0]
            certified += ok.size
            for k in ok.tolist():
                assert (Fb[:, n, m, k] == F[:, n, m, k]).all()
                assert _walk(Fb, k, eq2, n, m) == _walk(F, k, eq2, n, m), (n, m, SYSTEMS[k].tolist())
                walked += 1
    print("n", n, "m", m, "certified (region, system) cases", certified, "walks compared", walked)
    assert certified >= CERTIFIED_FLOOR and walked == certified, (n, m, certified, walked)


def _plan(native, n, m, nprob=64, system=DEFAULT_SYS, band=0):
    flags = (28 << native.TA_NW_ALPHABET_SHIFT) | native.TA_NW_OPENS_SAME | native.TA_NW_CODES8
    n32, m32 = np.full(nprob, n, np.int32), np.full(nprob, m, np.int32)
    p = np.array(system, dtype=np.int32)
    out, u, r = np.zeros(8, np.int32), np.zeros(nprob, np.int32), np.zeros(2 * 64, np.int32)
    assert native.lib.ta_nw2_band_plan(n32.ctypes.data, m32.ctypes.data, nprob, p.ctypes.data, 0, flags, band,
                                       out.ctypes.data, u.ctypes.data, r.ctypes.data, len(r)) == 0
    return out, u, [tuple(x) for x in r[:2 * out[3]].reshape(-1, 2).tolist()]


def _funnel(native, n, m, w, system=DEFAULT_SYS):
    n32, m32 = np.full(1, n, np.int32), np.full(1, m, np.int32)
    p = np.array(system, dtype=np.int32)
    x0, r, out = np.zeros(1, np.int32), np.zeros(2 * 64, np.int32), np.zeros(4, np.int32)
    assert native.lib.ta_nw2_funnel_plan(n32.ctypes.data, m32.ctypes.data, 1, p.ctypes.data, 0, w, 0, x0.ctypes.data,
                                         r.ctypes.data, len(r), out.ctypes.data) == 0
    ns = (n + 255) // 256
    return bool(out[0]), out[1] / 1000.0, [tuple(x) for x in r[:2 * ns].reshape(-1, 2).tolist()], int(x0[0])


HEADLINE = [(0, 512), (0, 544), (0, 592), (0, 624), (0, 672), (0, 704), (0, 752), (64, 800), (160, 832), (256, 880),
            (368, 912), (464, 960), (560, 992), (672, 1040), (768, 1040), (864, 1040)]


def test_plan_reports_the_funnel_at_the_headline(native):
    out, u, ranges = _plan(native, 4096, 4096, nprob=4096)
    prm = np.array(DEFAULT_SYS, dtype=np.int32)
    assert out[0] == out[1] == 1820 and out[5] == 1 and out[3] == 16           # w is the outer band, unchanged
    assert (u == native.lib.ta_nw2_band_bound(4096, 4096, prm.ctypes.data, 1820)).all()
    assert ranges == HEADLINE
    assert out[2] == 524
    own, share, r2, x0 = _funnel(native, 4096, 4096, 1820)
    assert own and r2 == HEADLINE and abs(share - 0.524) < 1e-9
    # the host part of the exit bound.  Off the boundary row: strip 0 runs groups 0 .. 511, row 1 holds columns 1 .. 2048,
    # the best exit is (0, 2048) -> (1, 2049) with 4095 rows and 2047 columns left.  Off the boundary column: strip 7
    # is the first that starts past group 0, the best exit is (1792, 0) -> (1793, 1) with 2303 rows left, all of them
    # diagonal steps at best, and the 1792 columns over free of charge under gey = 0.  The larger one counts.
    row = -2048 + 8 + (2047 * 8 + 2048 * -3)
    col = -1792 + 8 + (4096 - 1793) * 8
    assert x0 == max(row, col) == 16640
    # a forced width keeps the uniform band
    out_f, _, ranges_f = _plan(native, 4096, 4096, nprob=4096, band=1820)
    assert out_f[0] == 1820 and out_f[5] == 0 and out_f[2] > 700 and ranges_f != HEADLINE


def test_funnel_shapes_and_declines(native):
    # n != m, both ways, and a smaller square: inside the uniform band, ranges that do not decrease, ends at the corners
    for n, m, w in [(4096, 3800, 1900), (3500, 4096, 1900), (4096, 4300, 1900), (3000, 3000, 1332), (1300, 900, 600),
                    (900, 1300, 600)]:
        own, share, ranges, x0 = _funnel(native, n, m, w)
        out_u, _, uni = _plan(native, n, m, band=w)
        assert own and len(ranges) == len(uni) == (n + 255) // 256
        r, ru = np.array(ranges), np.array(uni)
        assert (r[:, 0] >= ru[:, 0]).all() and (r[:, 1] <= ru[:, 1]).all()       # inside the outer band's groups
        assert (np.diff(r[:, 0]) >= 0).all() and (np.diff(r[:, 1]) >= 0).all() and (r[:, 0] < r[:, 1]).all()
        assert r[0, 0] == 0 and r[-1, 1] == (m + 63 + 3) // 4
        assert share <= out_u[2] / 1000.0 + 1e-9
    assert _funnel(native, 4096, 4096, 1820)[1] < _plan(native, 4096, 4096, band=1820)[0][2] / 1000.0 - 0.2
    # declined: a <= 0; gaps so cheap that a denominator is <= 0 -- the band's own ranges run
    for system in ([-1, -4, -7, -7, -3, 0], [4, -4, 0, 0, 1, 1], [8, -4, 3, 3, -1, -1]):
        own, share, ranges, x0 = _funnel(native, 2048, 2048, 500, system)
        assert not own and ranges == _plan(native, 2048, 2048, band=500, system=system)[2]
    # the rule's declines stay declined (the uniform band's share decides)
    out = _plan(native, 1100, 1100)[0]
    assert out[0] == 0 and out[1] == 488 and out[5] == 0
    assert _plan(native, 1000, 4096)[0][0] == 0
