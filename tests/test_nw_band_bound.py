"""The bound the banded fill's certificate rests on (csrc/ta_nw2.hip), without a GPU:
ta_nw2_band_bound(n, m, system, w) is at least what ANY alignment that visits a cell outside the band
min(0, m - n) - w <= j - i <= max(0, m - n) + w can score -- checked against exhaustive best-score tables of the
reference's recurrence (textSeqCompare.py:53-88, boundary G = -1) on small problems, for every scoring system of the
reference's grid search and the default one, and every width."""
import numpy as np
import pytest

from tools.nw_configs import DEFAULT_SYS, grid_systems

NEG = -10 ** 9
SYSTEMS = np.array(grid_systems() + [DEFAULT_SYS], dtype=np.int64)          # (S, 6)
SHAPES = [(5, 17), (13, 24), (16, 16), (24, 24), (23, 9), (24, 2)]          # n < m, n = m, n > m


def _tables(n, m, eq):
    """Forward tables F[s][i][j] (the reference's mat / x_mat / y_mat: best prefix ending at (i, j) in state s = M, X, Y)
    and backward tables B[s][i][j] (best remainder from (i, j) in state s to (n, m) in any state), for all systems at
    once (last axis).  A move along the boundary row / column costs G = -1; the two states the boundary defines there
    have the same value, whichever the path was in before."""
    S = len(SYSTEMS)
    mat, mis, gox, goy, gex, gey = (SYSTEMS[:, k] for k in range(6))
    sc = lambda i, j: np.where(eq[i - 1, j - 1], mat, mis)
    F = np.full((3, n + 1, m + 1, S), NEG, dtype=np.int64)
    for i in range(n + 1):
        F[0, i, 0] = -i; F[2, i, 0] = -i
    for j in range(m + 1):
        F[0, 0, j] = -j; F[1, 0, j] = -j
    F[2, 0, 0] = NEG
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            F[0, i, j] = F[:, i - 1, j - 1].max(axis=0) + sc(i, j)
            F[2, i, j] = np.maximum(np.maximum(F[0, i, j - 1] + goy + gey, F[1, i, j - 1] + goy + gey), F[2, i, j - 1] + gey)
            F[1, i, j] = np.maximum(np.maximum(F[0, i - 1, j] + gox + gex, F[1, i - 1, j] + gex), F[2, i - 1, j] + gox + gex)
    B = np.full((3, n + 1, m + 1, S), NEG, dtype=np.int64)
    B[:, n, m] = 0
    for i in range(n, -1, -1):
        for j in range(m, -1, -1):
            if i == n and j == m:
                continue
            best = [np.full(S, NEG, dtype=np.int64) for _ in range(3)]
            if i < n and j < m:                                   # diagonal, into M, from any state
                d = B[0, i + 1, j + 1] + sc(i + 1, j + 1)
                best = [np.maximum(b, d) for b in best]
            if j < m:                                             # horizontal
                if i == 0:                                        # along row 0, where M = X = -j whatever came before
                    step = np.maximum(B[0, 0, j + 1], B[1, 0, j + 1]) - 1
                    best[0] = np.maximum(best[0], step)
                    best[1] = np.maximum(best[1], step)
                else:                                             # into Y
                    y = B[2, i, j + 1]
                    best[0] = np.maximum(best[0], y + goy + gey)
                    best[1] = np.maximum(best[1], y + goy + gey)
                    best[2] = np.maximum(best[2], y + gey)
            if i < n:                                             # vertical
                if j == 0:                                        # along column 0, where M = Y = -i
                    step = np.maximum(B[0, i + 1, 0], B[2, i + 1, 0]) - 1
                    best[0] = np.maximum(best[0], step)
                    best[2] = np.maximum(best[2], step)
                else:                                             # into X
                    x = B[1, i + 1, j]
                    best[0] = np.maximum(best[0], x + gox + gex)
                    best[1] = np.maximum(best[1], x + gex)
                    best[2] = np.maximum(best[2], x + gox + gex)
            for s in range(3):
                B[s, i, j] = best[s]
    return F, B


def _through(n, m, eq):
    """best score of a complete path through every cell, (n + 1, m + 1, S); NEG where none"""
    F, B = _tables(n, m, eq)
    T = np.where((F > NEG // 2) & (B > NEG // 2), F + B, NEG).max(axis=0)
    # the tables agree with each other: the best path through the origin, and through the last cell, is the best path
    best = F[:, n, m].max(axis=0)
    assert (T[0, 0] == best).all() and (T[n, m] == best).all() and (T <= best).all()
    return T


@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("tokens", ["all_equal", "random"])
def test_bound_covers_every_path_outside_the_band(native, n, m, tokens):
    rng = np.random.default_rng(1000 * n + m)
    if tokens == "all_equal":
        eq = np.ones((n, m), dtype=bool)
    else:
        t, o = rng.integers(0, 3, size=n), rng.integers(0, 3, size=m)
        eq = t[:, None] == o[None, :]
    eq = eq[:, :, None]                                           # against the systems' axis
    T = _through(n, m, eq)
    diag = np.arange(m + 1)[None, :] - np.arange(n + 1)[:, None]
    prm = np.ascontiguousarray(SYSTEMS, dtype=np.int32)
    checked = 0
    for w in range(0, max(n, m) + 1):
        lo, hi = min(0, m - n) - w, max(0, m - n) + w
        outside = (diag < lo) | (diag > hi)
        if not outside.any():
            continue
        worst = T[outside].max(axis=0)                            # per system
        U = np.array([native.lib.ta_nw2_band_bound(n, m, prm[k].ctypes.data, w) for k in range(len(prm))])
        bad = np.nonzero(worst > U)[0]
        assert bad.size == 0, (n, m, w, SYSTEMS[bad[0]].tolist(), int(worst[bad[0]]), int(U[bad[0]]))
        checked += 1
    assert checked >= 1


def test_bound_default_system_closed_form(native):
    """n = m under the default system: U(w) = 8 n - 9 (w + 1)"""
    prm = np.array(DEFAULT_SYS, dtype=np.int32)
    for n, w in [(4096, 1820), (1100, 64), (1100, 488)]:
        assert native.lib.ta_nw2_band_bound(n, n, prm.ctypes.data, w) == 8 * n - 9 * (w + 1)


def test_plan_rule_and_declines(native):
    """ta_nw2_band_plan: the rule's width (smallest w with U(w) < 1/2 a min(n, m)), and the cases it leaves to the
    full fill"""
    lib = native.lib
    flags = (28 << native.TA_NW_ALPHABET_SHIFT) | native.TA_NW_OPENS_SAME | native.TA_NW_CODES8

    def plan(n, m, nprob, system=DEFAULT_SYS, band=0, fl=flags):
        n32, m32 = np.full(nprob, n, np.int32), np.full(nprob, m, np.int32)
        p = np.array(system, dtype=np.int32)
        out, u, r = np.zeros(8, np.int32), np.zeros(nprob, np.int32), np.zeros(2 * 64, np.int32)
        assert lib.ta_nw2_band_plan(n32.ctypes.data, m32.ctypes.data, nprob, p.ctypes.data, 0, fl, band, out.ctypes.data,
                                    u.ctypes.data, r.ctypes.data, len(r)) == 0
        return out, u, r

    prm = np.array(DEFAULT_SYS, dtype=np.int32)
    out, u, r = plan(4096, 4096, 4096)
    w = int(out[0])
    assert w == out[1] == 1820 and out[2] < 800 and out[3] == 16
    assert 2 * lib.ta_nw2_band_bound(4096, 4096, prm.ctypes.data, w) < 8 * 4096 <= 2 * lib.ta_nw2_band_bound(4096, 4096, prm.ctypes.data, w - 1)
    assert (u == lib.ta_nw2_band_bound(4096, 4096, prm.ctypes.data, w)).all()
    ranges = r[:32].reshape(16, 2)
    assert (ranges % 16 == 0).all() and (ranges[:, 0] < ranges[:, 1]).all() and ranges[0, 0] == 0 and ranges[-1, 0] > 0
    assert ranges[-1, 1] == (4096 + 63 + 3) // 4 and (np.diff(ranges[:, 0]) >= 0).all() and (np.diff(ranges[:, 1]) >= 0).all()
    assert plan(4096, 4096, 4096, band=1)[0][0] == 0                       # off
    assert plan(4096, 4096, 4096, band=300)[0][0] == 300                   # forced
    assert plan(1000, 4096, 64)[0][0] == 0                                 # fewer than 1024 rows
    out = plan(1100, 1100, 64)[0]
    assert out[0] == 0 and out[1] == 488 and out[2] >= 800                 # the band would run too much of the table
    assert plan(4096, 4096, 64, system=[-1, -4, -7, -7, -3, 0])[0][:2].tolist() == [0, -1]     # a <= 0
    assert plan(4096, 4096, 64, system=[1, -4, 0, 0, 2, 2])[0][:2].tolist() == [0, -1]         # gaps pay: a - cv - ch <= 0
    assert plan(4096, 4096, 64, fl=native.TA_NW_CODES8)[0][0] == 0         # no score profile: no banded kernel
