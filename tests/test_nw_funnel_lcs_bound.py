"""funnel_suf_lcs (csrc/nw_band.h) without a GPU, on small problems against exhaustive tables (test_nw_band_bound's
forward + backward recurrences), for the 729 systems of the reference's grid search and the default one:

* for every interior cell, the true best score of the remainder (any state) <= SufL(rn, rm, L(i, j)) <= Suf(rn, rm),
  L the suffix LCS of the two strings from a plain table; where mismatch >= match, SufL = Suf;
* the exit bound with SufL -- every border cell under ITS OWN count for all three neighbours, as the kernels take it --
  is at least what any complete path through a cell outside the region scores, on random and funnel-shaped regions;
* wherever v0 clears that bound, the walk over the banded tables is the walk over the full ones."""
import numpy as np
import pytest

from test_nw_band_bound import NEG, SYSTEMS, _tables
from test_nw_funnel_bound import _banded_forward, _pairs, _regions, _regions_that_can_certify, _walk

SHAPES = [(5, 17), (13, 12), (16, 16), (12, 9)]
CERTIFIED_FLOOR = 100


def _suffix_lcs(t, o):
    n, m = len(t), len(o)
    L = np.zeros((n + 2, m + 2), dtype=np.int64)
    for i in range(n - 1, -1, -1):
        for j in range(m - 1, -1, -1):
            L[i, j] = max(L[i + 1, j], L[i, j + 1], L[i + 1, j + 1] + (t[i] == o[j]))
    return L


@pytest.mark.parametrize("n,m", SHAPES)
def test_lcs_bounded_suffix_and_exit_bound(native, n, m):
    rng = np.random.default_rng(91000 + 100 * n + m)
    S = len(SYSTEMS)
    prm = np.ascontiguousarray(SYSTEMS, dtype=np.int32)
    suf = np.zeros((n + 2, m + 2, S), dtype=np.int64)
    ap = np.zeros(S, dtype=np.int64)
    for k in range(S):
        a_out = np.zeros(1, dtype=np.int32)
        for rn in range(n + 1):
            for rm in range(m + 1):
                suf[n - rn, m - rm, k] = native.lib.ta_nw2_funnel_suf(rn, rm, prm[k].ctypes.data, a_out.ctypes.data)
        ap[k] = a_out[0]
    certified = walked = tighter = 0
    for t, o in _pairs(n, m, rng):
        L = _suffix_lcs(t, o)
        eq2 = t[:, None] == o[None, :]
        eq = eq2[:, :, None]
        F, B = _tables(n, m, eq)
        T = np.where((F > NEG // 2) & (B > NEG // 2), F + B, NEG).max(axis=0)
        # sufl[i, j, k] = SufL(n - i, m - j, L(i, j)), the library's
        sufl = np.zeros((n + 2, m + 2, S), dtype=np.int64)
        for k in range(S):
            for i in range(n + 1):
                for j in range(m + 1):
                    sufl[i, j, k] = native.lib.ta_nw2_funnel_suf_lcs(n - i, m - j, int(L[i, j]), prm[k].ctypes.data)
        assert (sufl <= suf).all()
        assert (B[:, 1:, 1:] <= sufl[None, 1:n + 1, 1:m + 1]).all()          # the true remainder, every cell, every state
        flat = SYSTEMS[:, 1] >= SYSTEMS[:, 0]
        assert (sufl[:, :, flat] == suf[:, :, flat]).all()
        tighter += int((sufl < suf).sum())
        for inside in list(_regions(n, m, rng, 4)) + list(_regions_that_can_certify(n, m, T, rng)):
            Fb = _banded_forward(n, m, eq, inside)
            Db = Fb.max(axis=0)
            in_or_bnd = inside.copy(); in_or_bnd[0, :] = True; in_or_bnd[:, 0] = True
            outside = ~in_or_bnd
            if not outside.any():
                continue
            xhat = np.full(S, NEG, dtype=np.int64)
            for di, dj in ((0, 1), (1, 0), (1, 1)):
                src = in_or_bnd[:n + 1 - di, :m + 1 - dj] & outside[di:, dj:]
                if not src.any():
                    continue
                ci, cj = np.nonzero(src)
                for i, j in zip(ci.tolist(), cj.tolist()):                # the neighbour's remainder under the BORDER cell's count
                    rn, rm, l = n - (i + di), m - (j + dj), int(L[i, j])
                    rest = np.array([native.lib.ta_nw2_funnel_suf_lcs(rn, rm, l, prm[k].ctypes.data) for k in range(S)])
                    xhat = np.maximum(xhat, Db[i, j] + ap + rest)
            worst = T[outside].max(axis=0)
            bad = np.nonzero(worst > xhat)[0]
            assert bad.size == 0, (n, m, SYSTEMS[bad[0]].tolist(), int(worst[bad[0]]), int(xhat[bad[0]]))
            v0 = Fb[:, n, m].min(axis=0)
            ok = np.nonzero(v0 > xhat)[0]
            certified += ok.size
            for k in ok.tolist():
                assert (Fb[:, n, m, k] == F[:, n, m, k]).all()
                assert _walk(Fb, k, eq2, n, m) == _walk(F, k, eq2, n, m), (n, m, SYSTEMS[k].tolist())
                walked += 1
    print("n", n, "m", m, "certified", certified, "walks compared", walked, "cells where SufL < Suf", tighter)
    assert certified >= CERTIFIED_FLOOR and walked == certified and tighter > 0, (n, m, certified, walked, tighter)
