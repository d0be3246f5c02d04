"""Banded fill of the two-phase aligner on the GPU (csrc/ta_nw2.hip): whatever the band and
whether or not a problem's certificate passes, the alignment is the oracle's (oracle/nw_oracle: align_ids); the list of
problems filled again in full is exactly the problems whose banded score does not clear the bound."""
import functools

import numpy as np
import pytest

from tools.nw_configs import DEFAULT_SYS
from tools.synth import synth_pair_ids

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _pair(n, m, seed):
    return synth_pair_ids(n, m, seed)


@functools.lru_cache(maxsize=None)
def _random_pair(n, m, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 27, size=n).astype(np.int32), rng.integers(0, 27, size=m).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _shifted_pair(k):
    """t = X k + C, o = C + Y k: the best alignment runs k columns off the diagonal"""
    C = np.random.default_rng(900).integers(0, 20, size=900).astype(np.int32)
    return (np.concatenate([np.full(k, 25, np.int32), C]), np.concatenate([C, np.full(k, 26, np.int32)]))


_ORACLE = {}


def _oracle(t, o, system):
    from oracle import nw_oracle
    key = (t.tobytes(), o.tobytes(), tuple(int(v) for v in system))
    if key not in _ORACLE:
        _ORACLE[key] = nw_oracle.align_ids(t, o, [int(v) for v in system])
    return _ORACLE[key]


def _excursion(ops):
    d = np.concatenate([[0], np.cumsum((ops != 1).astype(np.int64) - (ops != 2).astype(np.int64))])
    return int(d.min()), int(d.max())


def _leaves_band(t, o, system, w):
    n, m = len(t), len(o)
    dmin, dmax = _excursion(_oracle(t, o, system))
    return dmin < min(0, m - n) - w or dmax > max(0, m - n) + w


def _host_v0(t, o, system):
    """The certificate's left side, recomputed on the host on the FULL table: the smallest of M, X, Y of the last cell
    (textSeqCompare.py:53-88).  Where the band certifies, the banded value is this one."""
    mat, mis, gox, goy, gex, gey = (int(v) for v in system)
    n, m = len(t), len(o)
    NEG = -10 ** 9
    M = -np.arange(m + 1, dtype=np.int64); X = M.copy(); Y = np.full(m + 1, NEG, dtype=np.int64)
    cols = np.arange(m, dtype=np.int64)
    sub = np.where(np.asarray(t)[:, None] == np.asarray(o)[None, :], mat, mis)
    for i in range(1, n + 1):
        Dp = np.maximum(np.maximum(M, X), Y)                    # of row i - 1
        Mn = np.empty(m + 1, dtype=np.int64); Xn = np.empty(m + 1, dtype=np.int64); Yn = np.empty(m + 1, dtype=np.int64)
        Mn[0], Xn[0], Yn[0] = -i, NEG, -i
        Mn[1:] = Dp[:-1] + sub[i - 1]
        Xn[1:] = np.maximum(np.maximum(M[1:] + gox + gex, X[1:] + gex), Y[1:] + gox + gex)
        # Y(i, j) = max over j' < j of max(M, X)(i, j') + goy + gey (j - j'), and Y(i, 0) + gey j: a running maximum
        cand = np.maximum(Mn, Xn)[:-1] + goy + gey - gey * cols
        cand[0] = max(cand[0], Yn[0] + gey)
        Yn[1:] = np.maximum.accumulate(cand) + gey * cols
        M, X, Y = Mn, Xn, Yn
    return int(min(M[m], X[m], Y[m]))


def _batch(probs, system, band, **kw):
    from text_alignment_amd import textSeqCompare as tsc
    batch = tsc.NWBatch([p[0] for p in probs], [p[1] for p in probs], system, two_phase=True)
    for k, v in kw.items():
        setattr(batch, k, v)
    batch.band = band
    return batch


def _run(probs, system, band, **kw):
    import torch
    batch = _batch(probs, system, band, **kw)
    batch.run()
    torch.cuda.synchronize()
    return batch, batch.results(), batch.band_fallbacks()


def _assert_oracle(probs, systems, res):
    for k, ((t, o), ops) in enumerate(zip(probs, res)):
        assert ops.tolist() == _oracle(t, o, systems[k]).tolist(), (k, len(t), len(o))


def _rule_w(probs, system):
    plan = _batch(probs, system, 0).band_plan()
    return plan["rule_w"]


def test_certified_band_at_the_rules_width():
    """1100 x 1100 and 1300 x 900 in one batch, w from the automatic rule for that batch (488: the widest any of its
    problems asks for; the plan itself declines a band that runs 0.8 or more of so small a table, so the width is
    forced): several strips, several checkpoint intervals, n != m, strips that start past group 0 -- and nothing falls
    back.  (1300 x 900 alone asks for w = 355, which its own score, 3391 <= U = 3596, does not certify: the 400 rows
    beyond the OCR string cost more than the rule's 1/2 a min(n, m) leaves room for; test_forced_narrow_band has it.)"""
    probs = [_pair(1100, 1100, 11), _pair(1300, 900, 12)]
    w = _rule_w(probs, DEFAULT_SYS)
    assert w == 488
    batch, res, fb = _run(probs, DEFAULT_SYS, w)
    plan = batch.band_plan()
    assert plan["w"] == w
    _assert_oracle(probs, [DEFAULT_SYS] * 2, res)
    assert any(gl > 0 for gl, gh in plan["ranges"]) and any(gh < plan["ranges"][-1][1] for gl, gh in plan["ranges"])
    assert fb == []


@pytest.mark.parametrize("w", [64, 200, 355])
def test_forced_narrow_band(w, native):
    probs = [_pair(1100, 1100, 11), _pair(1300, 900, 12)]
    batch, res, fb = _run(probs, DEFAULT_SYS, w)
    assert batch.band_plan()["w"] == w
    _assert_oracle(probs, [DEFAULT_SYS] * 2, res)
    prm = np.array(DEFAULT_SYS, dtype=np.int32)
    for k, (t, o) in enumerate(probs):
        U = native.lib.ta_nw2_band_bound(len(t), len(o), prm.ctypes.data, w)
        v0 = _host_v0(t, o, DEFAULT_SYS)
        print("w", w, "problem", k, "v0", v0, "U", U, "listed", k in fb)
        # banded <= true: a problem whose true value does not clear the bound is listed; one that is not listed cleared
        # it with its banded value, which is then the true one
        assert (k in fb) == (not v0 > U), (k, v0, U)


@pytest.mark.parametrize("k", [256 - 70, 256, 256 + 70])
def test_path_that_leaves_the_band(k):
    w = 256
    t, o = _shifted_pair(k)
    batch, res, fb = _run([(t, o)], DEFAULT_SYS, w)
    assert batch.band_plan()["w"] == w
    _assert_oracle([(t, o)], [DEFAULT_SYS], res)
    if _leaves_band(t, o, DEFAULT_SYS, w):
        assert fb == [0]
    if k > w:
        assert _leaves_band(t, o, DEFAULT_SYS, w)


def test_unrelated_pair_falls_back():
    t, o = _random_pair(1100, 1100, 5)
    batch, res, fb = _run([(t, o)], DEFAULT_SYS, 488)
    _assert_oracle([(t, o)], [DEFAULT_SYS], res)
    assert fb == [0]


def test_mixed_batch_two_systems(native):
    """six problems, certified and failing ones, a scoring system per problem (two different ones)"""
    other = [10, -5, -7, -7, -2, -2]
    probs = [_pair(1100, 1100, 11), _random_pair(1100, 1100, 5), _pair(1300, 900, 12), _pair(1100, 1100, 21),
             _random_pair(1200, 1000, 6), _pair(1024, 1153, 22)]
    systems = [DEFAULT_SYS, DEFAULT_SYS, other, other, other, DEFAULT_SYS]
    w = 600
    batch, res, fb = _run(probs, np.array(systems), w)
    assert batch.params_stride == 6 and batch.band_plan()["w"] == w
    _assert_oracle(probs, systems, res)
    expect = []
    for k, (t, o) in enumerate(probs):
        prm = np.array(systems[k], dtype=np.int32)
        U = native.lib.ta_nw2_band_bound(len(t), len(o), prm.ctypes.data, w)
        assert batch.band_plan()["u"][k] == U
        if not _host_v0(t, o, systems[k]) > U:
            expect.append(k)
    assert fb == expect and 0 < len(fb) < len(probs), (fb, expect)
    # fill and traceback as two calls: the fallback belongs to the fill half
    batch.run(fill=True, traceback=False)
    batch.run(fill=False, traceback=True)
    _assert_oracle(probs, systems, batch.results())
    assert batch.band_fallbacks() == expect


def test_band_off_and_declined_band_are_todays_fill():
    """band off gives today's results; where the plan declines the band (the rule's band would run 0.84 of this table)
    the automatic run launches exactly the full kernel: same workspace, byte for byte"""
    import torch
    probs = [_pair(1100, 1100, 11)]
    auto = _batch(probs, DEFAULT_SYS, 0)
    assert auto.band_plan()["w"] == 0 and auto.band_plan()["rule_w"] == 488 and auto.band_plan()["share"] >= 0.8
    off = _batch(probs, DEFAULT_SYS, 1)
    assert off.band_plan()["w"] == 0
    for b in (auto, off):
        b.ws.zero_()
        b.run()
    torch.cuda.synchronize()
    assert torch.equal(auto.ws, off.ws)
    _assert_oracle(probs, [DEFAULT_SYS], off.results())
    _assert_oracle(probs, [DEFAULT_SYS], auto.results())
    assert off.band_fallbacks() == [] and auto.band_fallbacks() == []


def test_automatic_band_on_a_large_problem():
    """the plan's own choice where it does band: 2 x 3000 x 3000 (w = 1332, 0.77 of the groups), one related pair that
    certifies and one unrelated pair that falls back"""
    probs = [_pair(3000, 3000, 31), _random_pair(3000, 3000, 32)]
    batch, res, fb = _run(probs, DEFAULT_SYS, 0)
    plan = batch.band_plan()
    assert plan["w"] == plan["rule_w"] > 0 and plan["share"] < 0.8
    _assert_oracle(probs, [DEFAULT_SYS] * 2, res)
    assert fb == [1]
