"""The page-scope confidence checker tests/forced_page_conf_ref.py against the enumeration of all
legal paths of tiny pages, and the properties the rule promises on every page of tests/forced_page_cases.py."""
import numpy as np
import pytest

import forced_conf_ref as LR
import forced_page_cases as C
import forced_page_conf_cases as CC
import forced_page_conf_ref as R
import forced_page_ref as PR


def _tiny(rng, ties):
    nl, n = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    Ts = [int(rng.integers(1, 4)) for _ in range(nl)]
    no = 4
    while True:                                        # random legal windows
        lo = np.sort(rng.integers(0, n + 1, size=nl))
        hi = np.sort(rng.integers(0, n + 1, size=nl))
        lo[0], hi[-1] = 0, n
        if PR.windows_ok(lo, hi, n):
            break
    Ps = [np.full((T, no), 0.25, np.float32) if ties else C.probs(rng, T, no) for T in Ts]
    return Ps, C.text(rng, n, no), [int(v) for v in lo], [int(v) for v in hi]


def _enumerate(Ps, cs, lo, hi):
    """best[(f, s)] = the largest path_score over all legal paths that spend frame f in state s"""
    order = [(k, t) for k, P in enumerate(Ps) for t in range(len(P))]
    S, F = 2 * len(cs) + 1, len(order)
    best = {}

    def walk(path):
        if len(path) == F:
            total = PR.path_score(Ps, cs, lo, hi, [(k, t, s) for (k, t), s in zip(order, path)])
            if total is not None:
                for f, s in enumerate(path):
                    best[f, s] = max(best.get((f, s), total), total)
            return
        left = F - len(path) - 1                       # frames behind the one to add: the end must stay in reach
        for s in range(path[-1], min(path[-1] + 2, S - 1) + 1):
            if s + 2 * left >= S - 2:
                walk(path + [s])

    for s0 in (0, 1):
        if s0 + 2 * (F - 1) >= S - 2:
            walk([s0])
    return order, best


def test_every_entry_of_G_equals_the_enumeration_of_all_legal_paths():
    rng = np.random.default_rng(1413)
    with_path = 0
    for trial in range(96):
        Ps, cs, lo, hi = _tiny(rng, ties=trial % 4 == 0)
        order, best = _enumerate(Ps, cs, lo, hi)
        G = R.tables(Ps, cs, lo, hi)[2]
        for f, (k, t) in enumerate(order):
            for s in range(2 * len(cs) + 1):
                assert int(G[k][t, s]) == best.get((f, s), R.NEG), (trial, k, t, s)
        with_path += bool(best)
    assert with_path >= 48                             # the windows and frame counts leave most pages a path


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_the_properties_of_the_rule_on_every_page(case):
    name, no, pages = case
    aligned = C.want(name, pages)
    got = CC.want(name, pages)
    for p, ((Ps, cs, lo, hi), (status, score, frames), G) in enumerate(zip(pages, aligned, CC.tables(name, pages))):
        if status != PR.OK:
            assert G is None and got["peak"][p][0] == status
            continue
        Ts = [len(P) for P in Ps]
        assert R.queries_ok(frames[:, 0], frames[:, 3], Ts, lo, hi)               # sorted, and the own states live
        _, ql, qt, conf, rival, own = got["peak"][p]
        assert (own == score).all() and (conf >= 0).all()
        for k, g in enumerate(G):
            assert (g.max(axis=1) == score).all(), (p, k)
            assert (g[:, :2 * lo[k]] == R.NEG).all() and (g[:, 2 * hi[k] + 1:] == R.NEG).all()
        for which in CC.SETS:
            _, ql, qt, conf, rival, own = got[which][p]
            assert R.queries_ok(ql, qt, Ts, lo, hi)
            for i in range(len(cs)):
                k = int(ql[i])
                assert 2 * lo[k] <= rival[i] <= 2 * hi[k] and rival[i] != 2 * i + 1
                assert own[i] - conf[i] == G[k][int(qt[i]), rival[i]]
                if own[i] - conf[i] == R.NEG:
                    assert rival[i] == 2 * lo[k]


def test_a_zero_confidence_and_an_unreachable_rival_both_occur():
    zero = none = chars = with_path = 0
    for name, no, pages in C.cases():
        for w in CC.want(name, pages)["peak"]:
            if w[0] == PR.OK:
                with_path += 1
                chars += len(w[3])
                zero += int((w[3] == 0).sum())
                none += int((w[5] - w[3] == R.NEG).sum())
    assert with_path == 56 and chars == 4424
    assert zero == 15 and none == 14


def test_a_page_of_one_line_is_the_line_rule():
    seen = 0
    for name, no, pages in C.cases():
        for (Ps, cs, lo, hi), w in zip(pages, CC.want(name, pages)["seeded"]):
            if len(Ps) == 1 and w[0] == PR.OK and 2 * len(cs) + 1 <= len(Ps[0]):
                assert list(lo) == [0] and list(hi) == [len(cs)]
                conf, rival = LR.query(Ps[0], cs, w[2])
                assert np.array_equal(conf, w[3]) and np.array_equal(rival, w[4])
                seen += 1
    assert seen >= 8


def test_queries_the_kernel_refuses_are_a_value_error():
    rng = np.random.default_rng(3)
    Ps, cs, lo, hi = C._page(rng, (10, 9, 11), 9, (0, 1, 6), (5, 6, 9), 7)
    G = R.tables(Ps, cs, lo, hi)[2]
    ql, qt = CC.seeded_queries(rng, [10, 9, 11], 9, lo, hi)
    R.query_tables(G, lo, hi, ql, qt)
    for i, k, t in ((0, -1, 0), (8, 3, 0), (2, int(ql[2]), -1), (2, int(ql[2]), 11), (0, 2, 0), (8, 0, 9), (5, 0, 0)):
        bl, bt = ql.copy(), qt.copy()
        bl[i], bt[i] = k, t
        with pytest.raises(ValueError):
            R.query_tables(G, lo, hi, bl, bt)
    with pytest.raises(ValueError):
        R.query_tables(G, lo, hi, ql[:-1], qt[:-1])
