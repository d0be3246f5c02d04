"""The confidence checker tests/forced_conf_ref.py against what it claims to compute: every
path of tiny lattices enumerated, and the aligner's own answers (tests/forced_ref.py) on every line of
tests/forced_cases.py.  No GPU, no native code."""
import itertools

import numpy as np
import pytest

import forced_cases as C0
import forced_conf_cases as C
import forced_conf_ref as R
import forced_ref as R0


def _brute(P, cs):
    """G by enumeration: per (t, s) the largest total over EVERY allowed path that is in state s at frame t, NEG if none"""
    T, S = len(P), 2 * len(cs) + 1
    G = np.full((T, S), R.NEG, dtype=np.int64)
    # every walk by steps of 0 / 1 / 2 from state 0 or 1; path_score says which of them are paths
    for first, steps in itertools.product((0, 1), itertools.product((0, 1, 2), repeat=T - 1)):
        path = np.cumsum((first,) + steps)
        total = R0.path_score(P, cs, path) if path[-1] < S else None
        if total is not None:
            G[np.arange(T), path] = np.maximum(G[np.arange(T), path], total)
    return G


def test_the_checker_equals_brute_force_enumeration_on_tiny_lattices():
    rng = np.random.default_rng(1411)
    texts = [[1], [2], [1, 2], [2, 1], [1, 1], [2, 2], [3, 1]]
    seen = 0
    for n in range(30):
        cs = texts[n % len(texts)]
        L = len(cs)
        T = int(rng.integers(2 * L + 1, 2 * L + 4))
        P = C0.probs(rng, T, 4, sharp=2.0)
        if n % 5 == 0:
            P[:] = 0.25                                  # ties everywhere: the smallest-state rule decides
        G = R.tables(P, cs)[2]
        want = _brute(P, cs)
        assert np.array_equal(G, want), (n, cs, T)
        for tq in itertools.product(range(T), repeat=L):
            conf, rival, own = R.query_tables(G, tq)
            for i, t in enumerate(tq):
                others = [(int(want[t, s]), s) for s in range(2 * L + 1) if s != 2 * i + 1]
                best = max(g for g, _ in others)
                assert own[i] == want[t, 2 * i + 1] and conf[i] == int(want[t, 2 * i + 1]) - best
                assert rival[i] == min(s for g, s in others if g == best)
                seen += 1
    assert seen > 1000


@pytest.mark.parametrize("case", C0.cases(), ids=lambda c: c[0])
def test_at_the_aligners_peaks_own_is_the_score_and_confidence_is_not_negative(case):
    name, no, lines = case
    frames, score = C0.want(name, lines)
    at = 0
    for k, (P, cs) in enumerate(lines):
        L = len(cs)
        A, B, G = R.tables(P, cs)
        assert (G.max(axis=1) == score[k]).all()         # some state of the best path holds every frame
        conf, rival, own = R.query_tables(G, frames[at:at + L, 2])
        assert (own == score[k]).all() and (conf >= 0).all()
        assert (G[frames[at:at + L, 2], rival] > R.REACH).all()      # a reachable rival always exists
        at += L
        if name == "all ties":
            assert (conf == 0).any()
    want = C.want(name, lines)["peak"]
    assert len(want[1]) == at and (want[1] >= 0).all()


def test_the_number_of_ties_on_the_shared_cases():
    ties = total = 0
    for name, no, lines in C0.cases():
        conf = C.want(name, lines)["peak"][1]
        ties += int((conf == 0).sum())
        total += len(conf)
    assert total == 6289 and ties == 9


def test_arbitrary_queries_give_signed_values():
    """t = 0 for the last character and t = T - 1 for the first: the own state cannot hold the frame (unreachable: the
    difference is NEG minus the rival) or holds it worse than a rival does"""
    rng = np.random.default_rng(1412)
    P, cs = C0.probs(rng, 30, 6), C0.text(rng, 5, 6)
    G = R.tables(P, cs)[2]
    score = R0.align(P, cs)[0]
    conf, rival = R.query(P, cs, [0, 0, 0, 0, 0])
    assert rival[0] == 0 and conf[0] == G[0, 1] - G[0, 0]
    assert (conf[1:] == R.NEG - G[0, :2].max()).all() and (conf[1:] < 0).all()
    assert set(rival[1:].tolist()) == {int(G[0, :2].argmax())}
    conf, rival = R.query(P, cs, [29] * 5)
    assert (conf[:4] == R.NEG - score).all() and (rival[:4] == int(G[29].argmax())).all()
    assert conf[4] == G[29, 9] - G[29, 10] and rival[4] == 10
    assert G[29].max() == score and int(G[29].argmax()) in (9, 10)
    # L = 1 on three frames: every query of the one character
    P1, c1 = C0.probs(rng, 3, 4), [2]
    G1 = R.tables(P1, c1)[2]
    for t in range(3):
        conf, rival = R.query(P1, c1, [t])
        assert conf[0] == G1[t, 1] - max(G1[t, 0], G1[t, 2]) and rival[0] in (0, 2)
    with pytest.raises(ValueError):
        R.query(P1, c1, [3])
    with pytest.raises(ValueError):
        R.query(P1, c1, [0, 1])


def test_seeded_queries_have_the_shape_the_cases_promise():
    rng = np.random.default_rng(3)
    for T, L in ((3, 1), (9, 4), (200, 90)):
        tq = C.seeded_queries(rng, T, L)
        assert len(tq) == L and tq[-1] == T - 1 and (np.diff(tq) >= 0).all() and (L == 1 or tq[0] == 0)
    assert (np.diff(C.seeded_queries(rng, 200, 90)) == 0).any()
