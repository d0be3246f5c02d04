"""The chained span search's checker (tests/span_chain_ref.py) against statements that know nothing of carries: the
exhaustive maximum over monotone span tuples of span_ref's per-start fills, span_ref's single search for a chain of one
page, its numpy form, and the repeated-passage example the chain exists for."""
import numpy as np

import span_cases as C
import span_chain_ref as CH
import span_ref as R

DEFAULT = [8, -12, -6, -6, -2, -2]
SYSTEMS = [DEFAULT, C.SYSTEMS[0], C.SYSTEMS[3], C.SYSTEMS[4]]


def _floor(t, pages, system):
    """what the Python layer passes: the call's score_bound"""
    return (len(t) + max([len(o) for o in pages] + [0]) + 2) * (3 * max(abs(v) for v in system) + 2)


def _random_chain(seed):
    rng = np.random.RandomState(seed)
    n = 0 if seed % 29 == 0 else int(rng.randint(0, 8))
    t = rng.randint(0, 3, size=n).tolist()
    pages = []
    for p in range(1 + seed % 3):
        m = 0 if (seed + p) % 11 == 0 else int(rng.randint(0, 5))
        o = rng.randint(0, 3, size=m).tolist()
        if n >= 2 and m >= 1 and (seed + p) % 3 == 0:      # a page cut from the transcript
            a = int(rng.randint(0, n - 1))
            o = t[a:a + m]
        pages.append(o)
    return t, pages, SYSTEMS[seed % len(SYSTEMS)]


def _exhaustive_total(t, pages, system):
    """max of sum_p S_p(i0_p, i1_p) over i0_0 <= i1_0 <= i0_1 <= ... <= n; S_p(i0, i1) = span_enumerate's per-start fill
    (column 0 below i0 unreachable).  Every tuple is covered: B_p(x) = the best of pages 0 .. p ending at or before x."""
    n = len(t)
    before = [0] * (n + 1)
    for o in pages:
        m = len(o)
        S = {}
        for i0 in range(n + 1):
            M, X, Y = R._fill(t, o, system, i0, False)
            for i1 in range(i0, n + 1):
                S[i0, i1] = max(M[i1][m], X[i1][m], Y[i1][m])[0]
        ending = [max(before[i0] + S[i0, i1] for i0 in range(i1 + 1)) for i1 in range(n + 1)]
        before = [max(ending[:x + 1]) for x in range(n + 1)]
    return before[n]


def test_total_is_the_exhaustive_maximum_and_the_floor_does_not_bind():
    for seed in range(300):
        t, pages, system = _random_chain(seed)
        spans, total, bound = CH.chain_plain(t, pages, system, _floor(t, pages, system))
        assert not bound, seed
        assert total == _exhaustive_total(t, pages, system), (seed, t, pages, system)
        limit = 0
        for i0, i1, _ in spans:                             # reading order
            assert limit <= i0 <= i1 <= len(t), (seed, spans)
            limit = i1


def test_a_chain_of_one_page_is_the_single_search():
    for seed in range(420):
        t, o, system = C.small_case(seed)
        spans, total, bound = CH.chain_plain(t, [o], system, _floor(t, [o], system))
        assert spans == [R.span_origins(t, o, system)] and total == spans[0][2] and not bound, seed


def test_numpy_form_equals_plain_form():
    for seed in range(200):
        t, pages, system = _random_chain(seed)
        for floor in (_floor(t, pages, system), 3):
            assert CH.chain_numpy(t, pages, system, floor) == CH.chain_plain(t, pages, system, floor), (seed, floor)
    rng = np.random.RandomState(9)
    t = rng.randint(0, 4, size=90)
    pages = [t[5:30].copy(), np.zeros(0, np.int64), rng.randint(0, 4, size=17), t[50:81].copy()]
    for system in C.SYSTEMS:
        assert CH.chain_numpy(t, pages, system, 4000) == CH.chain_plain(t, pages, system, 4000)


def repeated_passage(seed=3):
    """filler(30) + word + a + b + word + filler(30), |word| = 40, |a| = |b| = 60; the pages are a, b and the SECOND word"""
    rng = np.random.RandomState(seed)
    filler = lambda k: rng.randint(4, 8, size=k)
    word, a, b = rng.randint(0, 4, size=40), rng.randint(8, 12, size=60), rng.randint(12, 16, size=60)
    t = np.concatenate([filler(30), word, a, b, word, filler(30)])
    return t, [a, b, word]


def test_repeated_passage_goes_to_its_own_copy():
    t, pages = repeated_passage()
    alone = [R.span_numpy(t, o, DEFAULT)[:2] for o in pages]
    assert alone == [(70, 130), (130, 190), (30, 70)]       # the independent search: the FIRST copy, out of order
    spans, total, bound = CH.chain_numpy(t, pages, DEFAULT, _floor(t, pages, DEFAULT))
    assert [s[:2] for s in spans] == [(70, 130), (130, 190), (190, 230)]
    assert [s[2] for s in spans] == [8 * 60, 8 * 60, 8 * 40] and total == 8 * 160 and not bound


def test_ordered_pages_keep_their_own_scores():
    tr, _, _ = C.planted(21, 0, 600, 0, 1.0)
    rng = np.random.RandomState(22)
    cuts = [(20, 150), (170, 300), (300, 420), (450, 590)]
    ocr = [C.noisy(rng, tr[a:b], 0.85) for a, b in cuts]
    t, *pages = C.codes(tr, *ocr)
    for system in (DEFAULT, C.SYSTEMS[1]):
        alone = [R.span_numpy(t, o, system) for o in pages]
        assert all(alone[k][1] <= alone[k + 1][0] for k in range(len(alone) - 1))
        spans, total, bound = CH.chain_numpy(t, pages, system, _floor(t, pages, system))
        assert [s[2] for s in spans] == [a[2] for a in alone] and total == sum(a[2] for a in alone) and not bound


def test_a_floor_that_binds():
    bound_seen = 0
    for seed in range(120):
        t, pages, system = _random_chain(seed)
        got = CH.chain_numpy(t, pages, system, 5)
        assert got == CH.chain_plain(t, pages, system, 5), seed
        bound_seen += got[2]
    assert bound_seen > 10
    t, pages = repeated_passage()
    spans, total, bound = CH.chain_numpy(t, pages, DEFAULT, 5)
    assert bound and (spans, total, bound) == CH.chain_plain(t, pages, DEFAULT, 5)
