"""The checker of the page-scope posteriors (tests/forced_page_post_ref.py) against itself and
against exact arithmetic, without a GPU: its vectorised form bit-equal to its integer form, both against the enumeration of
all legal paths in fractions.Fraction, the posteriors of a frame summing to one, a page of one line against the line rule,
Z = 0 against the aligner's NOPATH, what holds at the aligner's own peaks, and the rule of the line break.  float32
probabilities are dyadic, so every exact value here is a rational with a power of two below."""
from fractions import Fraction

import numpy as np
import pytest

import forced_page_cases as C
import forced_page_post_cases as PC
import forced_page_post_ref as R
import forced_page_ref as PR
import forced_post_ref as LR
import forced_ref as R0

U = Fraction(1, 1 << 53)


def _exact(m, x):
    """the rational a pair stands for"""
    return Fraction(float(m)) * Fraction(2) ** int(x)


def _frexp_form(gm, gx):
    return all((((m == 0) | ((m >= 0.5) & (m < 1))).all() and (x[m == 0] == 0).all()) for m, x in zip(gm, gx))


def test_the_vectorised_form_equals_the_integer_form_bit_for_bit():
    seen = 0
    for name, no, pages in C.cases():
        for Ps, cs, lo, hi in pages:
            if sum(len(P) for P in Ps) > 40:
                continue
            a, b = R.tables(Ps, cs, lo, hi), R.tables_exact(Ps, cs, lo, hi)
            for k in range(len(Ps)):
                assert R.same_bits(a[0][k], b[0][k]) and np.array_equal(a[1][k], b[1][k]), (name, k)
            assert R.same_bits([a[2]], [b[2]]) and a[3] == b[3], name
            assert _frexp_form(a[0], a[1])
            seen += 1
    assert seen >= 30


def _tiny(rng, ties):
    """at most 3 lines x 3 frames and 3 characters, random legal windows; rows of 0 / NaN now and then"""
    nl, n = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    Ts = [int(rng.integers(1, 4)) for _ in range(nl)]
    no = 4
    while True:
        lo = np.sort(rng.integers(0, n + 1, size=nl))
        hi = np.sort(rng.integers(0, n + 1, size=nl))
        lo[0], hi[-1] = 0, n
        if PR.windows_ok(lo, hi, n):
            break
    Ps = [np.full((T, no), 0.25, np.float32) if ties else C.probs(rng, T, no) for T in Ts]
    if not ties and rng.random() < 0.4:
        k = int(rng.integers(0, nl))
        Ps[k][int(rng.integers(0, Ts[k]))] = 0.0
        k = int(rng.integers(0, nl))
        Ps[k][int(rng.integers(0, Ts[k]))] = np.nan
    return Ps, C.text(rng, n, no), [int(v) for v in lo], [int(v) for v in hi]


def _legal_paths(Ps, cs, lo, hi, legal):
    """every path, a state per frame, that legal(path as [(line, t, state)]) allows"""
    order = [(k, t) for k, P in enumerate(Ps) for t in range(len(P))]
    S, F = 2 * len(cs) + 1, len(order)
    out = []

    def walk(path):
        if len(path) == F:
            if legal([(k, t, s) for (k, t), s in zip(order, path)]):
                out.append(tuple(path))
            return
        for s in range(path[-1], min(path[-1] + 2, S - 1) + 1):
            walk(path + [s])

    walk([0])
    walk([1])
    return order, out


def _masses(Ps, cs, order, paths):
    """(g[f][s], Z) in Fraction from the paths' products of emissions"""
    lab = R0.states(cs)
    E = [LR.emission(P) for P in Ps]
    S = len(lab)
    g = [[Fraction(0)] * S for _ in order]
    Z = Fraction(0)
    for path in paths:
        mass = Fraction(1)
        for (k, t), s in zip(order, path):
            mass *= Fraction(float(E[k][t, lab[s]]))
        Z += mass
        for f, s in enumerate(path):
            g[f][s] += mass
    return g, Z


def test_both_forms_against_the_enumeration_of_all_legal_paths():
    """section 14.11's bound with its derivation: a value is a sum of products of non-negative terms, each of the at most
    3 F + 2 roundings on the way to it moves it by a relative 2^-53 at the most, so g and Z lie within 4 F 2^-53"""
    rng = np.random.default_rng(1415)
    with_path = 0
    worst = Fraction(0)
    for trial in range(96):
        Ps, cs, lo, hi = _tiny(rng, ties=trial % 4 == 0)
        order, paths = _legal_paths(Ps, cs, lo, hi, lambda p: PR.path_score(Ps, cs, lo, hi, p) is not None)
        g, Z = _masses(Ps, cs, order, paths)
        F = len(order)
        bound = 4 * F * U
        for form in (R.tables, R.tables_exact):
            gm, gx, zm, zx = form(Ps, cs, lo, hi)
            assert abs(_exact(zm, zx) - Z) <= bound * Z, trial
            assert (zm == 0) == (not paths) and (zx == 0 or zm != 0)
            for f, (k, t) in enumerate(order):
                for s in range(2 * len(cs) + 1):
                    got = _exact(gm[k][t, s], gx[k][t, s])
                    assert abs(got - g[f][s]) <= bound * g[f][s], (trial, k, t, s)      # exactly zero where there is no path
                    if g[f][s]:
                        worst = max(worst, abs(got - g[f][s]) / g[f][s])
        with_path += bool(paths)
    assert with_path >= 48
    print("worst relative error against the enumeration %.3g" % float(worst))


_TABLES = {}


def _tables(name, pages):
    if name not in _TABLES:
        _TABLES[name] = [R.tables(*pg) for pg in pages]
    return _TABLES[name]


def _frame_total(m, x):
    """sum_s m[s] 2^x[s] as (integer, exponent): exact but for the terms more than 1100 binades below the largest, which
    together are below S 2^-1100 of it -- nothing against a bound of F 2^-50"""
    have = m != 0
    M, X = np.ldexp(m[have], 53).astype(np.int64), x[have]
    keep = X > X.max() - 1100
    low = int(X[keep].min())
    return sum(int(a) << (int(b) - low) for a, b in zip(M[keep], X[keep])), low - 53


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_the_posteriors_of_every_frame_sum_to_one(case):
    name, no, pages = case
    for p, ((Ps, cs, lo, hi), (gm, gx, zm, zx)) in enumerate(zip(pages, _tables(name, pages))):
        if zm == 0:
            continue
        F = sum(len(P) for P in Ps)
        Z = _exact(zm, zx)
        worst = Fraction(0)
        for k in range(len(Ps)):
            assert (gm[k][:, :2 * lo[k]] == 0).all() and (gm[k][:, 2 * hi[k] + 1:] == 0).all()     # nothing outside the window
            for m, x in zip(gm[k], gx[k]):
                total, e = _frame_total(m, x)
                worst = max(worst, abs(Fraction(total) * Fraction(2) ** e / Z - 1))
        print("%s, page %d, %d frames: worst |sum g / Z - 1| = %.3g" % (name, p, F, float(worst)))
        assert worst <= 8 * F * U, (name, p)


def test_a_page_of_one_line_is_the_line_rule_bit_for_bit():
    seen = 0
    for name, no, pages in C.cases():
        for (Ps, cs, lo, hi), w in zip(pages, PC.want(name, pages)["seeded"]):
            if len(Ps) == 1 and 2 * len(cs) + 1 <= len(Ps[0]):
                assert list(lo) == [0] and list(hi) == [len(cs)] and w["status"] == PR.OK
                line = LR.query(Ps[0], cs, w["frame"])
                for key in R.PER_LABEL:
                    assert np.asarray(line[key]).tobytes() == np.asarray(w[key], R.DTYPES[key]).tobytes(), (name, key)
                assert R.same_bits([line["z_m"]], [w["z_m"]]) and line["z_x"] == w["z_x"]
                seen += 1
    assert seen >= 8


def test_z_is_zero_exactly_where_the_aligner_finds_no_path():
    nopath = 0
    for name, no, pages in C.cases():
        for (status, _, _), (gm, gx, zm, zx) in zip(C.want(name, pages), _tables(name, pages)):
            assert (zm == 0) == (status == PR.NOPATH), name
            assert status in (PR.OK, PR.NOPATH)
            if zm == 0:
                assert zx == 0 and all((m == 0).all() for m in gm)
                nopath += 1
    assert nopath == 2
    pages = dict((c[0], c[2]) for c in C.cases())["no path"]
    for (status, _, _), w in zip(C.want("no path", pages), PC.want("no path", pages)["peak"]):
        assert w["status"] == status and (status == PR.OK) == ("own_m" in w)


def test_at_the_aligners_own_peaks_the_posterior_is_positive_and_at_most_one():
    seen = 0
    for name, no, pages in C.cases():
        for (Ps, cs, lo, hi), w in zip(pages, PC.want(name, pages)["peak"]):
            if w["status"] != PR.OK:
                continue
            F = sum(len(P) for P in Ps)
            post = R.posterior(w["own_m"], w["own_x"], w["z_m"], w["z_x"])
            assert (w["own_m"] > 0).all(), name
            assert (post > 0).all() and (post <= 1 + 8 * F * 2.0 ** -53).all(), name
            rival = R.posterior(w["rival_m"], w["rival_x"], w["z_m"], w["z_x"])
            assert (rival >= 0).all() and (post + rival <= 1 + 16 * F * 2.0 ** -53).all(), name
            assert R.loglik_bits(w["z_m"], w["z_x"]) < 0
            for i, (k, s) in enumerate(zip(w["line"], w["rival_state"])):
                assert 2 * lo[k] <= s <= 2 * hi[k] and s != 2 * i + 1
                if w["rival_m"][i] == 0:
                    assert s == 2 * lo[k] and w["rival_x"][i] == 0
            seen += 1
    assert seen == 56


def test_no_mass_keeps_a_character_over_the_line_break():
    """break_case(): one character, two lines of two frames.  The restatement that allows the stay (line_stay=True) sums
    every path of the plain lattice; the rule's Z lacks exactly the paths that spend (0, 1) and (1, 0) in state 1"""
    Ps, cs, lo, hi = C.break_case()
    F, bound = 4, 4 * 4 * U
    # the plain lattice of one character: stay or advance, no skip; ends in the character or the last blank
    order, plain = _legal_paths(Ps, cs, lo, hi, lambda p: p[-1][2] in (1, 2) and all(b[2] - a[2] <= 1 for a, b in zip(p, p[1:])))
    over = [p for p in plain if p[1] == 1 and p[2] == 1]
    assert len(plain) == 10 and len(over) == 4
    g_rule, Z_rule = _masses(Ps, cs, order, [p for p in plain if p not in over])
    g_all, Z_all = _masses(Ps, cs, order, plain)
    for form in (R.tables, R.tables_exact):
        gm, gx, zm, zx = form(Ps, cs, lo, hi)
        sm, sx, szm, szx = form(Ps, cs, lo, hi, line_stay=True)
        assert abs(_exact(zm, zx) - Z_rule) <= bound * Z_rule and abs(_exact(szm, szx) - Z_all) <= bound * Z_all
        missing = _exact(szm, szx) - _exact(zm, zx)
        assert abs(missing - (Z_all - Z_rule)) <= bound * Z_all and missing > Z_all / 2       # the likely paths are the forbidden ones
        for f, (k, t) in enumerate(order):
            for s in range(3):
                assert abs(_exact(gm[k][t, s], gx[k][t, s]) - g_rule[f][s]) <= bound * g_rule[f][s]
                assert abs(_exact(sm[k][t, s], sx[k][t, s]) - g_all[f][s]) <= bound * g_all[f][s]
    # and the aligner's own frames of that page qualify as queries
    w = PC.want("line break", [C.break_case()])["peak"][0]
    assert w["status"] == PR.OK and R.posterior(w["own_m"], w["own_x"], w["z_m"], w["z_x"])[0] > 0


def test_queries_the_kernel_refuses_are_a_value_error():
    rng = np.random.default_rng(3)
    Ps, cs, lo, hi = C._page(rng, (10, 9, 11), 9, (0, 1, 6), (5, 6, 9), 7)
    gm, gx = R.tables(Ps, cs, lo, hi)[:2]
    ql, qt = PC.seeded_queries(rng, [10, 9, 11], 9, lo, hi)
    R.query_tables(gm, gx, lo, hi, ql, qt)
    for i, k, t in ((0, -1, 0), (8, 3, 0), (2, int(ql[2]), -1), (2, int(ql[2]), 11), (0, 2, 0), (8, 0, 9), (5, 0, 0)):
        bl, bt = ql.copy(), qt.copy()
        bl[i], bt[i] = k, t
        with pytest.raises(ValueError):
            R.query_tables(gm, gx, lo, hi, bl, bt)
    with pytest.raises(ValueError):
        R.query_tables(gm, gx, lo, hi, ql[:-1], qt[:-1])


def test_the_host_formulas():
    assert R.posterior(0.5, 3, 0.5, 5) == 0.25 and R.posterior(0.0, 0, 0.75, -9000) == 0.0
    assert R.loglik_bits(0.5, -99) == -100.0
