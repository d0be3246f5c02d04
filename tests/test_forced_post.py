"""The checker of the sum-product posteriors (tests/forced_post_ref.py) against itself and against
exact arithmetic, without a GPU: its vectorised form bit-equal to its integer form, both against the enumeration of all
paths in fractions.Fraction, the posteriors of a frame summing to one on long lines, and what holds at the aligner's own
peaks.  float32 probabilities are dyadic, so every exact value here is a rational with a power of two below."""
from fractions import Fraction

import numpy as np
import pytest

import forced_cases as C0
import forced_post_cases as C
import forced_post_ref as R
import forced_ref as R0

U = Fraction(1, 1 << 53)


def _exact(m, x):
    """the rational a pair stands for"""
    return Fraction(float(m)) * Fraction(2) ** int(x)


def _small_lines():
    """every line of the shared cases with T <= 40, and seeded ones up to T = 40 at both ends of L"""
    lines = [(name, P, cs) for name, _, ls in C.cases() for P, cs in ls if len(P) <= 40]
    rng = np.random.default_rng(1411)
    for T, L, no in ((40, 19, 6), (40, 1, 3), (39, 19, 128), (33, 7, 2), (17, 8, 5), (3, 1, 2)):
        lines.append(("seeded", C0.probs(rng, T, no, sharp=float(rng.integers(1, 9))), C0.text(rng, L, no)))
    return lines


def test_the_vectorised_form_equals_the_integer_form_bit_for_bit():
    lines = _small_lines()
    assert len(lines) >= 30
    for name, P, cs in lines:
        a, b = R.tables(P, cs), R.tables_exact(P, cs)
        assert R.same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, len(P), len(cs))
        assert R.same_bits([a[2]], [b[2]]) and a[3] == b[3], (name, len(P), len(cs))
        assert ((a[0] == 0) | ((a[0] >= 0.5) & (a[0] < 1))).all() and (a[1][a[0] == 0] == 0).all()    # frexp's form


def _paths(T, lab):
    """every path of the strict lattice as a tuple of states"""
    S = len(lab)
    out = []

    def walk(path):
        if len(path) == T:
            if path[-1] in (S - 1, S - 2):
                out.append(tuple(path))
            return
        s = path[-1]
        for d in (0, 1, 2):
            n = s + d
            if n < S and (d < 2 or (n % 2 == 1 and lab[n] != lab[n - 2])):
                walk(path + [n])
    walk([0])
    walk([1])
    return out


def _enumeration_lattices():
    rng = np.random.default_rng(53)
    out = []
    for cs in ([1], [1, 2], [2, 2]):
        S = 2 * len(cs) + 1
        for T in range(S, 2 * len(cs) + 4):
            for seed in range(2):
                P = C0.probs(rng, T, 3, sharp=1.0 + 4 * seed)
                out.append(("random", P, cs))
                out.append(("constant rows", np.repeat(P[:1], T, axis=0), cs))
                Q = P.copy()
                Q[rng.integers(0, T)] = 0.0
                Q[rng.integers(0, T)] = np.nan
                Q[rng.integers(0, T), rng.integers(0, 3)] = -1.0
                out.append(("zeros and NaN", Q, cs))
    return out


def test_both_forms_against_the_enumeration_of_all_paths():
    lattices = _enumeration_lattices()
    assert len(lattices) >= 40
    worst = Fraction(0)
    for kind, P, cs in lattices:
        T, S = len(P), 2 * len(cs) + 1
        lab = R0.states(cs)
        E = R.emission(P)
        g = [[Fraction(0)] * S for _ in range(T)]
        Z = Fraction(0)
        paths = _paths(T, lab)
        assert paths
        for path in paths:
            mass = Fraction(1)
            for t, s in enumerate(path):
                mass *= Fraction(float(E[t, lab[s]]))
            Z += mass
            for t, s in enumerate(path):
                g[t][s] += mass
        bound = 4 * T * U                                 # at most 3 T + 2 roundings of non-negative terms
        for form in (R.tables, R.tables_exact):
            gm, gx, zm, zx = form(P, cs)
            assert abs(_exact(zm, zx) - Z) <= bound * Z, kind
            for t in range(T):
                for s in range(S):
                    got = _exact(gm[t, s], gx[t, s])
                    assert abs(got - g[t][s]) <= bound * g[t][s], (kind, t, s)
                    if g[t][s]:
                        worst = max(worst, abs(got - g[t][s]) / g[t][s])
    print("worst relative error against the enumeration %.3g" % float(worst))


@pytest.mark.parametrize("T,L", [(5000, 70), (2047, 1023), (5000, 1023)])
def test_the_posteriors_of_a_frame_sum_to_one(T, L):
    """sum_s g[t][s] / Z at every 97th frame, exactly: the significands as integers at the row's smallest exponent, the
    ratio in Fraction"""
    rng = np.random.default_rng(T + L)
    P, cs = C0.probs(rng, T, 40), C0.text(rng, L, 40)
    frames = np.arange(0, T, 97)
    gm, gx, zm, zx = R.tables(P, cs, frames)
    Z = _exact(zm, zx)
    worst = Fraction(0)
    for m, x in zip(gm, gx):
        have = m != 0
        M, X = [int(v * (1 << 53)) for v in m[have]], [int(v) for v in x[have]]
        low = min(X)
        total = Fraction(sum(a << (b - low) for a, b in zip(M, X))) * Fraction(2) ** (low - 53)
        worst = max(worst, abs(total / Z - 1))
    print("T = %d, L = %d: worst |sum g / Z - 1| = %.3g" % (T, L, float(worst)))
    assert worst <= 8 * T * U


def test_at_the_aligners_own_peaks_the_posterior_is_positive_and_at_most_one():
    for name, _, lines in C0.cases():
        _, wanted = C.want(name, lines)["peak"]
        at = 0
        for k, (P, cs) in enumerate(lines):
            T, L = len(P), len(cs)
            own_m, own_x = wanted["own_m"][at:at + L], wanted["own_x"][at:at + L]
            post = R.posterior(own_m, own_x, wanted["z_m"][k], wanted["z_x"][k])
            assert (own_m > 0).all(), name
            assert (post > 0).all() and (post <= 1 + 8 * T * 2.0 ** -53).all(), name
            rival = R.posterior(wanted["rival_m"][at:at + L], wanted["rival_x"][at:at + L], wanted["z_m"][k], wanted["z_x"][k])
            assert (rival >= 0).all() and (post + rival <= 1 + 16 * T * 2.0 ** -53).all(), name
            assert R.loglik_bits(wanted["z_m"][k], wanted["z_x"][k]) < 0
            at += L


def test_the_host_formulas():
    assert R.posterior(0.5, 3, 0.5, 5) == 0.25 and R.posterior(0.0, 0, 0.75, -9000) == 0.0
    assert R.loglik_bits(0.5, -99) == -100.0
