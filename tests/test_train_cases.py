"""The training cases of tests/train_cases.py, held to their own conditions without any kernel: what the case builder
promises about the logadd threshold, and that the cases CAN fail -- deliberately wrong variants of the checker
(tests/train_ref.py), each a one-line change of its source, must miss the bound the kernels are held to
(train_ref.bound64) by a factor of at least 100 on at least one case."""
import inspect

import numpy as np
import pytest

import train_cases as C
import train_ref as R

MISS = 100.0


def test_limits_are_the_headers(native):
    assert (C.MAX_T, C.MAX_STATES) == (native.TA_TRAIN_MAX_T, native.TA_CTC_MAX_STATES)
    assert C.LATTICE_SHAPES[-1][0] == 2 * C.LATTICE_SHAPES[-1][1] + 1 == C.MAX_STATES
    assert max(s[0] for s in C.LATTICE_SHAPES) == C.MAX_T


def test_yardstick_is_the_long_double_run():
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is no wider than float64 here: noise64 would be 0"
    a = np.asarray([1.0, -3.0])
    assert R.noise64(a, a.astype(np.longdouble) + np.longdouble(2) ** -60) == 2.0 ** -60
    assert R.bound64(a, 0.0) == 64 * 4 * np.spacing(3.0) and R.bound64(a, 1e-12) == 64e-12
    assert R.distance(a, a) == 0.0 and R.distance([1.0, np.nan], a) == np.inf and R.distance(a[:1], a) == np.inf


@pytest.mark.parametrize("name", [c[0] for c in C.lattice_cases()])
def test_lattice_case_keeps_its_conditions(name):
    """no logadd of the case within 1e-9 of the shortcut's threshold (the kernel and numpy differ near 1e-13 there and a
    tie is a 4.5e-5 jump); every case beyond T = 3 takes both sides of the shortcut; the labels and zeros as promised"""
    _, P, cs = C.lattice_case(name)
    w = C.lattice_want(name)
    T, no = P.shape
    assert w.stats["min_threshold_distance"] >= 1e-9, w.stats
    if T > 3:
        assert w.stats["max_logadd_gap"] > 10.0 > w.stats["min_logadd_gap"], w.stats
    assert np.abs(P.sum(axis=1) - 1).max() < 1e-14 and (P >= 0).all()
    if T * no >= 100 and no >= 5:                                   # (the straight line's class is never zeroed)
        assert 0.05 < (P == 0).mean() < 0.15
    if len(cs) > 1:
        assert cs[0] == cs[1]
    if cs:
        assert cs[-1] == no - 1 and min(cs) >= 1
    assert np.abs(w.ref["aligned"].sum(axis=1) - 1).max() <= w.bound["aligned"]
    assert all(np.isfinite(v) and v > 0 for v in w.bound.values())


def test_network_cases_are_what_they_say():
    rows = {name: sum(len(x) for x in lines) for name, _, lines, _ in C.net_cases()}
    assert rows["57 rows"] % C.OUT_ROWS == 1 and rows["55 rows"] % C.OUT_ROWS == 7
    assert [m[2].shape[0] for _, m, _, _ in C.net_cases()][2:6] == [2, 3, 127, 128]
    for name, model, lines, codes in C.net_cases():
        assert all(2 * len(cs) + 1 <= len(x) for x, cs in zip(lines, codes))
        assert any(2 * len(cs) + 1 == len(x) for x, cs in zip(lines, codes))
    assert [len(cs) for cs in C.net_case("57 rows")[3]] == [0, 0, 1, 4, 20]
    # line_answer is train_ref.gradients with the intermediate arrays kept
    _, model, lines, codes = C.net_case("55 rows")
    g = R.gradients(model[0], model[1], model[2], lines[2], codes[2])
    a = C.net_want("55 rows")[2].ref
    flat = {"fwd " + k: g["fwd"][k] for k in g["fwd"]}
    flat.update({"rev " + k: g["rev"][k] for k in g["rev"]})
    flat.update(W2=g["W2"], probs=g["probs"], aligned=g["aligned"], deltas=g["deltas"])
    assert all(np.array_equal(a[k], v) for k, v in flat.items()) and a["err"][0] == g["error"]
    # the saturated model passes every clamp, and the float32 checker cannot judge it
    _, model, lines, codes = C.net_case("saturated")
    out = R.net_forward(model[0], model[1], model[2], lines[3])
    gates = np.concatenate([out["f"][k] for k in ("gi", "gf", "go")])
    assert gates.max() == 1 / (1 + np.exp(-20.0)) and gates.min() == 1 / (1 + np.exp(20.0))
    assert np.abs(out["probs"][:, 0] - 0.5).max() < 1e-15 and out["probs"][:, 1].max() < 1e-80
    with np.errstate(all="ignore"):
        assert not np.isfinite(R.net_forward(model[0], model[1], model[2], lines[3], np.float32)["probs"]).all()


# ---- wrong variants of the checker ------------------------------------------------------------------------------------
def mutated(fn, old, new, **extra):
    """`fn` of train_ref with `old` (which must occur exactly once in its source) replaced by `new`"""
    src = inspect.getsource(fn)
    assert src.count(old) == 1, (fn.__name__, old)
    ns = dict(vars(R), **extra)
    exec(src.replace(old, new), ns)
    return ns[fn.__name__]


def _alternate(first, second):
    """a stand-in for _lattice: ctc_align_targets calls it for the forward recursion, then for the reversed one"""
    calls = []

    def lattice(lm, stats=None):
        calls.append(0)
        return (first if len(calls) % 2 else second)(lm, stats)
    return lattice


LATTICE_VARIANTS = {
    "states >= 256 not advanced": lambda: {"_lattice": mutated(
        R._lattice, "v = logadd(v, w) + lm[t]", "v = np.concatenate(((logadd(v, w) + lm[t])[:256], v[256:]))")},
    "no logadd shortcut": lambda: {"logadd": lambda x, y: np.logaddexp(x, y)},
    "floor without renormalisation": lambda: {"match_matrix": mutated(
        R.match_matrix, "Q = Q / Q.sum(axis=1, keepdims=True)", "pass")},
    "reversed entry penalty from t": lambda: {"_lattice": _alternate(R._lattice, mutated(
        R._lattice, "np.array([-5.0 * t]", "np.array([-5.0 * (T - 1 - t)]"))},
}
TAIL = [0]                             # rows of the line in hand that lie in the batch's last, partial group of 8 rows
NET_VARIANTS = {
    "softmax tail rows from zeros": lambda: {"net_forward": mutated(
        R.net_forward, "T = y.shape[0]\n", "T = y.shape[0]\n    y = y.copy()\n    y[T - TAIL[0]:] = 0\n", TAIL=TAIL)},
    "peepholes applied at s = 0": lambda: {"lstm_forward_states": mutated(
        R.lstm_forward_states, "        if t > 0:\n            c_new", "        if True:\n            c_new")},
    "gf c dropped at s = 1": lambda: {"lstm_forward_states": mutated(
        R.lstm_forward_states, "c_new = c_new + gf * c", "c_new = c_new + (gf * c if t != 1 else 0)")},
    "no sigmoid clamp": lambda: {"_sigmoid": mutated(R._sigmoid, "np.clip(-x, -20, 20)", "(-x)")},
    "no logit clip": lambda: {"net_forward": mutated(R.net_forward, "np.clip(z, -100, 100)", "z")},
    "carry with gf[t]": lambda: {"lstm_backward": mutated(R.lstm_backward, "ec_next * gf[t + 1]", "ec_next * gf[t]")},
}
NET_KEYS = ("probs", "aligned") + tuple(C.flat_names())


def _worst(monkeypatch, variant, lattice):
    """(largest distance / bound over the cases and arrays, where), stopping at the first case beyond MISS"""
    best = (0.0, None)
    with monkeypatch.context() as m:
        for k, v in variant().items():
            m.setattr(R, k, v)
        if lattice:
            for name, P, cs in C.lattice_cases():
                with np.errstate(all="ignore"):
                    q = C.lattice_want(name).miss(C.lattice_answer(P, cs))
                best = max([best] + [(v, (name, k)) for k, v in q.items()], key=lambda e: e[0])
                if best[0] >= MISS:
                    break
        else:
            for name, model, lines, codes in C.net_cases():
                for b, (xs, cs) in enumerate(zip(lines, codes)):
                    TAIL[0] = min(len(xs), sum(len(x) for x in lines) % C.OUT_ROWS) if b == len(lines) - 1 else 0
                    with np.errstate(all="ignore"):
                        q = C.net_want(name)[b].miss(C.line_answer(model, xs, cs), NET_KEYS)
                    best = max([best] + [(v, (name, b, k)) for k, v in q.items()], key=lambda e: e[0])
                if best[0] >= MISS:
                    break
    return best


def test_unchanged_checker_meets_its_own_bound(monkeypatch):
    assert _worst(monkeypatch, dict, True)[0] == 0.0 and _worst(monkeypatch, dict, False)[0] == 0.0


@pytest.mark.parametrize("name", list(LATTICE_VARIANTS))
def test_lattice_cases_catch_the_wrong_variant(monkeypatch, name):
    q, where = _worst(monkeypatch, LATTICE_VARIANTS[name], True)
    print("%s: %.3g x the bound at %s" % (name, q, where))
    assert q >= MISS, (name, q, where)


@pytest.mark.parametrize("name", list(NET_VARIANTS))
def test_network_cases_catch_the_wrong_variant(monkeypatch, name):
    q, where = _worst(monkeypatch, NET_VARIANTS[name], False)
    print("%s: %.3g x the bound at %s" % (name, q, where))
    assert q >= MISS, (name, q, where)


def test_both_sharpnesses_are_needed(monkeypatch):
    """the peaked S == T case alone misses the two variants that only move the low digits; its near-uniform twin catches
    them: why every shape is in the set at both sharpnesses"""
    for variant in ("no logadd shortcut", "floor without renormalisation"):
        q = {}
        with monkeypatch.context() as m:
            for k, v in LATTICE_VARIANTS[variant]().items():
                m.setattr(R, k, v)
            for sharp in C.SHARPNESS:
                name = "T513 L256 no20 sharp%g" % sharp
                _, P, cs = C.lattice_case(name)
                q[sharp] = max(C.lattice_want(name).miss(C.lattice_answer(P, cs)).values())
        print(variant, q)
        assert q[0.0] >= MISS, (variant, q)
