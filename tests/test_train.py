"""CPU tests of line-model training: they pin the CHECKER (tests/train_ref.py, the float64 numpy restatement of
DESIGN.md section 14 that the training kernels are compared with on the GPU, tests/test_train_gpu.py), the model
writer, and the argument checking of the new entry points (no GPU needed)."""
import itertools

import numpy as np
import pytest

import train_ref as R


# ---- 1. gradients against central differences ---------------------------------------------------------------------
def _small_net(seed=11, ni=6, ns=5, no=7, T=9):
    rng = np.random.default_rng(seed)
    na = 1 + ni + ns

    def lstm():
        d = {k: rng.uniform(-0.8, 0.8, size=(ns, na)) for k in R.GATES}
        d.update({k: rng.uniform(-0.8, 0.8, size=(ns,)) for k in R.PEEPS})
        return d
    fwd, rev = lstm(), lstm()
    W2 = rng.uniform(-0.8, 0.8, size=(no, 1 + 2 * ns))
    xs = rng.uniform(0, 1, size=(T, ni))
    return fwd, rev, W2, xs, [3, 3, 5]                 # a repeated character: 7 states in 9 timesteps


def test_gradients_match_central_differences():
    """Every weight family (the four gate matrices with their bias column, the three peepholes, both directions, W2):
    the analytic derivative of -CE, `aligned` held fixed, against central differences of -CE.  Bound: 1e-5 relative on
    every component above 1e-3 in magnitude."""
    fwd, rev, W2, xs, cs = _small_net()
    g = R.gradients(fwd, rev, W2, xs, cs)
    aligned = g["aligned"]
    h = 1e-6
    families = [("fwd", k, fwd[k], g["fwd"][k]) for k in R.GATES + R.PEEPS]
    families += [("rev", k, rev[k], g["rev"][k]) for k in R.GATES + R.PEEPS]
    families.append(("out", "W2", W2, g["W2"]))
    checked = {}
    for where, name, arr, ana in families:
        assert ana.shape == arr.shape
        num = np.zeros_like(arr)
        flat, nflat = arr.reshape(-1), num.reshape(-1)
        for i in range(flat.size):
            keep = flat[i]
            flat[i] = keep + h
            up = R.cross_entropy(fwd, rev, W2, xs, aligned)
            flat[i] = keep - h
            dn = R.cross_entropy(fwd, rev, W2, xs, aligned)
            flat[i] = keep
            nflat[i] = -(up - dn) / (2 * h)
        big = np.abs(num) > 1e-3
        rel = np.abs(ana - num)[big] / np.abs(num)[big]
        checked[(where, name)] = (int(big.sum()), float(rel.max()) if big.any() else 0.0)
        assert big.any(), (where, name)
        assert rel.max() < 1e-5, (where, name, rel.max())
        if arr.ndim == 2 and name != "W2":
            assert big[:, 0].any(), "no bias component of %s %s above 1e-3" % (where, name)
    print(checked)


# ---- 2. invariants of the alignment ---------------------------------------------------------------------------------
def test_ctc_rows_sum_to_one_and_foreign_classes_sit_at_the_floor():
    rng = np.random.default_rng(5)
    for T, no, cs in [(40, 9, [3, 4, 4, 7]), (12, 5, [2]), (25, 12, [5, 5, 5, 6, 1]), (7, 4, [])]:
        P = rng.random((T, no)) ** 3
        P /= P.sum(axis=1, keepdims=True)
        al = R.ctc_align_targets(P, cs)
        assert al.shape == (T, no)
        assert np.abs(al.sum(axis=1) - 1).max() < 1e-12
        foreign = [c for c in range(no) if c != 0 and c not in cs]
        assert foreign
        # the clamp floor as the row normalisation left it: one value per row, the row's smallest
        assert np.all(al[:, foreign] == al[:, foreign[:1]]) and np.all(al[:, foreign[0]] == al.min(axis=1))
        assert np.all(al[:, foreign] > 0)
    with pytest.raises(ValueError):
        R.ctc_align_targets(np.full((4, 3), 1 / 3.0), [1, 2])             # 5 states, 4 timesteps


# ---- 3. the lattice against an enumeration of paths -------------------------------------------------------------------
def _paths_logsum(lm):
    """A[t, s] = log of the summed weight of every monotone path (stay / advance by one) that ends in state s at time
    t, with the lattice's entry penalties: a path starts before t = 0 in any state p (weight -5 p) or enters state 0 at
    any time t0 (weight -5 t0)."""
    T, S = lm.shape
    tot = np.zeros((T, S))
    for t in range(T):
        # started before time 0 in state p: t + 1 moves
        for p in range(S):
            for moves in itertools.product((0, 1), repeat=t + 1):
                s, w, ok = p, -5.0 * p, True
                for u, m in enumerate(moves):
                    s += m
                    if s >= S:
                        ok = False
                        break
                    w += lm[u, s]
                if ok:
                    tot[t, s] += np.exp(w)
        # entered state 0 at time t0: t - t0 moves after it
        for t0 in range(t + 1):
            for moves in itertools.product((0, 1), repeat=t - t0):
                s, w, ok = 0, -5.0 * t0 + lm[t0, 0], True
                for u, m in enumerate(moves):
                    s += m
                    if s >= S:
                        ok = False
                        break
                    w += lm[t0 + 1 + u, s]
                if ok:
                    tot[t, s] += np.exp(w)
    return np.log(tot)


def test_ctc_lattice_equals_brute_force_enumeration():
    """T <= 6, L <= 2: the aligned targets built from an explicit enumeration of all paths equal the lattice's to
    1e-12.  An enumeration sums paths exactly, while the spec's logadd drops the smaller term when two differ by more
    than 10, so the comparison is made where that shortcut never fires: the targets' classes are all unlikely and
    about equally so (a foreign class takes most of every row), which keeps neighbouring states within 10 of each
    other.  The test asserts that this held (max_logadd_gap), so it cannot pass by accident of the shortcut."""
    rng = np.random.default_rng(17)
    cases = [(T, cs) for T in range(1, 7) for cs in ([], [1], [2], [1, 2], [2, 1], [1, 1]) if 2 * len(cs) + 1 <= T]
    assert any(T == 6 and len(cs) == 2 for T, cs in cases)
    for T, cs in cases:
        no = 4
        P = np.empty((T, no))
        P[:, :3] = 0.03 * rng.uniform(0.7, 1.3, size=(T, 3))
        P[:, 3] = 1 - P[:, :3].sum(axis=1)
        stats = {}
        got = R.ctc_align_targets(P, cs, stats=stats)
        assert stats["max_logadd_gap"] <= 10.0, (T, cs, stats)
        lm = R.match_matrix(P, cs)
        A = _paths_logsum(lm)
        B = _paths_logsum(lm[::-1, ::-1])[::-1, ::-1]
        want = R.normalise_paths(A + B, R.ctc_labels(cs), no)
        assert np.abs(got - want).max() < 1e-12, (T, cs, np.abs(got - want).max())


def test_logadd_shortcut_and_float32_variant():
    x, y = np.array([0.0, -3.0, 5.0]), np.array([-11.0, -2.0, 16.0])
    got = R.logadd(x, y)
    assert got[0] == 0.0 and got[2] == 16.0 and abs(got[1] - np.log(np.exp(-3.0) + np.exp(-2.0))) < 1e-15
    fwd, rev, W2, xs, cs = _small_net()
    g32 = R.gradients(fwd, rev, W2, xs, cs, dtype=np.float32)
    g64 = R.gradients(fwd, rev, W2, xs, cs)
    assert g32["W2"].dtype == np.float32 and g32["fwd"]["WGI"].dtype == np.float32 and g32["aligned"].dtype == np.float32
    gap = np.abs(g32["W2"] - g64["W2"]).max()
    assert 0 < gap < 1e-3                      # single precision: different, and only in the low digits


def test_checker_update_is_momentum_sgd():
    fwd, rev, W2, xs, cs = _small_net()
    tr = R.Trainer(fwd, rev, W2, lrate=1e-2, momentum=0.5)
    g1 = R.gradients(fwd, rev, W2, xs, cs)
    tr.update([xs], [cs])
    assert np.allclose(tr.W2, W2 + 1e-2 * g1["W2"], rtol=0, atol=1e-15)
    g2 = R.gradients(tr.fwd, tr.rev, tr.W2, xs, cs)
    before = tr.fwd["WIP"].copy()
    tr.update([xs], [cs])
    assert np.allclose(tr.fwd["WIP"], before + 0.5 * 1e-2 * g1["fwd"]["WIP"] + 1e-2 * g2["fwd"]["WIP"], rtol=0, atol=1e-15)
    assert np.array_equal(fwd["WIP"], _small_net()[0]["WIP"])         # the caller's arrays are not touched


# ---- 4. the model writer ----------------------------------------------------------------------------------------------
def test_save_pyrnn_round_trip(tmp_path):
    import sys
    from text_alignment_amd import model_io, train
    m = train.fresh_model(u"abc ā~", seed=4)
    assert m.codec == ["", " ", "~", "a", "b", "c", u"ā"]
    assert all(np.abs(m.fwd[k]).max() < 0.1 for k in R.GATES + R.PEEPS) and np.abs(m.W2).max() < 0.1
    f, r, W2 = R.fresh_weights(4, len(m.codec))
    assert np.array_equal(m.fwd["WGO"], f["WGO"]) and np.array_equal(m.rev["WOP"], r["WOP"]) and np.array_equal(m.W2, W2)
    path = str(tmp_path / "m.pyrnn.gz")
    model_io.save_pyrnn(m, path)
    assert "ocrolib" not in sys.modules and "ocrolib.lstm" not in sys.modules
    assert open(path, "rb").read(2) == b"\x1f\x8b"
    back = model_io.load_pyrnn(path)
    assert back.codec == m.codec and back.no == m.no
    for k in R.GATES + R.PEEPS:
        assert np.array_equal(back.fwd[k], m.fwd[k]) and np.array_equal(back.rev[k], m.rev[k])
    assert np.array_equal(back.W2, m.W2) and back.W2.dtype == np.float64


# ---- 5. error paths ---------------------------------------------------------------------------------------------------
def test_line_trainer_argument_errors():
    from text_alignment_amd import train
    line = np.zeros((40, 48), dtype=np.float32)
    with pytest.raises(ValueError):
        train.LineTrainer()                                         # neither a model nor a charset
    with pytest.raises(ValueError):
        train.LineTrainer(model=train.fresh_model("ab"), charset="ab")
    with pytest.raises(ValueError):
        train.LineTrainer(charset="ab", lines_per_update=0)
    with pytest.raises(ValueError):
        train.LineTrainer(charset="ab", lrate=0.0)
    tr = train.LineTrainer(charset="ab c")
    assert tr.codec == ["", " ", "~", "a", "b", "c"]
    for fn in (tr.train, tr.gradients, tr.align):
        with pytest.raises(ValueError, match="codec"):
            fn([line], ["abx"])                                     # a character outside the codec
        with pytest.raises(ValueError, match="does not fit"):
            fn([line], ["ab" * 10])                                 # 41 states, 40 timesteps
        with pytest.raises(ValueError, match="longer"):
            fn([np.zeros((5001, 48), dtype=np.float32)], ["ab"])
        with pytest.raises(ValueError):
            fn([line, line], ["ab"])
    assert train.encode_text(tr.codec, "a b~") == [3, 1, 4, 2]
    m = tr.model()                                                   # no device needed to get the weights back
    assert m.no == 6 and m.fwd["WGI"].shape == (100, 149)


def test_new_entry_points_refuse_bad_sizes_without_gpu(native):
    import ctypes
    lib = native.lib
    assert lib.ta_ctc_workspace_bytes(72, 5, 8) == 72 * (11 + 8) * 8
    assert lib.ta_ctc_workspace_bytes(10, 5, 8) == -1               # 11 states, 10 timesteps
    assert lib.ta_ctc_workspace_bytes(5001, 5, 8) == -1 and lib.ta_ctc_workspace_bytes(5000, 1025, 8) == -1
    assert lib.ta_ctc_workspace_bytes(72, 5, 129) == -1 and lib.ta_ctc_workspace_bytes(72, 5, 1) == -1

    def ctc(T, L, no=8, ws=1 << 30, ptr=None):
        Th, Lh = (ctypes.c_int32 * 1)(T), (ctypes.c_int32 * 1)(L)
        return lib.ta_ctc_align(ptr, ptr, ptr, ptr, ptr, ptr, ptr, 1, no, T, L, Th, Lh, ptr, ws, ptr, ptr, ptr, None)
    assert ctc(10, 5) == native.TA_EINVAL and b"do not fit" in lib.ta_last_error()
    with pytest.raises(ValueError):
        native.check(ctc(10, 5), "ta_ctc_align")
    assert ctc(5001, 5) == native.TA_EINVAL
    assert ctc(0, 0) == native.TA_EINVAL
    assert ctc(72, 5, no=200) == native.TA_EINVAL
    assert ctc(72, 5, ws=8) == native.TA_EINVAL and b"workspace" in lib.ta_last_error()
    assert ctc(72, 5) == native.TA_EINVAL and b"null" in lib.ta_last_error()
    assert lib.ta_ctc_align(None, None, None, None, None, None, None, 1, 8, 72, 5, None, None, None, 0, None, None,
                            None, None) == native.TA_EINVAL
    fw = lambda n, max_T, rows, no: lib.ta_lstm_train_forward(None, None, None, n, max_T, rows, None, None, None, no,
                                                              None, None, None, None)
    bw = lambda n, max_T, rows: lib.ta_lstm_train_backward(None, None, None, None, n, max_T, rows, None, None, None,
                                                           None, None)
    assert fw(1, 72, 72, 8) == native.TA_EINVAL and b"null" in lib.ta_last_error()
    assert bw(1, 72, 72) == native.TA_EINVAL and b"null" in lib.ta_last_error()
    assert fw(1, 5001, 5001, 8) == native.TA_EINVAL and b"TA_TRAIN_MAX_T" in lib.ta_last_error()
    assert bw(1, 5001, 5001) == native.TA_EINVAL
    assert fw(-1, 72, 72, 8) == native.TA_EINVAL and bw(1, 72, -1) == native.TA_EINVAL
    assert fw(1, 72, 72, 129) == native.TA_EINVAL
    assert fw(0, 0, 0, 8) == native.TA_OK and bw(0, 0, 0) == native.TA_OK
