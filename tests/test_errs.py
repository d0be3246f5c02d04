"""Held-out scoring of line models without a GPU: the plain-Python checker tests/errs_ref.py
against known answers, an independent two-row Levenshtein and its own invariants; the host side of
text_alignment_amd/errs.py; and everything the C ABI and the Python layers refuse before the device is touched."""
import ctypes
import math

import numpy as np
import pytest

import errs_ref as R

CODEC = ["", " ", "~"] + list("abcdefghijklmnopqrstuvwxyz")


def _codes(s):
    return [CODEC.index(ch) for ch in s]


def _levenshtein_two_rows(a, g):
    prev = list(range(len(g) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(g)
        for j in range(1, len(g) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != g[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(g)]


def test_known_answers():
    nc = len(CODEC) + 1
    t, conf = R.score_line(_codes("kitten"), _codes("sitting"), nc)
    assert t == (3, 6, 7, 2, 0, 1)
    assert conf[CODEC.index("k"), CODEC.index("s")] == 1 and conf[CODEC.index("e"), CODEC.index("i")] == 1
    assert conf[0, CODEC.index("g")] == 1 and conf[CODEC.index("t"), CODEC.index("t")] == 2
    t, conf = R.score_line([], [], nc)
    assert t == (0, 0, 0, 0, 0, 0) and conf.sum() == 0
    t, conf = R.score_line([], _codes("abc"), nc)
    assert t == (3, 0, 3, 0, 0, 3) and conf[0].sum() == 3
    t, conf = R.score_line(_codes("abc"), [], nc)
    assert t == (3, 3, 0, 0, 3, 0) and conf[:, 0].sum() == 3
    # the tie order decides: "xab" against "ab" costs 1 whichever of x, a is the insertion; the walk takes the
    # diagonals from the end and is left with the leading one
    t, conf = R.score_line(_codes("xab"), _codes("ab"), nc)
    assert t == (1, 3, 2, 0, 1, 0) and conf[CODEC.index("x"), 0] == 1
    # "aab" against "ab": the diagonal is preferred at (2, 1) although a[1] = a would match as well one row up
    t, conf = R.score_line(_codes("aab"), _codes("ab"), nc)
    assert t == (1, 3, 2, 0, 1, 0) and conf[CODEC.index("a"), 0] == 1 and conf[CODEC.index("a"), CODEC.index("a")] == 1


def test_checker_against_two_row_levenshtein_and_its_invariants():
    rng = np.random.default_rng(5)
    nc = 12
    for trial in range(200):
        n, m = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        alpha = 3 if trial % 2 else 8                   # small alphabets: many ties
        a = rng.integers(2, 2 + alpha, size=n).tolist()
        g = rng.integers(2, 2 + alpha, size=m).tolist() if trial % 5 else list(a[:m])
        (errors, nn, mm, subs, ins, dels), conf = R.score_line(a, g, nc, "exact")
        assert (nn, mm) == (len(a), len(g))
        n, m = len(a), len(g)
        assert errors == _levenshtein_two_rows(a, g)
        matches = int(np.trace(conf))
        assert subs + ins + dels == errors
        assert matches + subs + ins == n and matches + subs + dels == m
        assert conf[0, 0] == 0 and conf[1:, 0].sum() == ins and conf[0, 1:].sum() == dels
        assert conf.sum() - matches - ins - dels == subs
        for c in range(1, nc):                          # row sums: the decoded codes; column sums: the truth's
            assert conf[c].sum() == a.count(c) and conf[:, c].sum() == g.count(c)


def test_text_kinds():
    from text_alignment_amd import errs
    for mod in (R, errs):
        assert mod.normalise_text("  a  b\t c \n", "exact") == "a b c"
        assert mod.normalise_text("  a  b\t c \n", "nospace") == "abc"
        assert mod.normalise_text("é", "exact") == "é"             # NFC first
        assert mod.encode_target(CODEC, " a  b ", "exact") == _codes("a b")
        assert mod.encode_target(CODEC, " a  b ", "nospace") == _codes("ab")
        with pytest.raises(ValueError):
            mod.normalise_text("a", "loose")
    sp = 1
    dec = [0, sp, sp, 3, 0, sp, 0, sp, 4, sp, 0]        # class 0 scattered; leading, doubled, trailing spaces
    assert R.filter_decoded(dec, "exact") == [3, sp, 4]
    assert R.filter_decoded(dec, "nospace") == [3, 4]
    assert R.filter_decoded([sp, 0, sp], "exact") == [] and R.filter_decoded([sp, 0, sp], "nospace") == []
    assert R.score_line(dec, _codes("a b"), 30, "exact")[0] == (0, 3, 3, 0, 0, 0)
    assert R.score_line(dec, _codes("ab"), 30, "nospace")[0] == (0, 2, 2, 0, 0, 0)
    assert R.score_line(dec, _codes("ab"), 30, "exact")[0] == (1, 3, 2, 0, 1, 0)


def test_unknown_character_is_an_error_under_question_mark():
    from text_alignment_amd import errs
    no = len(CODEC)
    for mod in (R, errs):
        assert mod.encode_target(CODEC, "aßb", "exact") == [CODEC.index("a"), no, CODEC.index("b")]
    t, conf = R.score_line(_codes("asb"), R.encode_target(CODEC, "aßb"), no + 1)
    assert t == (1, 3, 3, 1, 0, 0)
    assert R.confusions(conf, CODEC) == [(1, "s", "?")]
    t, conf = R.score_line(_codes("ab"), R.encode_target(CODEC, "aßb"), no + 1)
    assert t == (1, 2, 3, 0, 0, 1) and R.confusions(conf, CODEC) == [(1, "_", "?")]
    per = np.array([[1, 3, 3, 1, 0, 0], [0, 0, 0, 0, 0, 0]], dtype=np.int32)
    assert R.totals(per) == {"errors": 1, "chars": 3, "lines": 2, "cer": 1 / 3}
    assert math.isnan(R.totals(per[1:])["cer"])
    res = errs.ErrsResult(per, None)
    assert (res.errors, res.chars, res.lines, res.cer) == (1, 3, 2, 1 / 3)
    assert math.isnan(errs.ErrsResult(per[1:], None).cer) and math.isnan(errs.ErrsResult(per[:0], None).cer)


def test_python_refuses_before_the_device():
    from text_alignment_amd import errs, ocr, train
    model = ocr.LineModel.random(3, no=len(CODEC))
    line = np.zeros((40, 48))
    with pytest.raises(ValueError, match="2 lines but 1 texts"):
        errs.evaluate(model, [line, line], ["a"])
    with pytest.raises(ValueError, match="kind"):
        errs.evaluate(model, [line], ["a"], kind="loose")
    with pytest.raises(ValueError, match="exceeds"):
        errs.evaluate(model, [line], ["ab" * 2049])
    with pytest.raises(ValueError):
        errs.evaluate_models([model, model], [line], ["a", "b"])
    with pytest.raises(ValueError, match="exceeds"):
        errs.evaluate_models([model], [line], ["a" * 4097])
    assert len(errs.encode_target(model.codec, "a " * 4096, "exact")) == 8191      # the limit is on the NORMALISED text
    assert len(errs.encode_target(model.codec, " a" * 4096, "nospace")) == 4096
    tr = train.LineTrainer(model=model)
    with pytest.raises(ValueError):
        tr.evaluate([line], ["a", "b"])
    with pytest.raises(ValueError, match="kind"):
        tr.evaluate([line], ["a"], kind="fuzzy")
    assert tr.W is None                                                            # nothing reached the device
    # the low-level call: the host arguments are checked before the tensors are looked at
    with pytest.raises(ValueError, match="targets"):
        errs.score_decoded(None, None, None, [40, 40], [[2]], 29)
    with pytest.raises(ValueError, match="kind"):
        errs.score_decoded(None, None, None, [40], [[2]], 29, kind="x")
    with pytest.raises(ValueError, match="exceeds"):
        errs.score_decoded(None, None, None, [40], [[2] * 4097], 29)
    with pytest.raises(ValueError, match="codes"):
        errs.score_decoded(None, None, None, [40], [[30]], 29)
    with pytest.raises(ValueError, match="codes"):
        errs.score_decoded(None, None, None, [40], [[0]], 29)
    with pytest.raises(ValueError, match="timesteps"):
        errs.score_decoded(None, None, None, [5001], [[2]], 29)
    with pytest.raises(ValueError, match="device tensor"):
        errs.score_decoded(None, None, None, [40], [[2]], 29)


def test_abi_refuses_before_the_device(native):
    lib = native.lib
    ws = lib.ta_errs_workspace_bytes
    assert ws(-1, 5) == native.TA_EINVAL and ws(5, -1) == native.TA_EINVAL
    assert ws(2501, 5) == native.TA_ELIMIT and ws(5, 4097) == native.TA_ELIMIT
    assert ws(2500, 4096) > 0 and ws(0, 0) == 0 and ws(10, 0) == 0
    one = (ctypes.c_int32 * 1)(100)
    p = ctypes.addressof(one)                   # any non-null address: nothing is dereferenced on the device before the checks

    def call(n=1, nclasses=97, kind=0, dec_c=p, conf=p, nb=one, m=one, ws_bytes=1 << 30, dec_len=1000, tgt_len=1000):
        return lib.ta_edit_distance(dec_c, p, p, dec_len, p, p, p, tgt_len, p, p, n, nclasses, kind,
                                    ctypes.addressof(nb) if nb is not None else None,
                                    ctypes.addressof(m) if m is not None else None, p, ws_bytes, p, conf, None)
    assert call(dec_c=None) == native.TA_EINVAL and b"null" in lib.ta_last_error()
    assert call(conf=None) == native.TA_EINVAL and b"null" in lib.ta_last_error()
    assert call(nb=None) == native.TA_EINVAL and call(m=None) == native.TA_EINVAL
    assert call(n=-1) == native.TA_EINVAL and call(dec_len=-1) == native.TA_EINVAL and call(tgt_len=-1) == native.TA_EINVAL
    assert call(kind=2) == native.TA_EINVAL and call(kind=-1) == native.TA_EINVAL and b"kind" in lib.ta_last_error()
    assert call(nclasses=1) == native.TA_EINVAL and call(nclasses=130) == native.TA_EINVAL
    assert call(nb=(ctypes.c_int32 * 1)(-1)) == native.TA_EINVAL and call(m=(ctypes.c_int32 * 1)(-3)) == native.TA_EINVAL
    assert call(nb=(ctypes.c_int32 * 1)(2501)) == native.TA_ELIMIT
    assert call(m=(ctypes.c_int32 * 1)(4097)) == native.TA_ELIMIT and b"TA_ERRS_MAX" in lib.ta_last_error()
    assert call(ws_bytes=ws(100, 100) - 1) == native.TA_EINVAL and b"workspace" in lib.ta_last_error()
    assert call(n=0) == native.TA_OK
    with pytest.raises(ValueError):
        native.check(call(kind=7), "ta_edit_distance")


def test_workspace_bytes_monotone_and_bounded(native):
    ws = native.lib.ta_errs_workspace_bytes
    ns = [0, 1, 5, 63, 64, 65, 200, 1000, 2499, 2500]
    ms = [0, 1, 63, 64, 65, 128, 129, 600, 4095, 4096]
    for m in ms:
        col = [ws(n, m) for n in ns]
        assert col == sorted(col) and (m == 0 or len(set(col)) == len(col))        # strictly with n once there are columns
    for n in ns:
        row = [ws(n, m) for m in ms]
        assert row == sorted(row)
        for m, b in zip(ms, row):
            assert b % 16 == 0
            assert 4 * b >= n * m                                  # two pointer bits for every cell
            assert b <= n * m + 16 * (n + m) + 1024                # at most a byte per cell plus O(n + m)
