"""Forced alignment without a GPU: the emission score's error bound by enumeration, the checker
tests/forced_ref.py against a brute-force search over ALL valid paths, hand-worked cases, and the box rule under
refinement -- the checker's per-character rule on hand-made pages, and forced.py's array realisation against it."""
import itertools

import numpy as np
import pytest

import forced_ref as R
import harvest_ref as H


def test_emission_score_error_and_edges():
    g = np.arange(65536, dtype=np.int64)
    p = ((127 << 23) | (g << 7)).astype(np.uint32).view(np.float32)          # every g at e = 0: 1 <= p < 2 before the clamp
    frac = g + ((((g * (65536 - g)) >> 16) * 22713) >> 16)
    err = (frac - 65536.0 * np.log2(1.0 + g / 65536.0)) / 65536.0            # in bits
    assert np.abs(err).max() < 0.008 and err.min() < -0.0076 and err.max() > 0.0076
    assert (np.diff(frac) >= 0).all() and frac[0] == 0 and frac[-1] < 65536
    # the same through q_of, one octave down (p in [0.5, 1)): q = -65536 + frac, non-decreasing in p
    q = R.q_of((p * np.float32(0.5)).astype(np.float32))
    assert np.array_equal(q, frac - 65536)
    every = R.q_of(np.sort(np.random.default_rng(0).random(20000).astype(np.float32)))
    assert (np.diff(every) >= 0).all() and every.max() <= 0
    floor = -17 * 65536
    edge = np.asarray([1.0, 1.5, 2.0 ** -17, 2.0 ** -18, 0.0, -1.0, np.nan, np.inf, -np.inf, 1e-45, 0.5, 0.25], np.float32)
    assert R.q_of(edge).tolist() == [0, 0, floor, floor, floor, floor, floor, 0, floor, floor, -65536, -131072]
    assert R.q_of(np.float32(2.0 ** -17 * (1 + 2.0 ** -16))) == floor + 1   # just above the floor


def _all_paths(T, S, lab):
    """every state sequence the topology allows"""
    def ok(a, b):
        d = b - a
        return d in (0, 1) or (d == 2 and b % 2 == 1 and b >= 3 and lab[b] != lab[b - 2])
    paths = [[s] for s in (0, 1) if s < S]
    for _ in range(T - 1):
        paths = [p + [b] for p in paths for b in range(p[-1], min(p[-1] + 3, S)) if ok(p[-1], b)]
    return [p for p in paths if p[-1] in (S - 1, S - 2)]


def test_checker_against_brute_force_over_all_paths():
    rng = np.random.default_rng(2)
    seen = 0
    for no in (2, 3, 4):
        for L in (1, 2, 3):
            for cs in itertools.product(range(1, no), repeat=L):
                for T in list(range(2 * L + 1, 8)) * 2:
                    P = rng.random((T, no)).astype(np.float32)
                    if seen % 3 == 0:                                # coarse values: many equal totals
                        P = (2.0 ** -rng.integers(0, 3, size=(T, no))).astype(np.float32)
                    score, frames, path = R.align(P, cs)
                    lab = R.states(cs)
                    best = max(R.path_score(P, cs, p) for p in _all_paths(T, 2 * L + 1, lab))
                    assert score == best and R.path_score(P, cs, path.tolist()) == score, (cs, T)
                    for i in range(L):                               # every label state is visited, in order
                        ts = np.nonzero(path == 2 * i + 1)[0]
                        assert len(ts) and frames[i, 0] == ts[0] and frames[i, 1] == ts[-1] and ts[-1] - ts[0] + 1 == len(ts)
                        assert frames[i, 0] <= frames[i, 2] <= frames[i, 1]
                    seen += 1
    assert seen == 216


def test_hand_worked_line():
    """T = 6, text "ab" (classes 1, 2 of blank, a, b), probabilities 2^-k with k =

        t   blank  a  b
        0     1    2  3
        1     3    1  3
        2     2    2  2
        3     1    3  3
        4     3    3  1
        5     1    3  2

    so q = -65536 k.  States: blank a blank b blank.  In units of 65536, v after each step (. = unreachable):

        t = 0    -1   -2    .    .    .
        t = 1    -4   -2   -5   -5    .      (s = 3 by the skip from a: -2 - 3)
        t = 2    -6   -4   -4   -4   -7      (s = 2 from a: -2 - 2; s = 3 by the skip again: -2 - 2)
        t = 3    -7   -7   -5   -7   -5      (everything stays but the last blank, which advances: -4 - 1)
        t = 4   -10  -10   -8   -6   -8      (s = 3 advances from the blank: -5 - 1)
        t = 5   -11  -13   -9   -8   -7      (s = 4 advances from b: -6 - 1)

    The end is the last blank (-7 against -8); back: blank(5) <- b(4) <- blank(3) = blank(2) <- a(1) <- blank(0).
    a sits in t = 1 alone, b in t = 4 alone."""
    K = np.array([[1, 2, 3], [3, 1, 3], [2, 2, 2], [1, 3, 3], [3, 3, 1], [1, 3, 2]])
    score, frames, path = R.align((2.0 ** -K).astype(np.float32), [1, 2])
    assert score == -7 * 65536 and path.tolist() == [0, 1, 2, 2, 3, 4]
    assert frames.tolist() == [[1, 1, 1], [4, 4, 4]]


def test_all_equal_probabilities_the_tie_order_decides_every_move():
    """every path has the same total, T q(0.25): stay beats advance beats skip at every state, so every state is entered
    as late as the NEXT state allows only when it must be -- walked back from the last blank (S - 1 wins the tie at the
    end), the path stays there for as long as that state was reachable and takes the skips on the way down:
    "abc" in 9 steps is a(0) b(1) c(2) and then the last blank from t = 3 on (it was reached by advancing from c); "aa" in
    8 steps cannot skip the blank between the two: a(0) blank(1) a(2), the last blank from t = 3 on."""
    score, frames, path = R.align(np.full((9, 4), 0.25, np.float32), [1, 2, 3])
    assert score == 9 * -131072 and path.tolist() == [1, 3, 5, 6, 6, 6, 6, 6, 6]
    assert frames.tolist() == [[0, 0, 0], [1, 1, 1], [2, 2, 2]]
    score, frames, path = R.align(np.full((8, 4), 0.25, np.float32), [1, 1])
    assert score == 8 * -131072 and path.tolist() == [1, 2, 3, 4, 4, 4, 4, 4]
    assert frames.tolist() == [[0, 0, 0], [2, 2, 2]]
    with pytest.raises(ValueError):
        R.align(np.full((4, 4), 0.25, np.float32), [1, 1])            # 2 L + 1 > T
    with pytest.raises(ValueError):
        R.align(np.full((9, 4), 0.25, np.float32), [1, 4])            # a label that is no class


# ---- boxes under refinement ----------------------------------------------------------------------------------------------

def _ocr_boxes(o_line, x0=100, w=10):
    """a box per OCR character: 10 wide, one after the other, line l at y = 50 l .. 50 l + 40"""
    return [(x0 + w * j, 50 * l, x0 + w * j + w, 50 * l + 40) for j, l in enumerate(o_line)]


def test_box_rule_on_a_hand_made_page():
    """two lines; on the first the decoder lost "cd" of "ab cd ef" (op-1 columns) and read an extra "x" (op 2), the
    transcript has a space in front that was aligned with nothing.  Refined: every kept character has the line's own box
    for it, the syllable "cd" -- no box without refinement -- has one; the OCR "x" lends nothing; the second line keeps
    its OCR boxes."""
    tra, ocr = H.aligned_from_strings(" ab cd# ef gh", "#ab###x ef gh")
    o_line = [0, 0, 0, 0, 0, 0, 1, 1, 1]                               # a b x ' ' e f | ' ' g h
    ob = _ocr_boxes(o_line)
    plain = R.char_boxes(tra, ocr, o_line, ob, {})
    assert plain[0] is None and plain[1] == ob[0] and plain[4] is None and plain[5] is None and plain[10] == ob[7]
    assert R.syllable_box(plain, 4, 5) is None
    new = [(500 + 7 * k, 0, 507 + 7 * k, 40) for k in range(8)]        # "ab cd ef": t_first = 1, L = 8
    got = R.char_boxes(tra, ocr, o_line, ob, {0: (1, 8, new)})
    assert got[0] is None and got[1:9] == new and got[9:] == plain[9:]
    assert R.syllable_box(got, 4, 5) == (521, 0, 535, 40)
    # a trimmed end space whose partner lies on the refined line loses its box
    tra, ocr = H.aligned_from_strings("ab cd ", "ab cd ")
    ob = _ocr_boxes([0] * 6)
    got = R.char_boxes(tra, ocr, [0] * 6, ob, {0: (0, 5, new[:5])})
    assert got == new[:5] + [None]
    # a syllable over two lines takes the lower one (largest uly), as today
    assert R.syllable_box([(1, 0, 2, 40), (3, 50, 9, 90), (4, 50, 12, 90)], 0, 2) == (3, 50, 12, 90)


def test_box_rule_on_the_harvest_worked_example_with_its_last_line_acceptable():
    """DESIGN.md section 14.6's page with the seam behind its last line closed (the final " " over a gap dropped and the
    "bum" in front of it paired) so that line 3 is accepted; lines 0 and 1 stay rejected and keep their OCR boxes"""
    from test_harvest import WORKED, _classes
    seg = WORKED[:4] + [("bum", "bum", 1), WORKED[5]]
    tra, ocr = "".join(s[0] for s in seg), "".join(s[1] for s in seg)
    o_line = [s[2] for s in seg for ch in s[1] if ch != "#"]
    transcript = tra.replace("#", "")
    tr_al, oc_al = H.aligned_from_strings(tra, ocr)
    rows = H.harvest_page(tr_al, oc_al, o_line, 0, 4, _classes(transcript), {0: 40, 1: 40, 2: 40, 3: 19}, 4, 5)
    assert [rows[l][0] for l in range(4)] == [H.SEAM | H.UNANCHORED, 0, H.EMPTY | H.LOW, 0]
    assert rows[3][1:3] == [27, 9] and transcript[27:36] == "et verbum"
    ob = _ocr_boxes(o_line)
    t_peak = [3, 5, 6, 8, 9, 11, 13, 15, 17]
    new = R.peak_boxes(t_peak, 19, 90, 40, 150, 190, 1)                # T = 19, pad 1: x = (t - 1) 90 / 17
    assert new[0] == (40, 150, 51, 190) and new[1] == (51, 150, 61, 190) and new[-1][2] == 40 + 85
    got = R.char_boxes(tr_al, oc_al, o_line, ob, {3: (27, 9, new)})
    plain = R.char_boxes(tr_al, oc_al, o_line, ob, {})
    assert got[:27] == plain[:27] and got[27:36] == new
    assert plain[32] == ob[o_line.index(3) + 6]                        # the "b" the decoder read as "8" had the 8's box


def _random_page(rng):
    import harvest_cases as HC
    from oracle import nw_oracle
    t = HC._words(rng, int(rng.integers(0, 90)))
    o = HC._noisy(rng, t, 0.08, 0.08, 0.05)
    nl = int(rng.integers(1, 6))
    pg = HC._page(rng, t, o, nl, empty=tuple(l for l in range(1, nl) if rng.random() < 0.15), T=[400] * nl)
    ops = nw_oracle.align_ids(pg["t"], pg["o"], HC.DEFAULT)
    return pg, np.asarray(ops, dtype=np.uint8)


def test_array_realisation_equals_the_per_character_rule_on_random_columns():
    """forced.refine_columns + the box array against R.char_boxes on random pages (tests/harvest_cases.py style): the
    harvest checker says which lines are accepted, each of them is 'refined' with made-up boxes"""
    from text_alignment_amd import forced
    rng = np.random.default_rng(77)
    refined_lines = pages_with = 0
    for _ in range(120):
        pg, ops = _random_page(rng)
        tra, ocr = H.aligned_from_ops(ops.tolist(), pg["t"].tolist(), pg["o"].tolist())
        o_line = pg["o_line"].tolist()
        rows = H.harvest_page(tra, ocr, o_line, 0, pg["lines"], pg["t_class"].tolist(), pg["T"].tolist(), 3, 5)
        m = len(o_line)
        old = np.asarray(_ocr_boxes(o_line), dtype=np.int64).reshape(-1, 4)
        idx = rng.permutation(m + 5)[:m].astype(np.int64)              # the page's characters lie anywhere in the box array
        boxes = np.full((m + 5, 4), -1, dtype=np.int64)
        boxes[idx] = old
        lines, refined, extra = [], {}, []
        for l in range(pg["lines"]):
            if rows[l][0] == 0 and rng.random() < 0.8:
                L = rows[l][2]
                new = [(1000 * l + 3 * k, 50 * l + 1, 1000 * l + 3 * k + 3, 50 * l + 41) for k in range(L)]
                lines.append((l, rows[l][1], L, len(boxes) + len(extra)))
                refined[l] = (rows[l][1], L, new)
                extra += new
        all_boxes = np.concatenate([boxes, np.asarray(extra, dtype=np.int64).reshape(-1, 4)])
        ops2, idx2 = forced.refine_columns(ops, idx, pg["o_line"], lines)
        assert int((ops2 != 2).sum()) == len(pg["t"]) and int((ops2 != 1).sum()) == len(idx2)
        got, j = [], 0
        for op in ops2:
            if op == 0:
                got.append(tuple(int(v) for v in all_boxes[idx2[j]]))
            elif op == 1:
                got.append(None)
            j += op != 1
        assert got == R.char_boxes(tra, ocr, o_line, old, refined)
        if not lines:
            assert np.array_equal(ops2, ops) and np.array_equal(idx2, idx)
        refined_lines += len(lines)
        pages_with += bool(lines)
    assert refined_lines > 60 and pages_with > 40


def test_peak_boxes_equal_the_checkers():
    from text_alignment_amd import forced
    rng = np.random.default_rng(3)
    L = [5, 1, 12]
    T, raw_w, x_min, y_min = [60, 35, 200], [113, 20, 777], [40, 7, 0], [100, 220, 340]
    peaks = [np.sort(rng.choice(np.arange(16, t - 16), size=l, replace=False)) for l, t in zip(L, T)]
    got = forced.peak_boxes(np.concatenate(peaks), L, T, raw_w, x_min, y_min, [y + 60 for y in y_min], 16)
    want = [b for k in range(3) for b in R.peak_boxes(peaks[k], T[k], raw_w[k], x_min[k], y_min[k], y_min[k] + 60, 16)]
    assert [tuple(r) for r in got.tolist()] == want


def test_library_refuses_bad_arguments_before_any_launch(native):
    """TA_EINVAL / TA_ELIMIT from the real library without a device: the checks come before the launch"""
    lib = native.lib
    assert lib.ta_forced_workspace_bytes(3, 1) == 256 and lib.ta_forced_workspace_bytes(2, 1) == -1
    T, L = np.asarray([9], np.int32), np.asarray([3], np.int32)
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data

    def call(no=4, rows=9, nlabels=3, T=T, L=L, ws=p, ws_bytes=4096, frames=p, nlines=1):
        return lib.ta_forced_align(p, p, p, p, p, p, p, nlines, no, rows, nlabels, T.ctypes.data, L.ctypes.data, ws, ws_bytes,
                                   frames, p, p, None)
    assert call(no=1) == native.TA_EINVAL and call(no=129) == native.TA_EINVAL and call(nlines=-1) == native.TA_EINVAL
    assert call(rows=8) == native.TA_EINVAL and call(nlabels=2) == native.TA_EINVAL and call(ws_bytes=255) == native.TA_EINVAL
    assert call(frames=None) == native.TA_EINVAL and call(ws=p + 4) == native.TA_EINVAL
    assert call(L=np.asarray([5], np.int32)) == native.TA_EINVAL and call(L=np.asarray([0], np.int32)) == native.TA_EINVAL
    assert call(T=np.asarray([5001], np.int32)) == native.TA_ELIMIT
    assert call(T=np.asarray([4000], np.int32), L=np.asarray([1024], np.int32)) == native.TA_ELIMIT
    assert call(nlines=0) == native.TA_OK
    assert not buf.any()
