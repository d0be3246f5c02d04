"""tests/forced_page_omit_ref.py, the specification of record of page-scope forced alignment with omission (DESIGN.md
section 14.12), held against what it must satisfy: a page of one line is forced_omit_ref.align, an omission dearer than
any path gives forced_page_ref.align_page wherever that finds a path, small lattices against the enumeration of every
legal path, the closed form against the written one -- and forced.page_columns with omitted rows against a hand-made
answer.  No GPU."""
import numpy as np
import pytest

import forced_cases as FC
import forced_omit_ref as OR
import forced_page_cases as PC
import forced_page_omit_ref as R
import forced_page_ref as PR
import forced_ref as FR

UNIT = 1 << 16
OMITS = (0, UNIT, 5 * UNIT, 1 << 26)


def _windows(rng, nl, n):
    """random windows that keep section 14.8's conditions"""
    lo, hi = [0], [int(rng.integers(0, n + 1))]
    for k in range(1, nl):
        lo.append(int(rng.integers(lo[-1], hi[-1] + 1)))
        hi.append(int(rng.integers(hi[-1], n + 1)))
    hi[-1] = n
    assert PR.windows_ok(lo, hi, n)
    return lo, hi


def test_a_page_of_one_line_is_the_line_alignment_with_omission():
    rng = np.random.default_rng(1412)
    seen = 0
    for trial in range(60):
        L = int(rng.integers(1, 4))
        T = int(rng.integers(2 * L + 1, 10))
        no = int(rng.integers(3, 6))
        P, cs = FC.probs(rng, T, no, sharp=2.0), FC.text(rng, L, no)
        if trial % 5 == 4:
            P = np.full_like(P, 1.0 / no)
        for omit in OMITS:
            score, frames, path = OR.align(P, cs, omit)
            for f in (R.align_page_omit, R.align_page_omit_closed):
                st, score2, frames2, path2 = f([P], cs, [0], [L], omit)
                assert st == R.OK and score2 == score
                here = frames[:, 0] != OR.OMITTED
                assert np.array_equal(frames2[:, 1:], frames) and (frames2[here, 0] == 0).all()
                assert (frames2[~here] == R.OMITTED).all()
                assert [s for _, _, s in path2] == path.tolist()
            seen += 1
    assert seen == 240


def _small_page(rng, trial):
    nl = int(rng.integers(1, 4))
    Ts = [int(rng.integers(1, 5)) for _ in range(nl)]
    n = int(rng.integers(1, 5))
    no = int(rng.integers(3, 6))
    cs = rng.integers(1, no, size=n)
    lo, hi = _windows(rng, nl, n)
    Ps = [FC.probs(rng, T, no, sharp=1.5) for T in Ts]
    if trial % 4 == 3:
        Ps = [np.full_like(P, 0.25) for P in Ps]
    return Ps, cs, lo, hi


def test_an_omission_dearer_than_any_path_gives_the_strict_page_alignment():
    """at most 12 frames: 12 * 17 * 65536 < 2^26, so no path with an omission beats one without; where the strict lattice
    has no path the combined rule still has one, at every price"""
    rng = np.random.default_rng(1413)
    found = nopath = 0
    for trial in range(300):
        Ps, cs, lo, hi = _small_page(rng, trial)
        st0, score0, frames0, path0 = PR.align_page(Ps, cs, lo, hi)
        for omit in (0, 3 * UNIT, 1 << 26):
            st, score, frames, path = R.align_page_omit(Ps, cs, lo, hi, omit)
            assert st == R.OK and score > R.DEAD
            assert R.path_score(Ps, cs, lo, hi, omit, path) == score
        if st0 == PR.OK:
            assert score == score0 and np.array_equal(frames, frames0) and path == path0
            found += 1
        else:
            assert (frames == R.OMITTED).any()
            nopath += 1
    assert found > 150 and nopath > 50


def _legal_paths(Ts, cs, lo, hi):
    """every path [(line, t, state)] the rule allows on a small page, by enumeration"""
    lab = FR.states(cs)
    S = len(lab)
    frames = [(k, t) for k, T in enumerate(Ts) for t in range(T)]
    out = []

    def go(i, path):
        if i == len(frames):
            out.append(list(path))
            return
        k, t = frames[i]
        if i == 0:
            nxt = list(range(S))
        else:
            s = path[-1][2]
            nxt = [] if (t == 0 and s % 2 == 1) else [s]
            nxt += [s + 1] + ([s + 2] if s % 2 == 1 and s + 2 < S and lab[s + 2] != lab[s] else [])
            nxt += [x for x in range(s + 2, S) if x not in nxt and s <= 2 * (x // 2) - 2]
        for s in nxt:
            if s < S and 2 * lo[k] <= s <= 2 * hi[k]:
                path.append((k, t, s))
                go(i + 1, path)
                path.pop()
    go(0, [])
    return out


def _enumeration_cases():
    rng = np.random.default_rng(1414)
    shapes = [(3,), (4, 5), (2, 3, 4), (1, 1, 5), (5, 1, 3), (3, 3, 3), (1, 8), (2, 2, 2, 3), (1,), (1, 1)]
    out = []
    for Ts in shapes:
        for trial in range(8):
            n = int(rng.integers(1, 4))
            no = int(rng.integers(3, 5))
            cs = rng.integers(1, no, size=n)
            lo, hi = _windows(rng, len(Ts), n)
            Ps = [FC.probs(rng, T, no, sharp=1.5) for T in Ts]
            if trial % 4 == 3:
                Ps = [np.full_like(P, 0.25) for P in Ps]                       # every candidate ties
            out.append((Ps, cs, lo, hi))
    return out


def test_small_lattices_against_every_legal_path():
    seen = 0
    for Ps, cs, lo, hi in _enumeration_cases():
        paths = _legal_paths([len(P) for P in Ps], cs, lo, hi)
        assert paths
        for omit in OMITS:
            st, score, frames, path = R.align_page_omit(Ps, cs, lo, hi, omit)
            totals = [R.path_score(Ps, cs, lo, hi, omit, p) for p in paths]
            assert None not in totals
            assert st == R.OK and score == max(totals)
            assert R.path_score(Ps, cs, lo, hi, omit, path) == score and path in paths
            for i in range(len(cs)):
                at = [(k, t) for k, t, s in path if s == 2 * i + 1]
                if not at:
                    assert frames[i].tolist() == [-1] * 4
                    continue
                assert len({k for k, _ in at}) == 1
                assert frames[i, 0] == at[0][0] and frames[i, 1] == at[0][1] and frames[i, 2] == at[-1][1]
                q = FR.q_of(Ps[at[0][0]])[at[0][1]:at[-1][1] + 1, cs[i]]
                assert frames[i, 3] == at[0][1] + int(np.argmax(q))
            seen += 1
    assert seen >= 300


def test_the_closed_form_equals_the_rule():
    rng = np.random.default_rng(1415)
    pages = _enumeration_cases()
    pages += [PC._page(rng, (12, 11), 8, (0, 4), (4, 8), 7),                  # windows that shift by many, 1 and 0 characters
              PC._page(rng, (6, 5, 7), 9, (0, 1, 1), (5, 6, 9), 7),
              PC._page(rng, (3, 2, 2), 20, (0, 5, 14), (9, 16, 20), 5),
              PC._page(rng, (9, 7, 8, 1, 15, 17), 18, (0, 1, 2, 5, 5, 11), (6, 7, 9, 9, 16, 18), 6)]
    u = lambda T: np.full((T, 4), 0.25, np.float32)                            # noqa: E731
    pages.append(([u(6), u(1), u(6)], np.asarray([1, 1, 2, 2], np.int32), [0, 1, 1], [3, 3, 4]))
    for Ps, cs, lo, hi in pages:
        for omit in OMITS + (3 * UNIT + 1,):
            a = R.align_page_omit(Ps, cs, lo, hi, omit)
            for wc in (False, True):
                b = R.align_page_omit_closed(Ps, cs, lo, hi, omit, window_coordinates=wc)
                assert a[0] == b[0] == R.OK and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_the_line_break_with_omission_on():
    """forced_page_cases.break_case: one character likely everywhere on two lines of two frames.  The strict rule makes it
    leave at the break; with omission the path may also start in the first blank and enter the character on line 1 -- but
    the character still cannot span the break."""
    Ps, cs, lo, hi = PC.break_case()
    q9, q1 = int(FR.q_of(np.float32(0.9))), int(FR.q_of(np.float32(0.1)))
    strict = PR.align_page(Ps, cs, lo, hi)
    assert strict[1] == 2 * q9 + 2 * q1
    for omit in OMITS:
        st, score, frames, path = R.align_page_omit(Ps, cs, lo, hi, omit)
        print("omit %d: strict %d, with omission %d" % (omit, strict[1], score))
        assert st == R.OK and score == strict[1]                  # no path does better: the character holds one line
        assert [s for _, _, s in path] == [1, 1, 2, 2] and frames.tolist() == [[0, 0, 1, 0]]
        assert R.path_score(Ps, cs, lo, hi, omit, [(0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 1)]) is None
    # two characters of the same likely class: omission lets the second take line 1 where the strict rule must put a
    # blank's frame between them
    cs2, lo2, hi2 = np.asarray([1, 1], np.int32), [0, 0], [2, 2]
    strict2 = PR.align_page(Ps, cs2, lo2, hi2)
    got2 = R.align_page_omit(Ps, cs2, lo2, hi2, 0)
    print("two equal characters: strict %d, omit 0 %d" % (strict2[1], got2[1]))
    assert strict2[0] == PR.OK and got2[1] >= strict2[1]


def test_page_columns_with_an_omitted_character_by_hand():
    from text_alignment_amd import forced
    # five characters; the path put 0 - 1 on line 0, omitted 2 and put 3 - 4 on line 1
    frames = np.asarray([[0, 2, 3, 3], [0, 6, 6, 6], [-1, -1, -1, -1], [1, 4, 6, 5], [1, 9, 9, 9]], np.int32)
    T, raw_w = np.asarray([12, 14]), np.asarray([40, 25])
    x_min, y_min, y_max = np.asarray([10, 100]), np.asarray([5, 50]), np.asarray([45, 90])
    ops, idx, boxes = forced.page_columns(frames, T, raw_w, x_min, y_min, y_max, 1, box_base=7)
    assert ops.tolist() == [0, 0, 1, 0, 0] and idx.tolist() == [7, 8, 9, 10]
    # x = (t_peak - pad) raw_w / (T - 2 pad): line 0 scale 4.0 -> 8, 20; line 1 scale 25/12 -> 8.3, 16.7
    assert boxes.tolist() == [[10, 5, 18, 45], [18, 5, 30, 45], [100, 50, 108, 90], [108, 50, 117, 90]]
    want = FR.peak_boxes([3, 6], 12, 40, 10, 5, 45, 1) + FR.peak_boxes([5, 9], 14, 25, 100, 50, 90, 1)
    assert [tuple(b) for b in boxes.tolist()] == want
    # without -1 rows: today's output
    full = frames.copy()
    full[2] = [1, 1, 1, 1]
    ops, idx, boxes = forced.page_columns(full, T, raw_w, x_min, y_min, y_max, 1, box_base=7)
    assert ops.tolist() == [0] * 5 and idx.tolist() == [7, 8, 9, 10, 11] and len(boxes) == 5
    # the lines of the PRESENT characters must not decrease
    bad = frames.copy()
    bad[[0, 3], 0] = [1, 0]
    with pytest.raises(ValueError):
        forced.page_columns(bad, T, raw_w, x_min, y_min, y_max, 1, box_base=7)
    # the old codes keep their numbers and their dictionary; the two new ones follow
    assert sorted(forced.PAGE_SCOPE) == list(range(8))
    assert (forced.PAGE_TOO_LONG, forced.PAGE_ALL_OMITTED) == (R.TOO_LONG, R.ALL_OMITTED) == (8, 9)
    assert sorted(forced.PAGE_OMIT_SCOPE) == list(range(10))
    assert all(forced.PAGE_OMIT_SCOPE[k] == forced.PAGE_SCOPE[k] for k in range(8) if k != forced.PAGE_FRAMES)


def test_page_omit_eligibility():
    from text_alignment_amd import forced
    rows = [[12, 3, 12], [6, 16, 8], [3, 0, 0], [4, 27, 9]]
    cls = np.ones(37, np.int32)
    f = forced.page_scope_eligibility
    assert f(True, 0, cls, rows, [9, 9, 9, 9], 2) == (PR.FRAMES, None)
    reason, win = f(True, 0, cls, rows, [9, 9, 9, 9], 2, omit=True)         # n <= frames is no longer required
    assert reason == 0 and win[0].tolist() == [0, 14, 22, 25]
    assert f(True, 0, cls, rows, [1, 1, 1, 1], 2, omit=True)[0] == 0
    assert f(False, 0, cls, rows, [9] * 4, 2, omit=True) == (PR.NOT_PLAIN, None)
    assert f(True, 0, cls[:0], rows, [9] * 4, 2, omit=True) == (PR.NO_TEXT, None)


def test_page_omit_refusals_come_before_any_work():
    """what refine_pages and process refuse about page_omit is refused on the arguments alone: no page, no model, no GPU"""
    from text_alignment_amd import alignToOCR as atocr, forced
    for kw in (dict(scope="line", page_omit=4.0), dict(page_omit=4.0), dict(scope="page", page_omit=4.0, confidence=True),
               dict(scope="page", page_omit=4.0, posterior=True), dict(scope="page", page_omit=-0.5),
               dict(scope="page", page_omit=1024.5), dict(scope="page", page_omit="4"), dict(scope="page", page_omit=True),
               dict(scope="page", page_omit=4.0, omit=2.0)):
        with pytest.raises(ValueError):
            forced.refine_pages([], [], None, **kw)
    with pytest.raises(ValueError, match="page scope has no omission") as e:          # the pinned refusal, now naming the keyword
        forced.refine_pages([], [], None, scope="page", omit=4.0)
    assert "page_omit" in str(e.value)
    with pytest.raises(ValueError, match="page_omit belongs to refine=True"):
        atocr.process(None, "", None, page_omit=4.0)
    with pytest.raises(TypeError):
        atocr.process_batch([], [], None, page_omit=4.0)


def test_the_checker_refuses_what_the_kernel_refuses():
    rng = np.random.default_rng(5)
    Ps = [FC.probs(rng, 6, 5), FC.probs(rng, 6, 5)]
    assert R.align_page_omit(Ps, [1, 2, 3, 4], [0, 2], [3, 4], 0)[0] == R.OK
    for cs, lo, hi, omit in (([1, 2, 3, 4], [1, 2], [3, 4], 0), ([1, 2, 3, 4], [0, 4], [3, 4], 0), ([1, 0, 3, 4], [0, 2], [3, 4], 0),
                             ([1, 5, 3, 4], [0, 2], [3, 4], 0), ([], [0, 0], [0, 0], 0), ([1, 2, 3, 4], [0, 2], [3, 4], -1),
                             ([1, 2, 3, 4], [0, 2], [3, 4], (1 << 26) + 1), ([1, 2, 3, 4], [0, 2], [3, 4], 1.5),
                             ([1, 2, 3, 4], [0, 2], [3, 4], True)):
        for f in (R.align_page_omit, R.align_page_omit_closed):
            with pytest.raises(ValueError):
                f(Ps, cs, lo, hi, omit)
