"""tests/forced_page_ref.py, the specification of record of page-scope forced alignment, held
against what it must satisfy: a page of one line is forced_ref.align, small lattices against the enumeration of every
legal path, the rule of the line break, the windows from harvest rows -- and forced.page_windows / the column
replacement of a page against hand-made answers.  No GPU."""
import numpy as np
import pytest

import forced_cases as FC
import forced_page_cases as C
import forced_page_ref as R
import forced_ref as FR


def test_a_page_of_one_line_is_the_line_alignment():
    seen = 0
    for name, no, lines in FC.cases():
        for P, cs in lines:
            if 2 * len(cs) + 1 > len(P):
                continue
            score, frames, path = FR.align(P, cs)
            st, score2, frames2, path2 = R.align_page([P], cs, [0], [len(cs)])
            assert st == R.OK and score2 == score
            assert np.array_equal(frames2[:, 1:], frames) and (frames2[:, 0] == 0).all()
            assert [s for _, _, s in path2] == path.tolist()
            seen += 1
    assert seen > 30


def _legal_paths(Ts, cs, lo, hi):
    """every legal path [(line, t, state)] of a small page, by enumeration"""
    lab = FR.states(cs)
    S = len(lab)
    frames = [(k, t) for k, T in enumerate(Ts) for t in range(T)]
    out = []

    def go(i, path):
        if i == len(frames):
            if path[-1][2] in (S - 1, S - 2):
                out.append(list(path))
            return
        k, t = frames[i]
        if i == 0:
            nxt = [0, 1]
        else:
            s = path[-1][2]
            nxt = [s, s + 1] + ([s + 2] if s % 2 == 1 and s + 2 < S and lab[s + 2] != lab[s] else [])
            if t == 0 and s % 2 == 1:
                nxt.remove(s)
        for s in nxt:
            if s < S and 2 * lo[k] <= s <= 2 * hi[k]:
                path.append((k, t, s))
                go(i + 1, path)
                path.pop()
    go(0, [])
    return out


def test_small_lattices_against_every_legal_path():
    rng = np.random.default_rng(31)
    shapes = [(3,), (4, 5), (2, 3, 4), (1, 1, 5), (5, 1, 3), (3, 3, 3), (1, 8), (2, 2, 2, 3)]      # at most 9 frames in all
    found = nopath = 0
    for Ts in shapes:
        for trial in range(12):
            n = int(rng.integers(1, 4))
            no = int(rng.integers(3, 5))
            cs = rng.integers(1, no, size=n)
            nl = len(Ts)
            # random windows that keep the conditions
            lo, hi = [0], [int(rng.integers(0, n + 1))]
            for k in range(1, nl):
                a = int(rng.integers(lo[-1], hi[-1] + 1))
                b = int(rng.integers(hi[-1], n + 1))
                lo.append(a)
                hi.append(b)
            hi[-1] = n
            assert R.windows_ok(lo, hi, n)
            Ps = [C.probs(rng, T, no, sharp=1.5) for T in Ts]
            if trial % 4 == 3:
                Ps = [np.full_like(P, 0.25) for P in Ps]                       # every candidate ties
            st, score, frames, path = R.align_page(Ps, cs, lo, hi)
            paths = _legal_paths(Ts, cs, lo, hi)
            totals = [R.path_score(Ps, cs, lo, hi, p) for p in paths]
            assert None not in totals
            if not paths:
                assert st == R.NOPATH
                nopath += 1
                continue
            assert st == R.OK and score == max(totals)
            assert R.path_score(Ps, cs, lo, hi, path) == score
            assert path in paths
            for i in range(n):
                at = [(k, t) for k, t, s in path if s == 2 * i + 1]
                assert len({k for k, _ in at}) == 1
                assert frames[i, 0] == at[0][0] and frames[i, 1] == at[0][1] and frames[i, 2] == at[-1][1]
                q = FR.q_of(Ps[at[0][0]])[at[0][1]:at[-1][1] + 1, cs[i]]
                assert frames[i, 3] == at[0][1] + int(np.argmax(q))
            found += 1
    assert found > 40 and nopath > 3


def test_no_character_spans_a_line_break():
    Ps, cs, lo, hi = C.break_case()
    st, score, frames, path = R.align_page(Ps, cs, lo, hi)
    st2, free, _, path2 = R.align_page(Ps, cs, lo, hi, line_stay=True)
    assert st == st2 == R.OK
    assert [s for _, _, s in path2] == [1, 1, 1, 1] and free == 4 * int(FR.q_of(np.float32(0.9)))
    assert score < free                                   # the rule costs the page its best unconstrained path
    assert score == 2 * int(FR.q_of(np.float32(0.9))) + 2 * int(FR.q_of(np.float32(0.1)))
    assert [s for _, _, s in path] == [1, 1, 2, 2] and frames.tolist() == [[0, 0, 1, 0]]     # ties: stay first
    assert R.path_score(Ps, cs, lo, hi, path2) is None


def test_the_shared_cases_cover_what_they_are_meant_to():
    status = {name: [w[0] for w in C.want(name, pages)] for name, no, pages in C.cases()
              if not name.startswith("window")}
    assert status.pop("no path") == [R.NOPATH, R.OK, R.NOPATH]
    assert all(s == R.OK for st in status.values() for s in st), status
    by = {name: pages for name, _, pages in C.cases()}
    for pg, (st, score, frames) in zip(by["ends in 2n-1"], C.want("ends in 2n-1", by["ends in 2n-1"])):
        path = R.align_page(*pg)[3]
        assert path[-1][2] == 2 * len(pg[1]) - 1
    # pages whose characters are spread over their lines, with characters that a window offered to two lines
    spread = [len(set(w[2][:, 0].tolist())) for w in C.want("overlaps", by["overlaps"]) + C.want("straddling", by["straddling"])]
    assert max(spread) >= 4 and sum(s >= 2 for s in spread) >= 8


def test_refusals_of_the_checker():
    rng = np.random.default_rng(5)
    Ps = [C.probs(rng, 6, 5), C.probs(rng, 6, 5)]
    cs = [1, 2, 3, 4]
    assert R.align_page(Ps, cs, [0, 2], [3, 4])[0] == R.OK
    for lo, hi in (([1, 2], [3, 4]), ([0, 2], [3, 3]), ([0, 4], [3, 4]), ([2, 0], [3, 4]), ([0, 2], [4, 3]), ([0], [4])):
        with pytest.raises(ValueError):
            R.align_page(Ps, cs, lo, hi)
    assert not R.windows_ok([0, 0], [1024, 1024], 1024) and R.windows_ok([0, 1], [1023, 1024], 1024)
    for bad in ([1, 0, 3, 4], [1, 5, 3, 4]):
        with pytest.raises(ValueError):
            R.align_page(Ps, bad, [0, 2], [3, 4])
    with pytest.raises(ValueError):
        R.align_page(Ps, [], [0, 0], [0, 0])


# DESIGN.md section 14.6's worked example: fields 0 - 2 of its four rows, a transcript of 37 characters
EXAMPLE = [[12, 3, 12], [6, 16, 8], [3, 0, 0], [4, 27, 9]]


def test_page_windows_by_hand():
    f = R.page_windows
    lo, hi = f(EXAMPLE, 37, 0)
    assert lo.tolist() == [0, 15, 24, 24] and hi.tolist() == [15, 24, 24, 37]
    lo, hi = f(EXAMPLE, 37, 2)
    assert lo.tolist() == [0, 14, 22, 25] and hi.tolist() == [17, 26, 26, 37]
    lo, hi = f(EXAMPLE, 37)                               # the default margin of 16
    assert lo.tolist() == [0, 0, 8, 11] and hi.tolist() == [31, 37, 37, 37]
    # leading and trailing lines without text, one marked PAGE: empty cores at the previous core's end
    rows = [[1, 0, 0], [64, 5, 2], [0, 2, 6], [1, 0, 0], [1, 0, 0]]
    lo, hi = f(rows, 10, 0)
    assert lo.tolist() == [0, 0, 0, 8, 8] and hi.tolist() == [0, 0, 8, 8, 10]
    lo, hi = f(rows, 10, 1)
    assert lo.tolist() == [0, 0, 1, 7, 7] and hi.tolist() == [1, 1, 9, 9, 10]
    # one line takes everything; every result keeps the conditions
    assert [a.tolist() for a in f([[0, 4, 3]], 12, 0)] == [[0], [12]]
    assert f([[0, 0, 1100]], 1100, 0) is None and f([[0, 0, 500], [0, 500, 600]], 1100, 0) is not None
    assert f([[0, 0, 500], [0, 500, 600]], 1100, 500) is None
    rng = np.random.default_rng(2)
    for _ in range(200):
        nl, n = int(rng.integers(1, 7)), int(rng.integers(1, 60))
        rows = [[int(rng.choice([0, 1, 2, 4, 64, 12])), int(rng.integers(0, n)), int(rng.integers(0, 12))] for _ in range(nl)]
        rows = [[r, t, min(L, n - t)] for r, t, L in rows]
        lo, hi = f(rows, n, int(rng.integers(0, 20)))
        assert R.windows_ok(lo, hi, n)
    with pytest.raises(ValueError):
        f(EXAMPLE, 37, -1)


def test_forced_page_windows_equals_the_checker():
    from text_alignment_amd import forced
    rng = np.random.default_rng(3)
    for trial in range(300):
        nl, n = int(rng.integers(1, 9)), int(rng.integers(1, 2500))
        rows = np.zeros((nl, 8), np.int32)
        rows[:, 0] = rng.choice([0, 1, 2, 4, 8, 64, 65, 6], size=nl)
        rows[:, 1] = np.sort(rng.integers(0, n, size=nl)) if trial % 2 else rng.integers(0, n, size=nl)
        rows[:, 2] = np.minimum(rng.integers(0, 700, size=nl), n - rows[:, 1])
        rows[:, 3:] = rng.integers(0, 50, size=(nl, 5))
        margin = int(rng.choice([0, 1, 16, 300]))
        want, got = R.page_windows(rows[:, :3], n, margin), forced.page_windows(rows, n, margin)
        assert (want is None) == (got is None)
        if want is not None:
            assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
            assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert forced.page_windows(EXAMPLE, 37)[1].tolist() == [31, 37, 37, 37]
    with pytest.raises(ValueError):
        forced.page_windows(EXAMPLE, 37, -1)


def test_page_columns_of_a_two_line_page_by_hand():
    """the column replacement at page scope: n pair columns whose boxes come from the frames, line by line"""
    from text_alignment_amd import forced
    # five characters; the path put 0 - 1 on line 0 and 2 - 4 on line 1
    frames = np.asarray([[0, 2, 3, 3], [0, 6, 6, 6], [1, 1, 1, 1], [1, 4, 6, 5], [1, 9, 9, 9]], np.int32)
    T, raw_w = np.asarray([12, 14]), np.asarray([40, 25])
    x_min, y_min, y_max = np.asarray([10, 100]), np.asarray([5, 50]), np.asarray([45, 90])
    pad = 1
    ops, idx, boxes = forced.page_columns(frames, T, raw_w, x_min, y_min, y_max, pad, box_base=7)
    assert ops.tolist() == [0] * 5 and idx.tolist() == [7, 8, 9, 10, 11]
    # x = (t_peak - pad) raw_w / (T - 2 pad): line 0 scale 4.0 -> 8, 20; line 1 scale 25/12 -> 0.0, 8.3, 16.7
    assert boxes.tolist() == [[10, 5, 18, 45], [18, 5, 30, 45],
                              [100, 50, 100, 90], [100, 50, 108, 90], [108, 50, 117, 90]]
    want = FR.peak_boxes([3, 6], 12, 40, 10, 5, 45, pad) + FR.peak_boxes([1, 5, 9], 14, 25, 100, 50, 90, pad)
    assert [tuple(b) for b in boxes.tolist()] == want
    # a line that received no character contributes no box
    frames2 = frames.copy()
    frames2[:, 0] *= 2
    ops, idx, boxes2 = forced.page_columns(frames2, np.asarray([12, 99, 14]), np.asarray([40, 7, 25]), np.asarray([10, 0, 100]),
                                           np.asarray([5, 0, 50]), np.asarray([45, 9, 90]), pad, box_base=0)
    assert boxes2.tolist() == boxes.tolist() and idx.tolist() == [0, 1, 2, 3, 4]


def test_page_scope_eligibility_and_reason_codes():
    from text_alignment_amd import forced
    assert (forced.PAGE_REFINED, forced.PAGE_NOT_PLAIN, forced.PAGE_HARVEST, forced.PAGE_CLASS0, forced.PAGE_NO_TEXT,
            forced.PAGE_WINDOWS, forced.PAGE_FRAMES, forced.PAGE_NO_PATH) == \
        (R.REFINED, R.NOT_PLAIN, R.HARVEST, R.CLASS0, R.NO_TEXT, R.WINDOWS, R.FRAMES, R.NO_PATH)
    assert (forced.PAGE_FIELDS, forced.NOPATH, forced.DEFAULT_MARGIN) == (R.FIELDS, R.NOPATH, 16)
    assert sorted(forced.PAGE_SCOPE) == list(range(8)) and sorted(forced.PAGE_STATUS) == [0, 1, 2, 3]
    f = forced.page_scope_eligibility
    cls = np.ones(37, np.int32)
    T = [40, 40, 40, 19]
    reason, win = f(True, 0, cls, EXAMPLE, T, 2)
    assert reason == 0 and win[0].tolist() == [0, 14, 22, 25] and win[1].tolist() == [17, 26, 26, 37]
    assert f(False, 0, cls, EXAMPLE, T, 2) == (R.NOT_PLAIN, None) and f(True, 2, cls, EXAMPLE, T, 2) == (R.HARVEST, None)
    bad = cls.copy()
    bad[5] = 0
    assert f(True, 0, bad, EXAMPLE, T, 2) == (R.CLASS0, None)
    assert f(True, 0, cls[:0], EXAMPLE, T, 2) == (R.NO_TEXT, None) and f(True, 0, cls, EXAMPLE[:0], T[:0], 2) == (R.WINDOWS, None)
    assert f(True, 0, np.ones(1100, np.int32), [[0, 0, 1100]], [3000], 0) == (R.WINDOWS, None)
    assert f(True, 0, cls, EXAMPLE, [9, 9, 9, 9], 2) == (R.FRAMES, None)
    assert f(True, 0, cls, EXAMPLE, [9, 9, 10, 9], 2)[0] == 0              # n == frames: eligible, the lattice decides
