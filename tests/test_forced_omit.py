"""The rule of the omission-tolerant forced alignment (tests/forced_omit_ref.py) held against
the enumeration of all paths, its closed form and the strict aligner, and the host-side pieces of forced.py that go
with it -- no kernel, no GPU."""
import itertools

import numpy as np
import pytest

import forced_cases as C0
import forced_omit_ref as R
import forced_ref as R0

UNIT = 1 << 16
OMITS = (0, UNIT, 5 * UNIT, 1 << 26)


def _all_paths(T, S):
    """every never-decreasing state sequence: a superset of what the rule allows (path_score sorts out the rest)"""
    return itertools.combinations_with_replacement(range(S), T)


def _brute_cases():
    rng = np.random.default_rng(77)
    out = []
    for T in (3, 4, 5, 6, 7):
        for L in (1, 2, 3):
            if 2 * L + 1 > T:
                continue
            for rep in range(3 if T < 7 else 4):
                no = 3 + rep % 3
                cs = C0.text(rng, L, no) if rep != 1 else np.full(L, 1, np.int32)
                P = C0.probs(rng, T, no, sharp=2.0) if rep != 2 else np.full((T, no), 1.0 / no, np.float32)
                out.append((P, cs))
    return out


def test_the_rule_equals_the_enumeration_of_all_paths():
    n = 0
    for P, cs in _brute_cases():
        T, S = len(P), 2 * len(cs) + 1
        paths = list(_all_paths(T, S))
        Q = R0.q_of(P)
        for omit in OMITS:
            score, frames, path = R.align(P, cs, omit)
            totals = [R.path_score(P, cs, omit, p, Q) for p in paths]
            assert score == max(t for t in totals if t is not None)
            assert R.path_score(P, cs, omit, path) == score
            for i in range(len(cs)):                     # the frames are the path's
                ts = np.flatnonzero(path == 2 * i + 1)
                assert frames[i].tolist()[:2] == ([int(ts[0]), int(ts[-1])] if len(ts) else [-1, -1])
                assert (frames[i, 2] == -1) == (len(ts) == 0)
            n += 1
    assert n >= 120


def test_the_closed_form_equals_the_rule():
    rng = np.random.default_rng(78)
    lines = [(P, cs) for P, cs in _brute_cases()]
    lines += [(C0.probs(rng, T, 5), C0.text(rng, L, 5)) for T, L in ((20, 7), (41, 20), (64, 9), (90, 33))]
    lines += [(np.full((T, 4), 0.25, np.float32), np.asarray(cs, np.int32)) for T, cs in ((9, [1, 2, 3]), (30, [1, 1, 2, 2, 3] * 2))]
    for P, cs in lines:
        for omit in OMITS + (3 * UNIT + 1,):
            a, b = R.align(P, cs, omit), R.align_closed(P, cs, omit)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_an_omission_dearer_than_any_path_gives_the_strict_alignment():
    """omit = 2^26 and T <= 40: 40 * 17 * 65536 < 2^26, so no path with an omission can win.  Not so for long lines."""
    rng = np.random.default_rng(79)
    shapes = [(3, 1), (40, 1), (40, 19), (39, 19)]
    while len(shapes) < 40:
        T = int(rng.integers(3, 41))
        shapes.append((T, int(rng.integers(1, (T - 1) // 2 + 1))))
    for T, L in shapes:
        P, cs = C0.probs(rng, T, 6), C0.text(rng, L, 6)
        got, want = R.align(P, cs, 1 << 26), R0.align(P, cs)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_the_checker_refuses_what_the_kernel_refuses():
    P = C0.probs(np.random.default_rng(1), 9, 4)
    for cs, omit in (([], 0), ([1, 2, 3, 1, 2], 0), ([4], 0), ([0], 0), ([1], -1), ([1], (1 << 26) + 1), ([1], 1.5), ([1], True)):
        with pytest.raises(ValueError):
            R.align(P, cs, omit)


# ---- forced.py: the host-side pieces ---------------------------------------------------------------------------------------

def test_omit_units():
    from text_alignment_amd import forced
    assert forced.omit_units(0) == 0 and forced.omit_units(1) == 65536 and forced.omit_units(1024) == 1 << 26
    assert forced.omit_units(2.5) == 163840 and forced.omit_units(np.float32(0.5)) == 32768 and forced.omit_units(np.int64(3)) == 196608
    assert forced.omit_units(1e-9) == 0 and isinstance(forced.omit_units(4.0), int)
    assert forced.OMIT_MAX == 1 << 26 and forced.OMITTED == -1
    for bad in (-1e-9, -1, 1024.001, 1025, float("nan"), float("inf"), "4", None, True, [4]):
        with pytest.raises(ValueError):
            forced.omit_units(bad)


def _columns_case(rng):
    """a page's columns with two OCR lines: (ops, idx, o_line, tra, ocr, boxes)"""
    ops = np.asarray([0, 0, 1, 0, 2, 0, 0, 1, 1, 0, 0, 2, 0, 0, 1, 0], np.uint8)
    n_o = int((ops != 1).sum())
    o_line = np.asarray([0] * 5 + [1] * (n_o - 5), np.int64)
    idx = np.arange(100, 100 + n_o, dtype=np.int64)
    boxes = rng.integers(0, 500, size=(200, 4))
    return ops, idx, o_line, boxes


def test_refine_columns_with_present_mask_equals_the_per_character_rule():
    """refine_columns(present=...): a kept character the path omits becomes a transcript character alone, in its place;
    the present ones pair with consecutive new box rows.  Held against forced_ref.char_boxes with the omitted kept
    characters having no box."""
    from text_alignment_amd import forced
    rng = np.random.default_rng(80)
    ops, idx, o_line, boxes = _columns_case(rng)
    has_t = ops != 2
    n_t = int(has_t.sum())
    tra = [("t%d" % k) for k in range(n_t)]
    # line 0 owns columns 0 .. 5 (OCR characters 0 .. 4: transcript characters 0 .. 4), line 1 the columns from OCR 5 on
    t_before = np.cumsum(has_t) - has_t
    col_of_o = np.flatnonzero(ops != 1)
    for trial in range(40):
        lines, refined, masks, row = [], {}, [], 150
        for line in (0, 1):
            if rng.random() < 0.2:
                continue
            js = np.flatnonzero(o_line == line)
            c0, c1 = int(col_of_o[js[0]]), int(col_of_o[js[-1]])
            ta, tb = int(t_before[c0]), int(t_before[c1]) + int(has_t[c1])
            t_first = int(rng.integers(ta, tb))
            L = int(rng.integers(1, tb - t_first + 1))
            present = rng.random(L) < 0.6
            if not present.any():
                present[int(rng.integers(0, L))] = True
            if trial % 5 == 0:
                present[:] = True
            lines.append((line, t_first, L, row))
            masks.append(present)
            per_char = [None] * L                        # the per-character restatement: a box for the present ones only
            for k, r in zip(np.flatnonzero(present), range(row, row + int(present.sum()))):
                per_char[k] = tuple(int(v) for v in boxes[r])
            refined[line] = (t_first, L, per_char)
            row += int(present.sum())
        new_ops, new_idx = forced.refine_columns(ops, idx, o_line, lines, present=masks)
        if all(m.all() for m in masks):
            same = forced.refine_columns(ops, idx, o_line, lines)
            assert np.array_equal(same[0], new_ops) and np.array_equal(same[1], new_idx)
        assert int((new_ops != 2).sum()) == n_t and int((new_ops != 1).sum()) == len(new_idx)
        # boxes per transcript character from the new columns ...
        got, j = [], 0
        for op in new_ops:
            if op == 0:
                got.append(tuple(int(v) for v in boxes[new_idx[j]]))
            elif op == 1:
                got.append(None)
            if op != 1:
                j += 1
        # ... and from the rule: char_boxes over the ORIGINAL columns
        tra_cols, ocr_cols, ti, oj = [], [], 0, 0
        for op in ops:
            tra_cols.append(tra[ti] if op != 2 else None)
            ocr_cols.append("o" if op != 1 else None)
            ti += op != 2
            oj += op != 1
        want = _char_boxes_with_gaps(tra_cols, ocr_cols, o_line, boxes[idx], refined)
        assert got == want, (trial, lines, masks)
    with pytest.raises(ValueError):
        forced.refine_columns(ops, idx, o_line, [(0, 0, 2, 150)], present=[np.asarray([True])])
    with pytest.raises(ValueError):
        forced.refine_columns(ops, idx, o_line, [(0, 0, 2, 150)], present=[])


def _char_boxes_with_gaps(tra, ocr, o_line, ocr_boxes, refined):
    """forced_ref.char_boxes where a refined line's `boxes` may hold None for a kept character the path omitted"""
    kept = {}
    for t_first, L, boxes in refined.values():
        for k in range(L):
            kept[t_first + k] = boxes[k]
    out, i, j = [], 0, 0
    for t, o in zip(tra, ocr):
        if t is not None:
            if i in kept:
                out.append(kept[i])
            elif o is not None and o_line[j] not in refined:
                out.append(tuple(int(v) for v in ocr_boxes[j]))
            else:
                out.append(None)
            i += 1
        if o is not None:
            j += 1
    return out


def test_char_boxes_restatement_is_forced_refs_rule_when_nothing_is_omitted():
    rng = np.random.default_rng(81)
    ops, idx, o_line, boxes = _columns_case(rng)
    tra = [("t" if op != 2 else None) for op in ops]
    ocr = [("o" if op != 1 else None) for op in ops]
    refined = {1: (6, 3, [tuple(int(v) for v in boxes[150 + k]) for k in range(3)])}
    assert _char_boxes_with_gaps(tra, ocr, o_line, boxes[idx], refined) == R0.char_boxes(tra, ocr, o_line, boxes[idx], refined)
