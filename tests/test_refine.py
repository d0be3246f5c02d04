"""tests/refine_ref.py, the checker of record for ta_refine_columns, pinned to forced.refine_columns -- the host function
whose rule the kernel restates -- on the 120 random pages tests/test_forced.py holds that function against the
per-character rule with.  The two number the new box rows differently (refine_columns takes each line's first row from
its caller, the device path puts slot k's rows at box_base + lab_off[k]), so rows are compared by the boxes they point
at."""
import numpy as np

import forced_ref as FR
import harvest_ref as H
import refine_ref as R
from test_forced import _ocr_boxes, _random_page


def test_checker_equals_refine_columns_on_random_pages():
    from text_alignment_amd import forced
    rng = np.random.default_rng(77)
    refined_lines = pages_with = grew = 0
    for _ in range(120):
        pg, ops = _random_page(rng)
        tra, ocr = H.aligned_from_ops(ops.tolist(), pg["t"].tolist(), pg["o"].tolist())
        o_line = pg["o_line"].tolist()
        rows = H.harvest_page(tra, ocr, o_line, 0, pg["lines"], pg["t_class"].tolist(), pg["T"].tolist(), 3, 5)
        m = len(o_line)
        old = np.asarray(_ocr_boxes(o_line), dtype=np.int64).reshape(-1, 4)
        idx = rng.permutation(m + 5)[:m].astype(np.int64)
        boxes = np.full((m + 5, 4), -1, dtype=np.int64)
        boxes[idx] = old
        # the host path: rows handed out line after line; the device path: a slot per chosen line, rows at lab_off with gaps
        lines, slots, extra, dev_rows, off = [], {}, [], {}, 2
        for l in range(pg["lines"]):
            if rows[l][0] == 0 and rng.random() < 0.8:
                L = rows[l][2]
                new = [(1000 * l + 3 * k, 50 * l + 1, 1000 * l + 3 * k + 3, 50 * l + 41) for k in range(L)]
                lines.append((l, rows[l][1], L, len(boxes) + len(extra)))
                extra += new
                slots[l] = (len(slots), L, off, FR.OK)
                for k in range(L):
                    dev_rows[len(boxes) + off + k] = new[k]
                off += L + 1
        host_boxes = np.concatenate([boxes, np.asarray(extra, dtype=np.int64).reshape(-1, 4)])
        dev_boxes = np.full((len(boxes) + off, 4), -7, dtype=np.int64)
        dev_boxes[:len(boxes)] = boxes
        for r, b in dev_rows.items():
            dev_boxes[r] = b
        ops2, idx2 = forced.refine_columns(ops, idx, pg["o_line"], lines)
        st, ops3, idx3, mine = R.refine_page(ops, idx, o_line, len(pg["t"]), 0, pg["lines"], rows, slots, True, len(boxes), off)
        assert st == R.OK and sorted(mine) == [l for l, _, _, _ in lines]
        assert ops3 == ops2.tolist() and len(idx3) == len(idx2)
        assert np.array_equal(dev_boxes[idx3], host_boxes[idx2])
        refined_lines += len(lines)
        pages_with += bool(lines)
        grew += len(idx3) > m
        # the predicate: a page that is not plain, a slot the forced alignment refused, a text over the limit
        assert R.refine_page(ops, idx, o_line, len(pg["t"]), 0, pg["lines"], rows, slots, False, len(boxes), off)[1:] == \
            (ops.tolist(), idx.tolist(), {})
        if lines:
            l0 = lines[0][0]
            for bad in ((slots[l0][0], slots[l0][1], slots[l0][2], FR.BOUNDS), (slots[l0][0], R.MAX_TARGET + 1, slots[l0][2], 0)):
                st, ops4, idx4, mine4 = R.refine_page(ops, idx, o_line, len(pg["t"]), 0, pg["lines"], rows, {**slots, l0: bad},
                                                      True, len(boxes), off)
                ops5, idx5 = forced.refine_columns(ops, idx, pg["o_line"], lines[1:])
                assert st == R.OK and l0 not in mine4 and ops4 == ops5.tolist()
                assert np.array_equal(dev_boxes[idx4], host_boxes[idx5])
    assert refined_lines > 60 and pages_with > 40
    assert grew > 0                      # a refined line can carry more pairs than it had OCR characters


def test_checker_refuses_what_refine_columns_refuses():
    import pytest
    from text_alignment_amd import forced
    ops = np.asarray([0, 0, 0, 1, 0, 0], np.uint8)
    o_line, idx = [0, 0, 0, 1, 1], np.arange(5)
    table = [[0, 0, 3], [0, 3, 3]]
    slots = {0: (0, 3, 0, 0), 1: (1, 3, 3, 0)}
    # line 1's run starts at transcript character 4: the op-1 column in front of it belongs to no line
    with pytest.raises(ValueError):
        forced.refine_columns(ops, idx, o_line, [(1, 3, 3, 10)])
    assert R.refine_page(ops, idx, o_line, 6, 0, 2, table, slots, True, 5, 6)[0] == R.CONTAIN
    table[1] = [0, 4, 2]
    slots[1] = (1, 2, 3, 0)
    st, new_ops, new_idx, mine = R.refine_page(ops, idx, o_line, 6, 0, 2, table, slots, True, 5, 6)
    assert (st, new_ops, new_idx, mine) == (R.OK, [0, 0, 0, 1, 0, 0], [5, 6, 7, 8, 9], {0: 0, 1: 1})


class _Rec(object):
    def __init__(self, codec):
        self.model = type("M", (), {"codec": codec})()


def test_refine_checks_refuse_up_front():
    """what process_batch(refine=True) refuses before any GPU work -- refine_pages' refusals"""
    import pytest
    from text_alignment_amd import forced
    codec = ["", " ", "~"] + list("abcdefgh")
    ints = [8, -12, -6, -6, -2, -2]
    assert forced.refine_checks(ints, [_Rec(codec)], 0.9) == (9, 10)
    assert forced.refine_checks(None, [_Rec(codec), _Rec(codec)], (4, 5)) == (4, 5)
    for params, codecs, agreement in (([8.5, -12, -6, -6, -2, -2], [codec], 0.9), ([lambda a, b: 1, -6, -6, -2, -2], [codec], 0.9),
                                      (ints, [codec, codec[:5] + ["ab"]], 0.9),       # a multi-character entry
                                      (ints, [["", "a", " "]], 0.9),                 # the space is not class 1
                                      (ints, [codec], 0), (ints, [codec], 1.5), (ints, [codec], (5, 4)), (ints, [codec], "much"),
                                      (ints, [codec], (1, 10 ** 7))):
        with pytest.raises(ValueError):
            forced.refine_checks(params, [_Rec(c) for c in codecs], agreement)


def test_line_caps_and_workspace_pieces():
    from text_alignment_amd import forced
    T = np.asarray([1432, 3, 2, 1, 4000, 90], np.int32)
    caps = forced.line_caps(T, [0, 2, 4, 6], ["x" * 2000, "", "abcde"])
    assert caps.tolist() == [715, 1, 0, 0, 5, 5] and caps.dtype == np.int32
    off, total = forced.workspace_pieces(T, caps)
    f = forced._native.lib.ta_forced_workspace_bytes
    sizes = [f(1432, 715), f(3, 1), 0, 0, f(4000, 5), f(90, 5)]
    assert off.tolist() == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist() and total == sum(sizes)
    assert all(o % 16 == 0 for o in off.tolist()) and f(1432, 715) == 256 * 2 * 1432
    assert forced.line_caps(np.asarray([5000], np.int32), [0, 1], ["y" * 5000]).tolist() == [forced.MAX_TARGET]
