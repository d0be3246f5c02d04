# -*- coding: utf-8 -*-
"""Host semantics of evaluate_text_alignment against the reference's evaluation (tests/golden/eval.json, written by
tools/gen_golden_eval.py from the imported reference), its quirks on hand-made cases, and the argument checks of the
evaluation kernels' entry points (no GPU needed)."""
import base64
import itertools
import json
import os
import zlib

import numpy as np
import pytest

from text_alignment_amd import _native
from text_alignment_amd import evaluate_text_alignment as eta
from text_alignment_amd.alignToOCR import CharBox

GOLD = os.path.join(os.path.dirname(__file__), "golden", "eval.json")


@pytest.fixture(scope="module")
def gold():
    with open(GOLD, encoding="utf-8") as f:
        return json.load(f)


def unpack_ink(rec):
    h, w = rec["shape"]
    bits = np.frombuffer(zlib.decompress(base64.b64decode(rec["bits"])), dtype=np.uint8)
    return np.unpackbits(bits)[:h * w].reshape(h, w).astype(bool)


def box(syl, ul, lr, difficult=0):
    return {"syl": syl, "ul": tuple(ul), "lr": tuple(lr), "difficult": difficult}


def test_read_gt_boxes_fixture(gold, tmp_path):
    xml = gold["pages"][0]["xml"]
    boxes = eta.read_gt_boxes(xml)
    assert len(boxes) == xml.count("<object>")
    assert set(boxes[0]) == {"syl", "difficult", "ul", "lr"}
    assert any(b["difficult"] for b in boxes) and any(b["syl"] == "a" for b in boxes)
    p = tmp_path / "x_gt.xml"
    p.write_text(xml.replace("<annotation>", "<annotation>\n  <folder>f</folder>"))
    assert eta.read_gt_boxes(str(p)) == boxes           # only <object> children are read


def test_direct_cases(gold):
    ink = unpack_ink(gold["pages"][0]["ink"])
    for c in gold["direct"]:
        a = {"ul": tuple(c["a"][:2]), "lr": tuple(c["a"][2:])}
        b = {"ul": tuple(c["b"][:2]), "lr": tuple(c["b"][2:])}
        assert eta.intersect(a, b) == c["intersect"] and type(eta.intersect(a, b)) is type(c["intersect"])
        assert eta.IOU(a, b) == c["iou"]
        if isinstance(c["black_iou"], str):
            with pytest.raises({"RuntimeError": RuntimeError, "ZeroDivisionError": ZeroDivisionError}[c["black_iou"]]):
                eta.black_area_IOU(a, b, ink)
        else:
            assert eta.black_area_IOU(a, b, ink) == c["black_iou"]
            assert eta.black_area_IOU(a, b, ink.astype(np.uint8) * 7) == c["black_iou"]


def test_score_alignment_equals_reference(gold):
    n = 0
    for pg in gold["pages"]:
        ink = unpack_ink(pg["ink"])
        gt = eta.read_gt_boxes(pg["xml"])
        for i, syl_boxes in pg["syl_boxes"].items():
            iou, area = eta.score_alignment(gt, syl_boxes, ink)
            assert iou == pg["iou"][int(i)] and area == pg["area"][int(i)]
            n += 1
    assert n == 3 * len(gold["sample_systems"])


def test_default_grid(gold):
    g = eta.default_grid()
    assert g.shape == (729, 6) and g.dtype == np.int64
    assert g.tolist() == [list(p) for p in itertools.product(*gold["grid"])]


def test_score_alignment_quirks():
    ink = np.zeros((50, 60), dtype=bool)
    ink[10:20, 10:20] = True
    ink[30:40, 30:50] = True
    pred = [box("do", (10, 10), (20, 20)), box("mi", (30, 30), (50, 40)), box("do", (12, 12), (20, 20))]
    # difficult boxes are skipped before they can overwrite anything
    a = eta.score_alignment([box("do", (10, 10), (20, 20)), box("do", (30, 30), (50, 40), 1)], pred, ink)
    assert a == (1.0, 1.0)
    # counted with eval_difficult: it overwrites (no overlap with a 'do' box -> 0)
    assert eta.score_alignment([box("do", (10, 10), (20, 20)), box("do", (30, 30), (50, 40), 1)], pred, ink,
                               eval_difficult=True) == (0.0, 0.0)
    # first maximum of the intersections: both 'do' boxes meet (12..20)^2 equally -> the first one
    iou, _ = eta.score_alignment([box("do", (12, 12), (20, 20))], pred, ink)
    assert iou == 64.0 / 100.0
    # containment both ways: 'o' is in 'do'; 'domi' contains 'do' and 'mi'
    assert eta.score_alignment([box("o", (10, 10), (20, 20))], pred, ink) == (1.0, 1.0)
    assert eta.score_alignment([box("domi", (30, 30), (50, 40))], pred, ink) == (1.0, 1.0)
    # no candidate / no overlap: 0
    assert eta.score_alignment([box("zz", (10, 10), (20, 20))], pred, ink) == (0.0, 0.0)
    assert eta.score_alignment([box("mi", (0, 0), (5, 5))], pred, ink) == (0.0, 0.0)
    # a later box of the same name overwrites the value, the name keeps its first position
    r = eta.score_alignment([box("do", (0, 0), (5, 5)), box("mi", (30, 30), (50, 40)), box("do", (10, 10), (20, 20))],
                            pred, ink)
    assert r == (np.mean([1.0, 1.0]), np.mean([1.0, 1.0]))
    vals = [eta.IOU(box("do", (10, 10), (19, 20)), pred[0]), 0.0, 1.0]
    r = eta.score_alignment([box("do", (0, 0), (5, 5)), box("mi", (0, 0), (5, 5)), box("do", (10, 10), (19, 20)),
                             box("ra", (0, 0), (3, 3)), box("mi", (30, 30), (50, 40))], pred, ink)
    assert r[0] == np.mean([vals[0], 1.0, 0.0])
    # nothing scored: numpy's nan
    with np.errstate(all="ignore"), pytest.warns(RuntimeWarning):
        r = eta.score_alignment([box("do", (10, 10), (20, 20), 1)], pred, ink)
    assert np.isnan(r[0]) and np.isnan(r[1])


def test_score_alignment_raising_cases():
    ink = np.zeros((50, 60), dtype=bool)
    ink[10:20, 10:20] = True
    # a predicted box off the page: Gamera's view constructor raises
    with pytest.raises(RuntimeError):
        eta.score_alignment([box("do", (0, 0), (10, 10))], [box("do", (-5, -5), (8, 8))], ink)
    # blank paper under both boxes: 0 / 0
    with pytest.raises(ZeroDivisionError):
        eta.score_alignment([box("do", (30, 30), (40, 40))], [box("do", (32, 32), (45, 45))], ink)
    # inclusive counts: a box ending where the ink starts still sees its first row and column
    assert eta.black_area_IOU({"ul": (0, 0), "lr": (10, 10)}, {"ul": (10, 10), "lr": (10, 10)}, ink) == 1.0


def test_sweep_page_host_errors():
    chars = [CharBox(c, (10 * k, 0), (10 * k + 8, 20)) for k, c in enumerate("do_minus")]
    with pytest.raises(AssertionError):
        eta.SweepPage(chars, "dominus", [], 0, (100, 50), (100, 50), np.zeros((50, 100))).prepared()
    chars = [CharBox(c, (10 * k, 0), (10 * k + 8, 20)) for k, c in enumerate("dominus")]
    pg = eta.SweepPage(chars, "dominus", [], 0, (100, 50), (100, 50), np.zeros((50, 100)))
    q = pg.prepared()
    assert q["names"] == ["do", "mi", "nus"] and q["first"].tolist() == [0, 2, 4]
    # abbreviation expansion lends the abbreviation's boxes to its segments
    pg = eta.SweepPage([CharBox(c, (10 * k, 0), (10 * k + 8, 20)) for k, c in enumerate("dns")], "dominus", [], 0,
                       (100, 50), (100, 50), np.zeros((50, 100)))
    assert pg.prepared()["boxes"][:, 0].tolist() == [0, 0, 10, 10, 20, 20, 20]
    with pytest.raises(ValueError):
        eta._systems_array([[8, -4, -7, -7, -3, 0.5]])
    with pytest.raises(ValueError):
        eta._systems_array([[lambda a, b: 1, -7, -7, -3, 0]])
    assert eta._systems_array([[10, -5, -7, -1]]).tolist() == [[10, -5, -7, -7, -1, -1]]


def test_representatives_and_candidates():
    chars = [CharBox(c, (10 * k, 0), (10 * k + 8, 20)) for k, c in enumerate("dominus a")]
    gt = [box("do", (0, 0), (1, 1)), box("a", (0, 0), (2, 2)), box("x", (0, 0), (3, 3), 1), box("do", (5, 5), (9, 9)),
          box("minus", (0, 0), (4, 4))]
    pg = eta.SweepPage(chars, "dominus a", gt, 0, (100, 50), (100, 50), np.zeros((50, 100)))
    names, boxes, cands, pick = pg.representatives()
    assert names == ["do", "a", "minus"]
    assert boxes.tolist() == [[0, 0, 1, 1], [0, 0, 2, 2], [5, 5, 9, 9], [0, 0, 4, 4]]
    assert [c.tolist() for c in cands] == [[0], [3], [0], [1, 2]]
    assert pick.tolist() == [2, 1, 3]                   # the LAST box of each name, names in first-counted order
    assert len(pg.representatives(eval_difficult=True)[1]) == 5


def test_eval_argument_errors_without_gpu():
    lib = _native.lib
    ptr = np.zeros(1, dtype=np.uint64)
    hh, ww = np.array([50000], np.int32), np.array([50000], np.int32)
    calls = [
        lambda: lib.ta_eval_integral(1, None, None, None, None, None),
        lambda: lib.ta_eval_syllable_boxes(None, None, None, None, None, 1, None, None, None, None, None, None, None,
                                           4, 100, None, None, None, None),
        lambda: lib.ta_eval_score(1, None, None, None, None, 4, None, None, None, None, None, None, None, None, 4,
                                  None, None, None, None),
    ]
    for call in calls:
        assert call() == _native.TA_EINVAL
        assert b"null" in lib.ta_last_error()
    # negative counts
    assert lib.ta_eval_integral(-1, None, None, None, None, None) == _native.TA_EINVAL
    assert lib.ta_eval_syllable_boxes(None, None, None, None, None, -1, None, None, None, None, None, None, None,
                                      4, 100, None, None, None, None) == _native.TA_EINVAL
    assert lib.ta_eval_score(1, None, None, None, None, -4, None, None, None, None, None, None, None, None, 4,
                             None, None, None, None) == _native.TA_EINVAL
    # a page over 2^31 - 1 pixels
    assert lib.ta_eval_integral(1, ptr.ctypes.data, hh.ctypes.data, ww.ctypes.data, ptr.ctypes.data, None) == _native.TA_EINVAL
    assert b"2^31" in lib.ta_last_error()
    # a problem too large for the LDS of the box kernel: TA_ELIMIT, before any device work
    dummy = np.zeros(8, dtype=np.int64)
    d = dummy.ctypes.data
    big = lib.ta_eval_max_columns() + 1
    assert lib.ta_eval_syllable_boxes(d, d, d, d, d, 1, d, d, d, d, d, d, d, 4, big, d, d, d, None) == _native.TA_ELIMIT
    with pytest.raises(Exception):
        _native.check(_native.TA_ELIMIT, "ta_eval_syllable_boxes")
    # nothing to do is fine
    assert lib.ta_eval_integral(0, None, None, None, None, None) == _native.TA_OK
    assert lib.ta_eval_score(0, None, None, None, None, 4, None, None, None, None, None, None, None, None, 4,
                             None, None, None, None) == _native.TA_OK
