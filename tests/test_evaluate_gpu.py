# -*- coding: utf-8 -*-
"""The scoring-system sweep on the device (evaluate_text_alignment.sweep, csrc/ta_eval.hip) against the reference's
own evaluation (tests/golden/eval.json) and against the package's host path at page size."""
import base64
import json
import os
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from text_alignment_amd import _native  # noqa: E402
from text_alignment_amd import evaluate_text_alignment as eta  # noqa: E402
from text_alignment_amd import latinSyllabification as latsyl  # noqa: E402
from text_alignment_amd import page_batch  # noqa: E402
from text_alignment_amd.alignToOCR import CharBox  # noqa: E402
from text_alignment_amd.page import Dim  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden", "eval.json")
pytestmark = pytest.mark.gpu


def unpack_ink(rec):
    h, w = rec["shape"]
    bits = np.frombuffer(zlib.decompress(base64.b64decode(rec["bits"])), dtype=np.uint8)
    return np.unpackbits(bits)[:h * w].reshape(h, w).astype(bool)


def fixture_page(pg):
    chars = [CharBox(c, tuple(ul), tuple(lr)) for c, ul, lr in pg["chars"]]
    return eta.SweepPage(chars, pg["transcript"], eta.read_gt_boxes(pg["xml"]), pg["angle"], pg["img_dim"],
                         pg["raw_dim"], unpack_ink(pg["ink"]))


def test_sweep_equals_reference_grid_search():
    with open(GOLD, encoding="utf-8") as f:
        gold = json.load(f)
    pages = [fixture_page(pg) for pg in gold["pages"]]
    res = eta.sweep(pages)
    want_iou = np.array([pg["iou"] for pg in gold["pages"]])
    want_area = np.array([pg["area"] for pg in gold["pages"]])
    assert (res.status == 0).all()
    assert res.iou.shape == (3, 729) and res.systems.tolist() == eta.default_grid().tolist()
    assert np.array_equal(res.iou, want_iou)            # bit for bit: 2 x 2 187 means
    assert np.array_equal(res.area, want_area)
    score = [np.mean([want_area[k, s] for k in range(3)]) for s in range(729)]
    assert res.score.tolist() == score
    want_rank = sorted([(tuple(int(v) for v in s), float(x)) for s, x in zip(eta.default_grid(), score)],
                       key=lambda t: t[1])
    assert res.ranking() == want_rank
    assert eta.try_params(res.systems[100].tolist(), pages) == score[100]


def page_size_pages():
    from tools.gen_golden_eval import make_page
    specs = [(9101, 0, (560, 4700), (560, 4700)), (9102, 0.35, (600, 4740), (560, 4700)),
             (9103, -0.4, (580, 4724), (560, 4700))]
    out = []
    for seed, angle, img_dim, raw_dim in specs:
        pg, ink = make_page(seed, angle, img_dim, raw_dim, latsyl, length=1050)
        chars = [CharBox(c, tuple(ul), tuple(lr)) for c, ul, lr in pg["chars"]]
        gt = [{"syl": g["syl"], "difficult": g["difficult"], "ul": tuple(g["box"][:2]), "lr": tuple(g["box"][2:])}
              for g in pg["gt"]]
        out.append(eta.SweepPage(chars, pg["transcript"], gt, angle, img_dim, raw_dim, ink))
    return out


def test_sweep_page_size_against_host_path():
    pages = page_size_pages()
    assert all(1000 <= len(p.transcript) <= 1500 for p in pages)
    res = eta.sweep(pages)
    P, S = 3, 729
    ops = res.batch.results()
    # device boxes of EVERY problem == syllable_boxes_batch + rotate_boxes on the downloaded alignment columns
    preps = [p.prepared() for p in pages]
    prob_page = np.repeat(np.arange(P), S)
    nchar = np.cumsum([0] + [len(q["boxes"]) for q in preps])
    all_boxes = np.concatenate([q["boxes"] for q in preps])
    host = page_batch.syllable_boxes_batch(
        [pages[k].transcript for k in prob_page], [latsyl.syllabify_text(pages[k].transcript) for k in prob_page], ops,
        [np.arange(nchar[k], nchar[k + 1]) for k in prob_page], all_boxes, [pages[k].angle for k in prob_page],
        [pages[k].image_dim for k in prob_page], [pages[k].raw_dim for k in prob_page])
    boxes, present, box_status = (t.cpu().numpy() for t in res.device_boxes)
    assert (box_status == 0).all()
    for p, (which, rot) in enumerate(host):
        assert np.flatnonzero(present[p]).tolist() == which.tolist(), p
        assert np.array_equal(boxes[p][which], rot), p
    # per-(page, system) means == score_alignment on those boxes: every system of page 0, 64 seeded of the others
    rng = np.random.default_rng(77)
    for k in range(P):
        cols = range(S) if k == 0 else sorted(rng.choice(S, size=64, replace=False).tolist())
        names = preps[k]["names"]
        for s in cols:
            which, rot = host[k * S + s]
            syl_boxes = [{"syl": names[w], "ul": tuple(b[:2]), "lr": tuple(b[2:])} for w, b in zip(which, rot)]
            try:
                iou, area = eta.score_alignment(pages[k].gt_boxes, syl_boxes, pages[k].ink)
            except RuntimeError:            # a rectangle outside the page: that (page, system) only is marked
                assert res.status[k, s] == _native.TA_EVAL_OUT_OF_RANGE and np.isnan(res.area[k, s]), (k, s)
                continue
            except ZeroDivisionError:
                assert res.status[k, s] == _native.TA_EVAL_ZERO_AREA and np.isnan(res.area[k, s]), (k, s)
                continue
            assert res.status[k, s] == 0 and res.iou[k, s] == iou and res.area[k, s] == area, (k, s)
    assert (res.status == 0).any() and set(np.unique(res.status)) <= {0, _native.TA_EVAL_OUT_OF_RANGE,
                                                                      _native.TA_EVAL_ZERO_AREA}


def test_summed_area_tables():
    rng = np.random.default_rng(5)
    shapes = [(4400, 1400), (1, 1), (7, 300), (129, 65), (65, 1), (300, 7), (64, 64), (193, 1031)]
    planes = [(rng.random(s) < 0.3).astype(np.uint8) * rng.integers(1, 256, size=s, dtype=np.uint8) for s in shapes]
    inks = [torch.from_numpy(p).cuda() for p in planes]
    sats = [torch.full(p.shape, -7, dtype=torch.int32, device="cuda") for p in planes]
    hh = np.array([s[0] for s in shapes], np.int32)
    ww = np.array([s[1] for s in shapes], np.int32)
    ip = np.array([t.data_ptr() for t in inks], np.uint64)
    sp = np.array([t.data_ptr() for t in sats], np.uint64)
    _native.check(_native.lib.ta_eval_integral(len(shapes), ip.ctypes.data, hh.ctypes.data, ww.ctypes.data,
                                               sp.ctypes.data, torch.cuda.current_stream().cuda_stream), "ta_eval_integral")
    torch.cuda.synchronize()
    for p, t in zip(planes, sats):
        want = np.cumsum(np.cumsum(p != 0, axis=0, dtype=np.int64), axis=1)
        got = t.cpu().numpy()
        assert np.array_equal(got, want), p.shape
        # rectangle counts touching every border
        h, w = p.shape
        for x0, y0, x1, y1 in [(0, 0, w - 1, h - 1), (0, h - 1, w - 1, h - 1), (w - 1, 0, w - 1, h - 1),
                               (0, 0, 0, 0), (w // 2, h // 3, w - 1, h - 1), (0, h // 2, w // 3, h - 1)]:
            S = lambda x, y: 0 if x < 0 or y < 0 else int(got[y, x])        # noqa: E731
            n = S(x1, y1) - S(x0 - 1, y1) - S(x1, y0 - 1) + S(x0 - 1, y0 - 1)
            assert n == int(np.count_nonzero(p[y0:y1 + 1, x0:x1 + 1]))


def tiny_page(text, x0, ink_under, gt):
    chars = [CharBox(c, (x0 + 12 * k, 20), (x0 + 12 * k + 10, 40)) for k, c in enumerate(text)]
    ink = np.zeros((60, 200), dtype=bool)
    for k in ink_under:
        ink[24:36, max(x0 + 12 * k + 2, 0):x0 + 12 * k + 8] = True
    gt = [{"syl": s, "difficult": 0, "ul": ul, "lr": lr} for s, ul, lr in gt]
    return eta.SweepPage(chars, text, gt, 0, (200, 60), (200, 60), ink)


def test_status_paths():
    # blank paper under the 'nus' pair: 0 / 0; a box that starts left of the page; a page that is fine
    blank = tiny_page("dominus", 10, [0, 1, 2, 3], [("do", (10, 20), (32, 40)), ("nus", (58, 20), (92, 40))])
    off = tiny_page("dominus", -20, range(7), [("do", (0, 20), (12, 40)), ("mi", (4, 20), (26, 40))])
    fine = tiny_page("dominus", 10, range(7), [("do", (10, 20), (32, 40)), ("mi", (34, 20), (56, 40))])
    systems = [[8, -4, -7, -7, -3, 0], [5, -10, -2, -2, 0, 0]]
    res = eta.sweep([blank, off, fine], systems)
    assert (res.status[0] == _native.TA_EVAL_ZERO_AREA).all()
    assert (res.status[1] == _native.TA_EVAL_OUT_OF_RANGE).all()
    assert (res.status[2] == 0).all() and np.isfinite(res.area[2]).all() and np.isfinite(res.iou[2]).all()
    assert np.isnan(res.area[:2]).all() and np.isnan(res.iou[:2]).all() and np.isnan(res.score).all()
    # the host path raises for the same inputs
    ops = res.batch.results()
    for k, exc in [(0, ZeroDivisionError), (1, RuntimeError)]:
        pg = [blank, off][k]
        q = pg.prepared()
        which, rot = page_batch.syllable_boxes_batch([pg.transcript], [latsyl.syllabify_text(pg.transcript)],
                                                     [ops[2 * k]], [np.arange(len(q["boxes"]))], q["boxes"], [0],
                                                     [Dim(200, 60)], [Dim(200, 60)])[0]
        syl_boxes = [{"syl": q["names"][w], "ul": tuple(b[:2]), "lr": tuple(b[2:])} for w, b in zip(which, rot)]
        with pytest.raises(exc):
            eta.score_alignment(pg.gt_boxes, syl_boxes, pg.ink)


def test_sweep_page_from_image():
    from text_alignment_amd import textAlignPreprocessing as preproc
    rng = np.random.default_rng(3)
    raw = np.full((400, 360), 235, dtype=np.uint8)
    text = "gloria patri et filio et spiritui sancto"
    chars = []
    for k, c in enumerate(text):
        line, col = divmod(k, 20)
        x, y = 30 + 15 * col, 60 + 80 * line
        chars.append(CharBox(c, (x, y), (x + 12, y + 30)))
        if c != " ":
            raw[y + 4:y + 26, x + 2:x + 10] = rng.integers(0, 60, size=(22, 8), dtype=np.uint8)
    gt = [{"syl": "glo", "difficult": 0, "ul": (30, 60), "lr": (72, 90)},
          {"syl": "pa", "difficult": 0, "ul": (120, 60), "lr": (147, 90)}]
    a = eta.SweepPage.from_image(raw, text, chars, gt)
    image, _, angle = preproc.preprocess_images(raw)
    ev_image, _, _ = preproc.preprocess_images(raw, correct_rotation=False)
    b = eta.SweepPage(chars, text, gt, angle, image.dim, Dim(360, 400), ev_image.ink)
    assert a.angle == b.angle and (a.image_dim.ncols, a.image_dim.nrows) == (b.image_dim.ncols, b.image_dim.nrows)
    systems = eta.default_grid()[::91]
    ra, rb = eta.sweep([a], systems), eta.sweep([b], systems)
    assert np.array_equal(ra.iou, rb.iou, equal_nan=True) and np.array_equal(ra.area, rb.area, equal_nan=True)
    assert np.array_equal(ra.status, rb.status)
    assert np.isfinite(ra.area).any()
