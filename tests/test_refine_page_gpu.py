"""forced.refine_pages(scope="page") end to end on the GPU: four synthetic pages of three short lines and a seeded model.
Every page's result must equal the one built on the host from the run's own harvest table and downloaded probabilities
with the checkers alone -- tests/forced_page_ref.py for windows and path, tests/forced_ref.py for boxes and syllables --
every transcript character must lie in a pair column with a box, the OCR characters must stay what they were, and the
default scope must return what it returns without the new arguments."""
import numpy as np
import pytest

import forced_page_ref as R
import forced_ref as FR
from test_forced_gpu import _line_texts, _model, _second_transcript

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEEDS = (70, 71, 72, 73)
PARAMS = [8, -12, -6, -6, -2, -2]


@pytest.fixture(scope="module")
def run():
    from oracle import ocr_ref_f64 as OR
    from test_page_gpu import _page
    from text_alignment_amd import alignToOCR as atocr, latinSyllabification as latsyl, ocr, page as page_mod
    om = _model(OR)
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    pages = [_page(seed, 3, OR, page_mod)[0] for seed in SEEDS]
    one = atocr.process_batch(pages, ["amen"] * len(pages), rec, PARAMS)
    trs = [_second_transcript(_line_texts(r[3], pg), latsyl)[0] for r, pg in zip(one, pages)]
    idx, arr = [], []
    plain = atocr.process_batch(pages, trs, rec, PARAMS, indices_out=idx, arrays_out=arr)
    return {"om": om, "rec": rec, "pages": pages, "trs": trs, "plain": plain, "idx": idx, "arr": arr}


def test_page_scope_gives_every_character_a_box_and_equals_the_checkers(run):
    from text_alignment_amd import forced, latinSyllabification as latsyl, ocr, page_batch as pb, train
    pages, trs, rec, om = run["pages"], run["trs"], run["rec"], run["om"]
    res = forced.refine_pages(pages, trs, rec, PARAMS, scope="page")
    h = res.harvest
    P = res.probs.cpu().numpy()
    assert len(res) == 4 and len(res.page_scope) == 4
    for p in range(4):
        a, b = int(h.line_first[p]), int(h.line_first[p + 1])
        cs = train.encode_text(om.codec, trs[p])
        n = len(cs)
        # ---- the precondition, from the checker alone: the page is eligible and has a path
        assert b - a == 3 and n >= 1 and min(cs) >= 1 and pb.plain_page(trs[p], latsyl.syllabify_text(trs[p]))
        win = R.page_windows(h.table[a:b, :3], n, 16)
        assert win is not None and n <= int(res.T[a:b].sum())
        Ps = [P[int(res.row_off[q]):int(res.row_off[q]) + int(res.T[q])] for q in range(a, b)]
        st, score, frames, _ = R.align_page(Ps, cs, win[0], win[1])
        assert st == R.OK
        # ---- the kernel's path is the checker's
        assert res.page_scope[p] == 0 and res.page_score[p] == score
        assert np.array_equal(res.windows[p][0], win[0]) and np.array_equal(res.windows[p][1], win[1])
        assert np.array_equal(res.page_frames[p], frames)
        assert res.refined[a:b].all()
        for q in range(a, b):
            assert np.array_equal(res.frames[q], frames[frames[:, 0] == q - a][:, 1:])
        # ---- every transcript character lies in a pair column with a box of its own
        ops, idx, boxes = res.columns[0][p], res.columns[1][p], res.columns[2]
        assert ops.tolist() == [0] * n and len(idx) == n and len(set(idx.tolist())) == n
        cb = []
        for k in range(3):
            s = h.lines[a + k].source
            mine = frames[frames[:, 0] == k]
            cb += FR.peak_boxes(mine[:, 3], int(res.T[a + k]), s.width, s.offset_x, s.offset_y, s.offset_y + s.height, ocr.PAD)
        assert len(cb) == n and [tuple(r) for r in boxes[idx].tolist()] == cb
        # ---- the syllables' boxes: the per-character rule on those boxes (angle 0: no rotation); none is missing
        syls = latsyl.syllabify_text(trs[p])
        named = [s for s in syls if len(s) >= 1]
        first, last = pb.syllable_spans(trs[p], syls)
        want = [FR.syllable_box(cb, int(f), int(l)) for f, l in zip(first, last)]
        assert None not in want and res.indices[p] == list(range(len(want)))
        assert [tuple(r) for r in res.arrays[p].tolist()] == want
        assert [s.char for s in res.results[p][0]] == named
        assert len(run["idx"][p]) <= len(want)
        # ---- the page's OCR characters are what they were
        assert res.results[p][3].chars == run["plain"][p][3].chars
        assert np.array_equal(res.results[p][3].boxes, run["plain"][p][3].boxes)
    # a margin of 0 and process(refine_scope="page"): the same rule, page by page
    from text_alignment_amd import alignToOCR as atocr
    res0 = forced.refine_pages(pages[:2], trs[:2], rec, PARAMS, scope="page", margin=0)
    for p in range(2):
        a, b = int(h.line_first[p]), int(h.line_first[p + 1])
        win = R.page_windows(h.table[a:b, :3], len(trs[p]), 0)
        assert np.array_equal(res0.windows[p][0], win[0]) and np.array_equal(res0.windows[p][1], win[1])
        Ps = [P[int(res.row_off[q]):int(res.row_off[q]) + int(res.T[q])] for q in range(a, b)]
        st, score, frames, _ = R.align_page(Ps, train.encode_text(om.codec, trs[p]), win[0], win[1])
        assert (res0.page_scope[p] == 0) == (st == R.OK) and (res0.page_scope[p] in (0, forced.PAGE_NO_PATH))
        if st == R.OK:
            assert np.array_equal(res0.page_frames[p], frames) and res0.page_score[p] == score
    single = atocr.process(pages[1], trs[1], rec, PARAMS, refine=True, refine_scope="page")
    assert np.array_equal(single[0].boxes, res.results[1][0].boxes) and single[0].chars == res.results[1][0].chars


def test_pages_that_are_not_eligible_come_back_unrefined(run):
    from text_alignment_amd import forced
    pages, trs, rec = run["pages"], run["trs"], run["rec"]
    tr = [trs[0][:4] + "é" + trs[0][4:], trs[1], trs[2][:6] + "." + trs[2][6:]]
    idx, arr = [], []
    from text_alignment_amd import alignToOCR as atocr
    plain = atocr.process_batch(pages[:3], tr, rec, PARAMS, indices_out=idx, arrays_out=arr)
    res = forced.refine_pages(pages[:3], tr, rec, PARAMS, scope="page")
    assert res.page_scope.tolist() == [forced.PAGE_CLASS0, 0, forced.PAGE_NOT_PLAIN] and res.object_pages == [2]
    for p in (0, 2):
        assert res.indices[p] == idx[p] and np.array_equal(res.arrays[p], arr[p]) and res.page_frames[p] is None
        assert [s.char for s in res.results[p][0]] == [s.char for s in plain[p][0]]
        assert not res.refined[3 * p:3 * p + 3].any()
    assert res.refined[3:6].all()
    with pytest.raises(ValueError):
        forced.refine_pages(pages[:1], trs[:1], rec, PARAMS, scope="chunk")
    with pytest.raises(ValueError):
        forced.refine_pages(pages[:1], trs[:1], rec, PARAMS, scope="page", margin=-1)


def test_line_scope_and_the_default_are_what_they_were(run):
    from text_alignment_amd import alignToOCR as atocr, forced
    pages, trs, rec = run["pages"], run["trs"], run["rec"]
    old = forced.refine_pages(pages, trs, rec, PARAMS, (4, 5))
    for new in (forced.refine_pages(pages, trs, rec, PARAMS, (4, 5), scope="line"),
                forced.refine_pages(pages, trs, rec, PARAMS, (4, 5), False, "line", 3)):
        assert new.page_scope is None and np.array_equal(new.refined, old.refined) and new.indices == old.indices
        assert all(np.array_equal(x, y) for x, y in zip(new.arrays, old.arrays))
        assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(new.frames, old.frames))
        assert new.score == old.score
        for p in range(4):
            assert [s.char for s in new.results[p][0]] == [s.char for s in old.results[p][0]]
            assert np.array_equal(new.results[p][0].boxes, old.results[p][0].boxes)
    a = atocr.process(pages[0], trs[0], rec, PARAMS, refine=True, min_agreement=0.8)
    b = atocr.process(pages[0], trs[0], rec, PARAMS, refine=True, min_agreement=0.8, refine_scope="line")
    assert np.array_equal(a[0].boxes, b[0].boxes) and a[0].chars == b[0].chars


def test_process_batch_refuses_page_scope_and_names_refine_pages(run):
    from text_alignment_amd import alignToOCR as atocr
    with pytest.raises(ValueError, match="refine_pages"):
        atocr.process_batch(run["pages"], run["trs"], run["rec"], PARAMS, refine=True, refine_scope="page")
    with pytest.raises(ValueError):
        atocr.process_batch(run["pages"], run["trs"], run["rec"], PARAMS, refine=True, refine_scope="word")
