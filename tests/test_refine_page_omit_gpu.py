"""forced.refine_pages(scope="page", page_omit=...) end to end on the GPU: the four synthetic pages of three lines and the
seeded model of tests/test_refine_page_gpu.py, each page's transcript holding the three inserted letters of
tests/test_refine_omit_gpu.py.  With page_omit at 4 bits every refined page's frames, score and omitted count must equal
the checker tests/forced_page_omit_ref.py on the run's own downloaded probabilities and harvest table, its columns and
syllable boxes what forced.page_columns' rule and the per-character rule build from them; every present transcript
character sits in a pair column with a box, every omitted one in a column without; the OCR characters stay what they
were.  page_omit=None is scope="page" as it was, and the refusals raise."""
import numpy as np
import pytest

import forced_page_omit_ref as R
import forced_page_ref as PR
import forced_ref as FR
from test_forced_gpu import _line_texts, _model, _second_transcript

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEEDS = (70, 71, 72, 73)
PARAMS = [8, -12, -6, -6, -2, -2]
OMIT = 4.0                  # bits, as tests/test_refine_omit_gpu.py argues for


@pytest.fixture(scope="module")
def run():
    from oracle import ocr_ref_f64 as OR
    from test_page_gpu import _page
    from text_alignment_amd import alignToOCR as atocr, forced, latinSyllabification as latsyl, ocr, page as page_mod
    om = _model(OR)
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    pages = [_page(seed, 3, OR, page_mod)[0] for seed in SEEDS]
    one = atocr.process_batch(pages, ["amen"] * len(pages), rec, PARAMS)
    built = [_second_transcript(_line_texts(r[3], pg), latsyl) for r, pg in zip(one, pages)]
    word = [b[1] for b in built]
    trs = [b[0][:hi + 1] + b[0][hi + 2:] for b, (lo, hi) in zip(built, word)]      # three letters the longest line lacks
    plain = atocr.process_batch(pages, trs, rec, PARAMS)
    res = forced.refine_pages(pages, trs, rec, PARAMS, scope="page", page_omit=OMIT)
    return {"om": om, "rec": rec, "pages": pages, "trs": trs, "word": word, "plain": plain, "res": res}


def test_with_page_omit_frames_columns_and_boxes_equal_the_checkers(run):
    from text_alignment_amd import forced, latinSyllabification as latsyl, ocr, page_batch as pb, train
    res, om, trs = run["res"], run["om"], run["trs"]
    h = res.harvest
    P = res.probs.cpu().numpy()
    omit_q = forced.omit_units(OMIT)
    assert len(res) == 4 and len(res.page_scope) == 4 and res.object_pages == []
    total_gone = 0
    for p in range(4):
        a, b = int(h.line_first[p]), int(h.line_first[p + 1])
        cs = train.encode_text(om.codec, trs[p])
        n = len(cs)
        # ---- the precondition, from the checker alone: the page is eligible
        assert b - a == 3 and n >= 1 and min(cs) >= 1 and pb.plain_page(trs[p], latsyl.syllabify_text(trs[p]))
        win = PR.page_windows(h.table[a:b, :3], n, 16)
        assert win is not None
        Ps = [P[int(res.row_off[q]):int(res.row_off[q]) + int(res.T[q])] for q in range(a, b)]
        st, score, frames = R.answer(Ps, cs, win[0], win[1], omit_q)
        assert st == R.OK
        gone = frames[:, 0] == R.OMITTED
        print("page %d: %d characters, %d omitted: %r" % (p, n, int(gone.sum()), "".join(np.asarray(list(trs[p]))[gone])))
        assert (~gone).any()
        # ---- the kernel's path is the checker's
        assert res.page_scope[p] == 0 and res.page_score[p] == score
        assert np.array_equal(res.windows[p][0], win[0]) and np.array_equal(res.windows[p][1], win[1])
        assert np.array_equal(res.page_frames[p], frames) and res.page_omitted[p] == int(gone.sum())
        assert res.refined[a:b].all()
        for q in range(a, b):
            assert np.array_equal(res.frames[q], frames[frames[:, 0] == q - a][:, 1:])
        total_gone += int(gone.sum())
        # ---- a present character lies in a pair column with a box of its own, an omitted one in a column without
        ops, idx, boxes = res.columns[0][p], res.columns[1][p], res.columns[2]
        assert ops.tolist() == np.where(gone, 1, 0).tolist()
        assert len(idx) == int((~gone).sum()) and len(set(idx.tolist())) == len(idx)
        new = []
        for k in range(3):
            s = h.lines[a + k].source
            mine = frames[frames[:, 0] == k]
            new += FR.peak_boxes(mine[:, 3], int(res.T[a + k]), s.width, s.offset_x, s.offset_y, s.offset_y + s.height, ocr.PAD)
        assert [tuple(r) for r in boxes[idx].tolist()] == new
        it = iter(new)
        cb = [None if g else next(it) for g in gone]
        # ---- the syllables' boxes: the per-character rule on those boxes; a syllable all of whose characters are omitted
        # has none
        syls = latsyl.syllabify_text(trs[p])
        named = [s for s in syls if len(s) >= 1]
        first, last = pb.syllable_spans(trs[p], syls)
        want = {k: FR.syllable_box(cb, int(f), int(l)) for k, (f, l) in enumerate(zip(first, last))}
        have = {k: bx for k, bx in want.items() if bx is not None}
        assert res.indices[p] == sorted(have)
        assert [tuple(r) for r in res.arrays[p].tolist()] == [have[k] for k in sorted(have)]
        assert [s.char for s in res.results[p][0]] == [named[k] for k in sorted(have)]
        # ---- the page's OCR characters are what they were
        assert res.results[p][3].chars == run["plain"][p][3].chars
        assert np.array_equal(res.results[p][3].boxes, run["plain"][p][3].boxes)
    assert total_gone > 0


def test_page_omit_none_is_page_scope_as_it_was(run):
    from text_alignment_amd import forced
    pages, trs, rec = run["pages"], run["trs"], run["rec"]
    old = forced.refine_pages(pages, trs, rec, PARAMS, scope="page")
    new = forced.refine_pages(pages, trs, rec, PARAMS, scope="page", page_omit=None)
    assert new.page_omitted is None and old.page_omitted is None
    assert np.array_equal(new.page_scope, old.page_scope) and np.array_equal(new.refined, old.refined)
    assert new.indices == old.indices and new.page_score == old.page_score and new.score == old.score
    same = lambda x, y: (x is None and y is None) or np.array_equal(x, y)                          # noqa: E731
    assert all(same(x, y) for x, y in zip(new.arrays, old.arrays))
    assert all(same(x, y) for x, y in zip(new.frames, old.frames))
    assert all(same(x, y) for x, y in zip(new.page_frames, old.page_frames))
    assert all((x is None and y is None) or (same(x[0], y[0]) and same(x[1], y[1])) for x, y in zip(new.windows, old.windows))
    for a, b in zip(new.columns[:2], old.columns[:2]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(new.columns[2], old.columns[2])
    for p in range(4):
        assert [s.char for s in new.results[p][0]] == [s.char for s in old.results[p][0]]
        assert np.array_equal(new.results[p][0].boxes, old.results[p][0].boxes)


def test_process_passes_page_omit_through(run):
    from text_alignment_amd import alignToOCR as atocr
    pages, trs, rec, res = run["pages"], run["trs"], run["rec"], run["res"]
    single = atocr.process(pages[1], trs[1], rec, PARAMS, refine=True, refine_scope="page", page_omit=OMIT)
    assert np.array_equal(single[0].boxes, res.results[1][0].boxes) and single[0].chars == res.results[1][0].chars


def test_a_page_with_more_characters_than_frames_is_refined(run):
    """the strict page lattice refuses such a page (PAGE_FRAMES); with page_omit it has a path, equal to the checker's"""
    from text_alignment_amd import forced, train
    pages, trs, rec, om = run["pages"], run["trs"], run["rec"], run["om"]
    frames_all = int(run["res"].T[:3].sum())
    long_tr = " ".join([trs[0]] * (frames_all // len(trs[0]) + 2))
    assert frames_all < len(long_tr) <= forced.MAX_TARGET         # one window can hold the whole text
    strict = forced.refine_pages(pages[:1], [long_tr], rec, PARAMS, scope="page", margin=1000)
    res = forced.refine_pages(pages[:1], [long_tr], rec, PARAMS, scope="page", margin=1000, page_omit=OMIT)
    assert strict.page_scope[0] == forced.PAGE_FRAMES and res.page_scope[0] == 0
    h, P = res.harvest, res.probs.cpu().numpy()
    Ps = [P[int(res.row_off[q]):int(res.row_off[q]) + int(res.T[q])] for q in range(3)]
    cs = train.encode_text(om.codec, long_tr)
    st, score, frames = R.answer(Ps, cs, res.windows[0][0], res.windows[0][1], forced.omit_units(OMIT))
    assert np.array_equal(res.page_frames[0], frames) and res.page_score[0] == score
    assert res.page_omitted[0] >= len(long_tr) - frames_all


def test_the_new_refusals_raise_and_the_pinned_ones_still_do(run):
    from text_alignment_amd import alignToOCR as atocr, forced
    pages, trs, rec = run["pages"][:1], run["trs"][:1], run["rec"]
    for kw in (dict(scope="line", page_omit=OMIT), dict(page_omit=OMIT), dict(scope="page", page_omit=OMIT, confidence=True),
               dict(scope="page", page_omit=OMIT, posterior=True), dict(scope="page", page_omit=-0.5),
               dict(scope="page", page_omit=1024.5), dict(scope="page", page_omit="4"), dict(scope="page", page_omit=True)):
        with pytest.raises(ValueError):
            forced.refine_pages(pages, trs, rec, PARAMS, **kw)
    with pytest.raises(ValueError):
        atocr.process(pages[0], trs[0], rec, PARAMS, refine=False, page_omit=OMIT)
    with pytest.raises(ValueError):
        atocr.process(pages[0], trs[0], rec, PARAMS, refine=True, page_omit=OMIT)                   # line scope
    # pinned: omit at page scope names page_omit now; process_batch knows neither omit nor page scope
    with pytest.raises(ValueError, match="page scope has no omission") as e:
        forced.refine_pages(pages, trs, rec, PARAMS, scope="page", omit=OMIT)
    assert "page_omit" in str(e.value)
    with pytest.raises(TypeError):
        atocr.process_batch(pages, trs, rec, PARAMS, refine=True, omit=OMIT)
    with pytest.raises(TypeError):
        atocr.process_batch(pages, trs, rec, PARAMS, refine=True, page_omit=OMIT)
    with pytest.raises(ValueError):
        atocr.process_batch(pages, trs, rec, PARAMS, refine=True, refine_scope="page")
