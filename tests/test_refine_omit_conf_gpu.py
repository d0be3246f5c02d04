"""forced.refine_pages(omit=..., omit_confidence=True) and alignToOCR.process with it, end to end on the GPU: the four
synthetic pages, the seeded model and the transcripts with three extra letters of tests/test_refine_omit_gpu.py.  With the
switch off the result is the call's without it, field for field; with it on frames, scores and boxes are unchanged, the
per-line values equal the checker tests/forced_omit_conf_ref.py on the run's own downloaded probabilities, the
per-character and per-syllable restatements agree with them, and the refusals raise."""
import numpy as np
import pytest

import forced_omit_conf_ref as R
from test_forced_gpu import _line_texts, _model, _second_transcript
from test_refine_omit_gpu import AGREE, OMIT, PARAMS, SEEDS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


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
    trs = [b[0][:hi + 1] + b[0][hi + 2:] for b, (lo, hi) in zip(built, [b[1] for b in built])]      # test_refine_omit_gpu's
    return {"om": om, "rec": rec, "pages": pages, "trs": trs,
            "off": forced.refine_pages(pages, trs, rec, PARAMS, AGREE, omit=OMIT),
            "on": forced.refine_pages(pages, trs, rec, PARAMS, AGREE, omit=OMIT, omit_confidence=True)}


def _same_refinement(new, old):
    assert new.page_scope is None and np.array_equal(new.refined, old.refined) and new.indices == old.indices
    assert all(np.array_equal(x, y) for x, y in zip(new.arrays, old.arrays))
    assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(new.frames, old.frames))
    assert new.score == old.score and new.omitted == old.omitted and new.object_pages == old.object_pages
    for a, b in zip(new.columns[:2], old.columns[:2]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(new.columns[2], old.columns[2])
    for p in range(len(new)):
        assert [s.char for s in new.results[p][0]] == [s.char for s in old.results[p][0]]
        assert np.array_equal(new.results[p][0].boxes, old.results[p][0].boxes)


def test_switch_off_is_the_call_without_it(run):
    from text_alignment_amd import forced
    off = forced.refine_pages(run["pages"], run["trs"], run["rec"], PARAMS, AGREE, omit=OMIT, omit_confidence=False)
    _same_refinement(off, run["off"])
    for res in (off, run["off"]):
        assert res.confidence is None and res.rival is None and res.char_confidence is None and res.syllable_confidence is None


def test_switch_on_values_equal_the_checker_and_nothing_else_moves(run):
    from text_alignment_amd import forced, latinSyllabification as latsyl, page_batch as pb, train
    res, om, trs = run["on"], run["om"], run["trs"]
    _same_refinement(res, run["off"])
    h = res.harvest
    P = res.probs.cpu().numpy()
    omit_q = forced.omit_units(OMIT)
    n_gone = n_shown = 0
    for p in range(4):
        char = np.full(len(trs[p]), forced.NO_CONFIDENCE, dtype=np.int64)
        shown = np.zeros(len(trs[p]), dtype=bool)
        for q in range(int(h.line_first[p]), int(h.line_first[p + 1])):
            if res.frames[q] is None:
                assert res.confidence[q] is None and res.rival[q] is None
                continue
            Pq = P[int(res.row_off[q]):int(res.row_off[q]) + int(res.T[q])]
            G = R.tables_closed(Pq, train.encode_text(om.codec, h.lines[q].text), omit_q)[2]
            value, rival = R.line_values(G, res.frames[q])
            assert res.confidence[q].dtype == np.int64 and res.rival[q].dtype == np.int32
            assert np.array_equal(res.confidence[q], value) and np.array_equal(res.rival[q], rival)
            here = res.frames[q][:, 0] >= 0
            assert (value[here] >= 0).all() and (value[~here] <= 0).all()
            for i in np.flatnonzero(here):                       # a present character's own term is the line's score
                assert R.query(G, i, res.frames[q][i, 2])[2] == res.score[q]
            for i in np.flatnonzero(~here):                      # minus the value bounds the exact margin from above
                assert -value[i] >= R.exact_margin(G, res.score[q], i)
            n_gone += int((~here).sum())
            n_shown += int(here.sum())
            if res.refined[q]:
                a = int(h.table[q][1])
                char[a:a + len(value)] = value
                shown[a:a + len(value)] = here
        # ---- the restatements: per transcript character, and per syllable the smallest value of its PRESENT characters
        assert np.array_equal(res.char_confidence[p], char)
        first, last = pb.syllable_spans(trs[p], latsyl.syllabify_text(trs[p]))
        want = []
        for k in res.indices[p]:
            mine = char[int(first[k]):int(last[k]) + 1][shown[int(first[k]):int(last[k]) + 1]]
            want.append(int(mine.min()) if len(mine) else None)
        assert res.syllable_confidence[p] == want
        assert all(v is None or v >= 0 for v in want)
    assert n_gone > 0 and n_shown > 0


def test_process_hands_the_page_over_and_the_refusals_raise(run):
    from text_alignment_amd import alignToOCR as atocr, forced
    pages, trs, rec, res = run["pages"], run["trs"], run["rec"], run["on"]
    out = []
    single = atocr.process(pages[1], trs[1], rec, PARAMS, refine=True, min_agreement=AGREE, omit=OMIT, omit_confidence=True,
                           confidence_out=out)
    assert np.array_equal(single[0].boxes, res.results[1][0].boxes) and single[0].chars == res.results[1][0].chars
    assert len(out) == 1 and isinstance(out[0], forced.PageConfidence)
    a, b = int(res.harvest.line_first[1]), int(res.harvest.line_first[2])
    assert np.array_equal(out[0].char_confidence, res.char_confidence[1])
    assert out[0].syllable_confidence == res.syllable_confidence[1]
    for x, y in zip(out[0].confidence + out[0].rival, res.confidence[a:b] + res.rival[a:b]):
        assert (x is None and y is None) or np.array_equal(x, y)
    quiet = []
    atocr.process(pages[1], trs[1], rec, PARAMS, refine=True, min_agreement=AGREE, omit=OMIT, confidence_out=quiet)
    assert quiet == []
    for over in (dict(omit_confidence=True), dict(scope="page", omit_confidence=True), dict(omit=OMIT, omit_confidence=1),
                 dict(scope="page", page_omit=OMIT, omit_confidence=True), dict(omit=OMIT, confidence=True)):
        with pytest.raises(ValueError):
            forced.refine_pages(pages[:1], trs[:1], rec, PARAMS, AGREE, **over)
    with pytest.raises(ValueError):
        atocr.process(pages[1], trs[1], rec, PARAMS, refine=False, omit_confidence=True)
    with pytest.raises(ValueError):
        atocr.process(pages[1], trs[1], rec, PARAMS, refine=True, omit_confidence=True)
    with pytest.raises(TypeError):
        atocr.process_batch(pages[:1], trs[:1], rec, PARAMS, refine=True, line_omit=OMIT, omit_confidence=True)
