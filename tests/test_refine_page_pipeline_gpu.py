"""process_batch(..., refine=True, refine_scope="page", page_margin=M): page scope inside the three-stage pipeline
 against forced.refine_pages(scope="page", margin=M) page by page.  Seven pages -- the four
three-line pages of seeds 70 - 73 that tests/test_refine_page_gpu.py pins as eligible with a path at margin 16, and three
fresh page objects of seeds 70, 72, 71, the first with a character outside the codec in its transcript, the second with one
that takes the syllables off the array path, the third unchanged -- interleaved, so that refined and unrefined pages share
chunks; PIPELINE_CHUNK_PAGES patched to 2 runs the lead chunk, the steady loop and the drain."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PARAMS = [8, -12, -6, -6, -2, -2]
ORDER = (("old", 70), ("new", 70), ("old", 71), ("new", 72), ("old", 72), ("new", 71), ("old", 73))
EDITED = {1: "PAGE_CLASS0", 3: "PAGE_NOT_PLAIN"}          # page -> the reason its edit gives it


@pytest.fixture(scope="module")
def book():
    """the seven pages, their transcripts, and refine_pages(scope="page") on every page alone -- computed once"""
    from oracle import ocr_ref_f64 as OR
    from test_forced_gpu import _line_texts, _model, _second_transcript
    from test_page_gpu import _page
    from text_alignment_amd import alignToOCR as atocr, forced, latinSyllabification as latsyl, ocr, page as page_mod
    om = _model(OR)
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    pages = [_page(seed, 3, OR, page_mod)[0] for _, seed in ORDER]
    assert len({id(pg) for pg in pages}) == 7
    one = atocr.process_batch(pages, ["amen"] * 7, rec, PARAMS)
    trs = [_second_transcript(_line_texts(r[3], pg), latsyl)[0] for r, pg in zip(one, pages)]
    trs[1] = trs[1][:4] + "é" + trs[1][4:]
    trs[3] = trs[3][:6] + "." + trs[3][6:]
    alone = [forced.refine_pages([pg], [tr], rec, PARAMS, scope="page", margin=16) for pg, tr in zip(pages, trs)]
    return dict(om=om, rec=rec, params=PARAMS, pages=pages, trs=trs, alone=alone)


def _boxes(seq):
    """a page's syllable boxes as rows: the array path's sequence holds them, the object path's list is CharBox objects"""
    if hasattr(seq, "boxes"):
        return np.asarray(seq.boxes, dtype=np.int64).reshape(-1, 4).tolist()
    return [[b.ulx, b.uly, b.lrx, b.lry] for b in seq]


def _same(a, b):
    """two process_batch results (results, indices, arrays), byte for byte"""
    (ra, ia, aa), (rb, ib, ab) = a, b
    assert len(ra) == len(rb) and ia == ib
    for p in range(len(ra)):
        assert np.array_equal(aa[p], ab[p]) and aa[p].dtype == ab[p].dtype
        assert [s.char for s in ra[p][0]] == [s.char for s in rb[p][0]] and _boxes(ra[p][0]) == _boxes(rb[p][0])
        assert ra[p][3].chars == rb[p][3].chars and np.array_equal(ra[p][3].boxes, rb[p][3].boxes)
        assert np.array_equal(np.asarray(ra[p][2]), np.asarray(rb[p][2]))


def _run(book, monkeypatch, chunk=2, **kw):
    from text_alignment_amd import alignToOCR as atocr
    monkeypatch.setattr(atocr, "PIPELINE_CHUNK_PAGES", chunk)
    idx, arr = [], []
    res = atocr.process_batch(kw.pop("pages", book["pages"]), kw.pop("trs", book["trs"]), kw.pop("rec", book["rec"]),
                              book["params"], indices_out=idx, arrays_out=arr, **kw)
    return res, idx, arr


def _page_run(book, monkeypatch, margin=16, **kw):
    refined, scope = [], []
    got = _run(book, monkeypatch, refine=True, refine_scope="page", page_margin=margin, refined_out=refined,
               page_scope_out=scope, **kw)
    return got, refined, scope


def _equals_alone(got, refined, scope, alone, pages=None):
    """per page every output of the pipeline against refine_pages(scope="page") on that page alone"""
    from text_alignment_amd import forced
    assert len(refined) == len(scope) == len(alone) == len(got[0])
    for p, a in enumerate(alone):
        assert got[1][p] == a.indices[0] and np.array_equal(got[2][p], a.arrays[0]) and got[2][p].dtype == a.arrays[0].dtype, p
        assert [s.char for s in got[0][p][0]] == [s.char for s in a.results[0][0]], p
        assert _boxes(got[0][p][0]) == _boxes(a.results[0][0]), p
        assert refined[p].dtype == bool and refined[p].tolist() == np.asarray(a.refined, dtype=bool).tolist(), p
        s = scope[p]
        assert isinstance(s, forced.PageScope) and s.reason == int(a.page_scope[0]), (p, s.reason, int(a.page_scope[0]))
        for mine, theirs in ((s.windows, a.windows[0]), (s.frames, a.page_frames[0])):
            assert (mine is None) == (theirs is None), p
        if s.windows is not None:
            assert np.array_equal(s.windows[0], a.windows[0][0]) and np.array_equal(s.windows[1], a.windows[0][1]), p
            assert s.windows[0].dtype == np.int32 and s.windows[1].dtype == np.int32
        if s.frames is not None:
            assert np.array_equal(s.frames, a.page_frames[0]) and s.frames.shape == (len(a.page_frames[0]), 4), p
        assert s.score == a.page_score[0], p
        assert (s.windows is not None) == (s.reason in (0, forced.PAGE_NO_PATH)) and (s.frames is not None) == (s.reason == 0)


def test_the_precondition_from_the_reference_call_alone(book):
    from text_alignment_amd import forced
    alone = book["alone"]
    reasons = [int(a.page_scope[0]) for a in alone]
    assert sum(r == 0 for r in reasons) >= 5
    for p, name in EDITED.items():
        assert reasons[p] == getattr(forced, name) and not np.asarray(alone[p].refined).any()
    for p in (0, 2, 4, 6):                               # the four pages tests/test_refine_page_gpu.py pins
        assert reasons[p] == 0 and np.asarray(alone[p].refined).all() and len(alone[p].refined) == 3


def test_the_pipeline_refines_at_page_scope_as_refine_pages_does_page_by_page(book, monkeypatch):
    from text_alignment_amd import alignToOCR as atocr
    assert len(atocr.plan_chunks([(None, list(range(7)))], 2, (1,))) == 4      # a lead chunk of one page, then three of two
    plain = _run(book, monkeypatch)
    got, refined, scope = _page_run(book, monkeypatch)
    _equals_alone(got, refined, scope, book["alone"])
    for p in range(7):                                   # the page's OCR characters are what they were without the switch
        assert got[0][p][3].chars == plain[0][p][3].chars and np.array_equal(got[0][p][3].boxes, plain[0][p][3].boxes)
        if p in EDITED:                                  # an unrefined page is the call without refinement
            assert got[1][p] == plain[1][p] and np.array_equal(got[2][p], plain[2][p])
    assert any(not np.array_equal(got[2][p], plain[2][p]) for p in range(7))
    again, refined2, scope2 = _page_run(book, monkeypatch)                      # a second call: the same bytes
    _same(got, again)
    _equals_alone(again, refined2, scope2, book["alone"])
    whole, refined3, scope3 = _page_run(book, monkeypatch, chunk=16)            # one chunk for all pages
    _same(got, whole)
    _equals_alone(whole, refined3, scope3, book["alone"])


def test_a_margin_of_zero_on_the_first_two_pages(book, monkeypatch):
    from text_alignment_amd import forced
    pages, trs = [book["pages"][0], book["pages"][2]], [book["trs"][0], book["trs"][2]]
    alone0 = [forced.refine_pages([pg], [tr], book["rec"], PARAMS, scope="page", margin=0) for pg, tr in zip(pages, trs)]
    assert all(int(a.page_scope[0]) in (0, forced.PAGE_NO_PATH) for a in alone0)
    got, refined, scope = _page_run(book, monkeypatch, margin=0, pages=pages, trs=trs)
    _equals_alone(got, refined, scope, alone0)


def test_the_host_path_is_not_what_ran(book, monkeypatch):
    from text_alignment_amd import forced
    for name in ("page_windows", "page_scope_eligibility", "forced_page_alignment"):
        monkeypatch.setattr(forced, name, lambda *a, _n=name, **k: pytest.fail("forced.%s ran inside the pipeline" % _n))
    got, refined, scope = _page_run(book, monkeypatch)
    _equals_alone(got, refined, scope, book["alone"])


def test_page_scope_without_page_margin_still_raises_and_names_refine_pages(book, monkeypatch):
    from text_alignment_amd import alignToOCR as atocr
    monkeypatch.setattr(atocr.PageChunk, "launch", lambda *a, **k: pytest.fail("GPU work before the refusal"))
    with pytest.raises(ValueError, match="refine_pages"):
        atocr.process_batch(book["pages"], book["trs"], book["rec"], PARAMS, refine=True, refine_scope="page")


def test_line_scope_and_no_refinement_are_the_calls_without_the_new_keywords(book, monkeypatch):
    refined, scope = [], []
    _same(_run(book, monkeypatch), _run(book, monkeypatch, refine=False, page_scope_out=scope))
    line = _run(book, monkeypatch, refine=True, min_agreement=(4, 5))
    _same(line, _run(book, monkeypatch, refine=True, min_agreement=(4, 5), refine_scope="line", page_margin=None,
                     refined_out=refined, page_scope_out=scope))
    assert scope == [] and len(refined) == 7


def test_locate_on_padded_transcripts(book, monkeypatch):
    """every page's transcript with words around it: the spans are found first, page scope runs on them; against
    refine_pages(locate=True, scope="page") on every page alone"""
    from text_alignment_amd import forced
    padded = ["domine deus " + tr + " et in terra" for tr in book["trs"]]
    alone = [forced.refine_pages([pg], [tr], book["rec"], PARAMS, locate=True, scope="page", margin=16)
             for pg, tr in zip(book["pages"], padded)]
    spans = []
    got, refined, scope = _page_run(book, monkeypatch, trs=padded, locate=True, spans_out=spans)
    assert spans == [a.spans[0] for a in alone]
    _equals_alone(got, refined, scope, alone)
    assert sum(s.reason == 0 for s in scope) >= 4


def test_a_list_of_two_models(book, monkeypatch):
    from text_alignment_amd import ocr
    om = book["om"]
    other = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    recs = [book["rec"] if p % 3 else other for p in range(7)]
    got, refined, scope = _page_run(book, monkeypatch, rec=recs)
    _equals_alone(got, refined, scope, book["alone"])
