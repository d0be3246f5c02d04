"""process_batch(..., refine=True): the refinement inside the three-stage pipeline against forced.refine_pages page by
page -- the lead chunk, the steady loop and the drain all run (PIPELINE_CHUNK_PAGES patched to 2, seven pages)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEEDS = (70, 71, 72, 73, 74, 75, 78)                     # page k has 3 + k % 2 lines


@pytest.fixture(scope="module")
def book():
    """the seven pages, their second-pass transcripts, and refine_pages on every page alone -- computed once"""
    from oracle import ocr_ref_f64 as OR
    from test_forced_gpu import _line_texts, _model, _second_transcript
    from test_page_gpu import _page
    from text_alignment_amd import alignToOCR as atocr, forced, latinSyllabification as latsyl, ocr, page as page_mod
    om = _model(OR)
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    params = [8, -12, -6, -6, -2, -2]
    pages = [_page(seed, 3 + k % 2, OR, page_mod)[0] for k, seed in enumerate(SEEDS)]
    one = atocr.process_batch(pages, ["amen"] * len(pages), rec, params)
    trs = [_second_transcript(_line_texts(r[3], pg), latsyl)[0] for r, pg in zip(one, pages)]
    alone = [forced.refine_pages([pg], [tr], rec, params, min_agreement=(4, 5)) for pg, tr in zip(pages, trs)]
    return dict(om=om, rec=rec, params=params, pages=pages, trs=trs, alone=alone)


def _run(book, monkeypatch, chunk=2, **kw):
    from text_alignment_amd import alignToOCR as atocr
    monkeypatch.setattr(atocr, "PIPELINE_CHUNK_PAGES", chunk)
    idx, arr = [], []
    res = atocr.process_batch(kw.pop("pages", book["pages"]), kw.pop("trs", book["trs"]), kw.pop("rec", book["rec"]),
                              book["params"], indices_out=idx, arrays_out=arr, **kw)
    return res, idx, arr


def _same(a, b):
    """two process_batch results (results, indices, arrays), byte for byte"""
    (ra, ia, aa), (rb, ib, ab) = a, b
    assert len(ra) == len(rb) and ia == ib
    for p in range(len(ra)):
        assert np.array_equal(aa[p], ab[p]) and aa[p].dtype == ab[p].dtype
        assert [s.char for s in ra[p][0]] == [s.char for s in rb[p][0]]
        assert np.array_equal(ra[p][0].boxes, rb[p][0].boxes)
        assert ra[p][3].chars == rb[p][3].chars and np.array_equal(ra[p][3].boxes, rb[p][3].boxes)
        assert np.array_equal(np.asarray(ra[p][2]), np.asarray(rb[p][2]))


def test_the_pipeline_refines_as_refine_pages_does_page_by_page(book, monkeypatch):
    """With the float64 restatement of the recogniser, the C aligner and tests/harvest_ref.py alone (min_agreement 4/5)
    the pages of seeds 70, 71, 72, 73, 74, 75 have all of their 3, 4, 3, 4, 3, 4 lines accepted and the page of seed 78
    two of its three (its first line is LOW): 23 of 24 lines, no page without one."""
    from text_alignment_amd import alignToOCR as atocr
    alone = book["alone"]
    lines = [np.asarray(a.refined, dtype=bool) for a in alone]
    assert sum(int(r.sum()) for r in lines) * 2 >= sum(len(r) for r in lines) and all(r.any() for r in lines)
    assert all(a.object_pages == [] for a in alone)
    plain = _run(book, monkeypatch)
    assert len(atocr.plan_chunks([(None, list(range(7)))], 2, (1,))) == 4      # a lead chunk of one page, then three of two
    refined = []
    got = _run(book, monkeypatch, refine=True, min_agreement=(4, 5), refined_out=refined)
    assert len(refined) == 7
    for p, a in enumerate(alone):
        assert refined[p].dtype == bool and refined[p].tolist() == lines[p].tolist()
        assert got[1][p] == a.indices[0] and np.array_equal(got[2][p], a.arrays[0])
        assert [s.char for s in got[0][p][0]] == [s.char for s in a.results[0][0]]
        assert np.array_equal(got[0][p][0].boxes, a.results[0][0].boxes)
        # the page's OCR characters are what they were without the switch
        assert got[0][p][3].chars == plain[0][p][3].chars and np.array_equal(got[0][p][3].boxes, plain[0][p][3].boxes)
    assert any(not np.array_equal(got[2][p], plain[2][p]) for p in range(7))   # and refinement changed boxes
    _same(got, _run(book, monkeypatch, refine=True, min_agreement=(4, 5)))      # a second call: the same bytes
    # one chunk for all pages: the branch without the pipeline takes the same methods
    _same(got, _run(book, monkeypatch, chunk=16, refine=True, min_agreement=(4, 5)))


def test_refine_false_is_the_call_without_the_argument(book, monkeypatch):
    refined = []
    _same(_run(book, monkeypatch), _run(book, monkeypatch, refine=False, refined_out=refined))
    assert refined == []


def test_full_agreement_on_substituted_transcripts_refines_nothing(book, monkeypatch):
    """one substituted character per line and min_agreement 1/1: no line is accepted, the result is refine=False's"""
    trs = []
    for a, tr in zip(book["alone"], book["trs"]):
        for r in a.harvest.table:
            at = int(r[1]) + int(r[2]) // 2
            while tr[at] == " ":
                at += 1
            tr = tr[:at] + ("x" if tr[at] != "x" else "y") + tr[at + 1:]
        trs.append(tr)
    refined = []
    got = _run(book, monkeypatch, trs=trs, refine=True, min_agreement=(1, 1), refined_out=refined)
    assert not any(r.any() for r in refined) and [len(r) for r in refined] == [3 + k % 2 for k in range(7)]
    _same(got, _run(book, monkeypatch, trs=trs))


def test_refusals_up_front(book, monkeypatch):
    from text_alignment_amd import alignToOCR as atocr, ocr
    pages, trs, rec = book["pages"], book["trs"], book["rec"]
    monkeypatch.setattr(atocr.PageChunk, "launch", lambda *a, **k: pytest.fail("GPU work before the refusal"))
    with pytest.raises(ValueError):
        atocr.process_batch(pages, trs, rec, [8.5, -12, -6, -6, -2, -2], refine=True)
    with pytest.raises(ValueError):
        atocr.process_batch(pages, trs, rec, [lambda a, b: 1, -6, -6, -2, -2], refine=True)
    for bad in (0, 1.5, (5, 4), "much", (1, 10 ** 7)):
        with pytest.raises(ValueError):
            atocr.process_batch(pages, trs, rec, book["params"], refine=True, min_agreement=bad)
    om = book["om"]
    codec = list(om.codec)
    codec[5] = "ab"                                       # a codec with a multi-character entry
    with pytest.raises(ValueError):
        atocr.process_batch(pages, trs, ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, codec)), book["params"],
                            refine=True)


def test_locate_on_padded_transcripts(book, monkeypatch):
    """every page's transcript with its neighbours' around it: the spans are found first, the refinement runs on them"""
    trs = book["trs"]
    padded = [" ".join(([trs[p - 1]] if p else []) + [trs[p]] + ([trs[p + 1]] if p + 1 < len(trs) else [])) for p in range(7)]
    spans, refined = [], []
    got = _run(book, monkeypatch, trs=padded, locate=True, spans_out=spans, refine=True, min_agreement=(4, 5),
               refined_out=refined)
    assert [padded[p][a:b] for p, (a, b) in enumerate(spans)] == trs
    want = _run(book, monkeypatch, refine=True, min_agreement=(4, 5))
    _same(got, want)
    assert [r.tolist() for r in refined] == [np.asarray(a.refined, dtype=bool).tolist() for a in book["alone"]]


def test_a_list_of_two_models(book, monkeypatch):
    """pages dealt to two recognisers (the same weights, two objects): every chunk has one, the pipeline runs across"""
    from text_alignment_amd import ocr
    om = book["om"]
    other = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    recs = [book["rec"] if p % 3 else other for p in range(7)]
    refined = []
    got = _run(book, monkeypatch, rec=recs, refine=True, min_agreement=(4, 5), refined_out=refined)
    _same(got, _run(book, monkeypatch, refine=True, min_agreement=(4, 5)))
    assert [r.tolist() for r in refined] == [np.asarray(a.refined, dtype=bool).tolist() for a in book["alone"]]
