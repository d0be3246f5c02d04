"""alignToOCR.locate_book / process_book: the pages of a book, in reading order, against ONE transcript string in which a
page's text occurs twice.  The synthetic pages and the seeded model of tests/test_refine_pipeline_gpu.py; the book is
the pages' second-pass transcripts joined, with page 4's transcript a second time at the front."""
import numpy as np
import pytest

from test_refine_pipeline_gpu import _same, book          # noqa: F401  (that module's fixture: pages, model, transcripts)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

REPEATED = 4


@pytest.fixture(scope="module")
def volume(book):
    trs = book["trs"]
    assert len(set(trs)) == len(trs)
    text = " ".join([trs[REPEATED]] + trs)
    own, at = [], len(trs[REPEATED]) + 1
    for tr in trs:
        own.append((at, at + len(tr)))
        at += len(tr) + 1
    assert [text[a:b] for a, b in own] == trs and text[:len(trs[REPEATED])] == trs[REPEATED]
    return dict(book, text=text, own=own)


def test_every_page_at_its_own_place_where_the_single_search_takes_the_first_copy(volume, monkeypatch):
    from text_alignment_amd import alignToOCR as atocr
    pages, rec, params, text, own = (volume[k] for k in ("pages", "rec", "params", "text", "own"))
    monkeypatch.setattr(atocr, "PIPELINE_CHUNK_PAGES", 2)          # several chunks of recognition in front of ONE chain
    spans = atocr.locate_book(pages, text, rec, params)
    assert spans == own
    assert atocr.locate_book(pages, text, [rec] * len(pages), params) == own
    alone = []
    atocr.process_batch(pages, [text] * len(pages), rec, params, locate=True, spans_out=alone)
    first_copy = (0, len(volume["trs"][REPEATED]))
    assert alone == [first_copy if p == REPEATED else own[p] for p in range(len(pages))]
    assert atocr.locate_book([], text, rec, params) == []


def test_process_book_is_process_batch_on_the_pages_own_spans(volume, monkeypatch):
    from text_alignment_amd import alignToOCR as atocr
    pages, rec, params, text = (volume[k] for k in ("pages", "rec", "params", "text"))
    monkeypatch.setattr(atocr, "PIPELINE_CHUNK_PAGES", 2)
    spans, idx, arr = [], [], []
    res = atocr.process_book(pages, text, rec, params, spans_out=spans, indices_out=idx, arrays_out=arr)
    assert spans == volume["own"]
    idx1, arr1 = [], []
    want = atocr.process_batch(pages, [text[a:b] for a, b in spans], rec, params, indices_out=idx1, arrays_out=arr1)
    _same((res, idx, arr), (want, idx1, arr1))
    ref, ref1 = [], []                                             # a switch passed through
    res = atocr.process_book(pages, text, rec, params, refine=True, min_agreement=(4, 5), refined_out=ref)
    want = atocr.process_batch(pages, volume["trs"], rec, params, refine=True, min_agreement=(4, 5), refined_out=ref1)
    assert [r.tolist() for r in ref] == [r.tolist() for r in ref1] and len(res) == len(want)
    for p in range(len(res)):
        assert np.array_equal(res[p][0].boxes, want[p][0].boxes)


def test_refusals_up_front(volume, monkeypatch):
    from text_alignment_amd import alignToOCR as atocr, ocr
    pages, rec, params, text, om = (volume[k] for k in ("pages", "rec", "params", "text", "om"))
    monkeypatch.setattr(atocr.PageChunk, "launch", lambda *a, **k: pytest.fail("GPU work before the refusal"))
    codec = list(om.codec)
    codec[5] = "ab"                                                # a codec with a multi-character entry
    bad_rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, codec))
    for fn in (atocr.locate_book, atocr.process_book):
        with pytest.raises(ValueError):
            fn(pages, text, rec, [8.5, -12, -6, -6, -2, -2])
        with pytest.raises(ValueError):
            fn(pages, text, rec, [lambda a, b: 1, -6, -6, -2, -2])
        with pytest.raises(ValueError):
            fn(pages, text, bad_rec, params)
        with pytest.raises(ValueError):
            fn(pages, text, [rec], params)                         # a list of models: one per page
        with pytest.raises(ValueError):
            fn(pages, [text] * len(pages), rec, params)            # the book is ONE string
    with pytest.raises(ValueError):
        atocr.process_book(pages, text, rec, params, locate=True)
