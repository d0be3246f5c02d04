"""process_batch(..., refine=True, confidence=True): the per-character confidence inside the three-stage pipeline against
forced.refine_pages(confidence=True) page by page -- the seven-page book of tests/test_refine_pipeline_gpu.py
(PIPELINE_CHUNK_PAGES patched to 2: lead chunk, steady loop and drain all run; min_agreement 4/5, 23 of 24 lines accepted,
the first line of the last page LOW: with the checkers alone 101 of the book's 111 syllables have a character on an accepted
line's kept range and 10, all on that page, have none)."""
import numpy as np
import pytest

from test_refine_pipeline_gpu import SEEDS, _run, _same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

AGREE = dict(refine=True, min_agreement=(4, 5))


@pytest.fixture(scope="module")
def book():
    """the seven pages, their second-pass transcripts, and refine_pages(confidence=True) on every page alone -- once"""
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
    alone = [forced.refine_pages([pg], [tr], rec, params, min_agreement=(4, 5), confidence=True) for pg, tr in zip(pages, trs)]
    return dict(om=om, rec=rec, params=params, pages=pages, trs=trs, alone=alone)


def _lines_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if w is not None:
            assert g.dtype == w.dtype and np.array_equal(g, w)


def _equals_alone(conf, alone):
    """every confidence_out field of every page against refine_pages on that page alone"""
    assert len(conf) == len(alone)
    for c, a in zip(conf, alone):
        assert c.char_confidence.dtype == np.int64 and np.array_equal(c.char_confidence, a.char_confidence[0])
        assert c.syllable_confidence == a.syllable_confidence[0]
        assert all(v is None or type(v) is int for v in c.syllable_confidence)
        _lines_equal(c.confidence, a.confidence)
        _lines_equal(c.rival, a.rival)


def test_the_pipeline_gives_the_confidences_refine_pages_gives_page_by_page(book, monkeypatch):
    from text_alignment_amd import forced
    alone = book["alone"]
    assert sum(int(np.asarray(a.refined).sum()) for a in alone) == 23 and sum(len(a.refined) for a in alone) == 24
    per_syl = [v for a in alone for v in a.syllable_confidence[0]]
    assert any(v is None for v in per_syl) and any(v is not None for v in per_syl)
    assert any(c is None for a in alone for c in a.confidence) and any((a.char_confidence[0] == forced.NO_CONFIDENCE).any()
                                                                       for a in alone)
    conf, refined = [], []
    got = _run(book, monkeypatch, confidence=True, confidence_out=conf, refined_out=refined, **AGREE)
    _equals_alone(conf, alone)
    assert [r.tolist() for r in refined] == [np.asarray(a.refined, dtype=bool).tolist() for a in alone]
    # results, indices, arrays and refined_out are byte for byte those of the call without the switch
    plain_ref = []
    plain = _run(book, monkeypatch, refined_out=plain_ref, **AGREE)
    _same(got, plain)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(refined, plain_ref))
    # a second call returns the same bytes
    conf2 = []
    _same(got, _run(book, monkeypatch, confidence=True, confidence_out=conf2, **AGREE))
    _equals_alone(conf2, alone)
    # one chunk for all pages: the branch without the pipeline
    conf16 = []
    _same(got, _run(book, monkeypatch, chunk=16, confidence=True, confidence_out=conf16, **AGREE))
    _equals_alone(conf16, alone)


def test_the_switch_off_is_the_call_without_the_argument(book, monkeypatch):
    from text_alignment_amd import forced
    conf = []
    launched = []
    for name in ("confidence_lines", "confidence_pages"):
        monkeypatch.setattr(forced.Refining, name, lambda self, name=name: launched.append(name))
    _same(_run(book, monkeypatch, **AGREE), _run(book, monkeypatch, confidence=False, confidence_out=conf, **AGREE))
    assert conf == [] and launched == []
    _same(_run(book, monkeypatch, chunk=16, **AGREE), _run(book, monkeypatch, chunk=16, confidence=False, confidence_out=conf, **AGREE))
    assert conf == [] and launched == []


def test_confidence_without_refine_is_refused_up_front(book, monkeypatch):
    from text_alignment_amd import alignToOCR as atocr
    monkeypatch.setattr(atocr.PageChunk, "launch", lambda *a, **k: pytest.fail("GPU work before the refusal"))
    with pytest.raises(ValueError):
        atocr.process_batch(book["pages"], book["trs"], book["rec"], book["params"], confidence=True)
    with pytest.raises(ValueError):
        atocr.process_batch(book["pages"], book["trs"], book["rec"], book["params"], confidence=True, refine=False,
                            confidence_out=[])
    with pytest.raises(ValueError):
        atocr.process(book["pages"][0], book["trs"][0], book["rec"], book["params"], confidence=True)


def test_process_hands_over_the_batchs_page(book, monkeypatch):
    from text_alignment_amd import alignToOCR as atocr
    conf = []
    got = _run(book, monkeypatch, confidence=True, confidence_out=conf, **AGREE)
    for p in (0, 6):
        mine = []
        res = atocr.process(book["pages"][p], book["trs"][p], book["rec"], book["params"], refine=True, min_agreement=(4, 5),
                            confidence=True, confidence_out=mine)
        assert [s.char for s in res[0]] == [s.char for s in got[0][p][0]] and np.array_equal(res[0].boxes, got[0][p][0].boxes)
        assert len(mine) == 1
        _equals_alone(mine, [book["alone"][p]])
        _equals_alone(mine, [_Page(conf[p])])
        with pytest.raises(ValueError):                       # refine_pages' own refusals pass through
            atocr.process(book["pages"][p], book["trs"][p], book["rec"], book["params"], refine=True, confidence=True, omit=2.0)
    none = []
    atocr.process(book["pages"][0], book["trs"][0], book["rec"], book["params"], refine=True, min_agreement=(4, 5),
                  confidence_out=none)
    assert none == []


class _Page(object):
    """a PageConfidence in the shape _equals_alone reads a RefineResult of one page in"""

    def __init__(self, c):
        self.char_confidence, self.syllable_confidence = [c.char_confidence], [c.syllable_confidence]
        self.confidence, self.rival = c.confidence, c.rival
