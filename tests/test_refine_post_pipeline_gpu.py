"""process_batch(..., refine=True, posterior=True): the sum-product posteriors inside the three-stage pipeline against
forced.refine_pages(posterior=True) page by page, BIT FOR BIT -- the seven-page book of tests/test_refine_pipeline_gpu.py
(PIPELINE_CHUNK_PAGES patched to 2: lead chunk, steady loop and drain all run; min_agreement 4/5, 23 of 24 lines accepted,
the first line of the last page LOW, so the book holds valued and valueless syllables and lines)."""
import numpy as np
import pytest

from forced_post_ref import same_bits
from test_refine_conf_pipeline_gpu import _equals_alone as _confidence_equals_alone
from test_refine_pipeline_gpu import SEEDS, _run, _same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

AGREE = dict(refine=True, min_agreement=(4, 5))


@pytest.fixture(scope="module")
def book():
    """the seven pages, their second-pass transcripts, and refine_pages(confidence=True, posterior=True) on every page
    alone -- once"""
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
    alone = [forced.refine_pages([pg], [tr], rec, params, min_agreement=(4, 5), confidence=True, posterior=True)
             for pg, tr in zip(pages, trs)]
    return dict(om=om, rec=rec, params=params, pages=pages, trs=trs, alone=alone)


def _lines_same(got, want, floats):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if w is None:
            continue
        if floats:
            assert np.asarray(g).dtype == np.float64 and same_bits(g, w)
        else:
            assert g.dtype == w.dtype == np.int32 and np.array_equal(g, w)


def _equals_alone(post, alone):
    """every posterior_out field of every page against refine_pages on that page alone"""
    assert len(post) == len(alone)
    for c, a in zip(post, alone):
        want = a if not hasattr(a, "results") else type(c)(a, 0)
        assert c.char_posterior.dtype == np.float64 and same_bits(c.char_posterior, want.char_posterior)
        assert len(c.syllable_posterior) == len(want.syllable_posterior)
        for g, w in zip(c.syllable_posterior, want.syllable_posterior):
            assert (g is None) == (w is None) and (w is None or (type(g) is float and same_bits(g, w)))
        _lines_same(c.posterior, want.posterior, True)
        _lines_same(c.rival_posterior, want.rival_posterior, True)
        _lines_same(c.posterior_rival, want.posterior_rival, False)
        _lines_same(c.loglik_bits, want.loglik_bits, True)
        assert all(v is None or type(v) is float for v in c.loglik_bits)


def test_the_pipeline_gives_the_posteriors_refine_pages_gives_page_by_page(book, monkeypatch):
    alone = book["alone"]
    assert sum(int(np.asarray(a.refined).sum()) for a in alone) == 23 and sum(len(a.refined) for a in alone) == 24
    per_syl = [v for a in alone for v in a.syllable_posterior[0]]
    assert any(v is None for v in per_syl) and any(v is not None for v in per_syl)
    assert any(c is None for a in alone for c in a.posterior) and any(c is not None for a in alone for c in a.posterior)
    assert any(np.isnan(a.char_posterior[0]).any() for a in alone) and any((~np.isnan(a.char_posterior[0])).any() for a in alone)
    post, refined = [], []
    got = _run(book, monkeypatch, posterior=True, posterior_out=post, refined_out=refined, **AGREE)
    _equals_alone(post, alone)
    assert [r.tolist() for r in refined] == [np.asarray(a.refined, dtype=bool).tolist() for a in alone]
    # results, indices, arrays and refined_out are byte for byte those of the call without the switch
    plain_ref = []
    plain = _run(book, monkeypatch, refined_out=plain_ref, **AGREE)
    _same(got, plain)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(refined, plain_ref))
    # a second call returns the same bytes
    post2 = []
    _same(got, _run(book, monkeypatch, posterior=True, posterior_out=post2, **AGREE))
    _equals_alone(post2, alone)
    _equals_alone(post2, post)
    # one chunk for all pages: the branch without the pipeline
    post16 = []
    _same(got, _run(book, monkeypatch, chunk=16, posterior=True, posterior_out=post16, **AGREE))
    _equals_alone(post16, alone)


def test_confidence_and_posterior_together_give_both(book, monkeypatch):
    conf, post = [], []
    got = _run(book, monkeypatch, confidence=True, confidence_out=conf, posterior=True, posterior_out=post, **AGREE)
    _confidence_equals_alone(conf, book["alone"])
    _equals_alone(post, book["alone"])
    _same(got, _run(book, monkeypatch, **AGREE))
    conf16, post16 = [], []
    _run(book, monkeypatch, chunk=16, confidence=True, confidence_out=conf16, posterior=True, posterior_out=post16, **AGREE)
    _confidence_equals_alone(conf16, book["alone"])
    _equals_alone(post16, book["alone"])


def test_the_switch_off_is_the_call_without_the_argument(book, monkeypatch):
    from text_alignment_amd import forced
    post = []
    launched = []
    for name in ("posterior_lines", "posterior_pages"):
        monkeypatch.setattr(forced.Refining, name, lambda self, name=name: launched.append(name))
    _same(_run(book, monkeypatch, **AGREE), _run(book, monkeypatch, posterior=False, posterior_out=post, **AGREE))
    assert post == [] and launched == []
    _same(_run(book, monkeypatch, chunk=16, **AGREE), _run(book, monkeypatch, chunk=16, posterior=False, posterior_out=post, **AGREE))
    assert post == [] and launched == []
    conf = []
    _run(book, monkeypatch, confidence=True, confidence_out=conf, **AGREE)       # nor does the confidence start them
    assert len(conf) == 7 and post == [] and launched == []


def test_posterior_without_refine_is_refused_up_front(book, monkeypatch):
    from text_alignment_amd import alignToOCR as atocr
    monkeypatch.setattr(atocr.PageChunk, "launch", lambda *a, **k: pytest.fail("GPU work before the refusal"))
    with pytest.raises(ValueError):
        atocr.process_batch(book["pages"], book["trs"], book["rec"], book["params"], posterior=True)
    with pytest.raises(ValueError):
        atocr.process_batch(book["pages"], book["trs"], book["rec"], book["params"], posterior=True, refine=False,
                            posterior_out=[])
