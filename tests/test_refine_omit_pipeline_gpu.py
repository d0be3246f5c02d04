"""process_batch(..., refine=True, line_omit=BITS): forced alignment with omission inside the three-stage pipeline against
forced.refine_pages(omit=BITS) page by page -- the seven pages of tests/test_refine_pipeline_gpu.py (the lead chunk, the
steady loop and the drain all run: PIPELINE_CHUNK_PAGES patched to 2), their transcripts built as
tests/test_refine_omit_gpu.py builds them: three letters a line does not hold, inserted in front of one of its words."""
import numpy as np
import pytest

from test_refine_omit_gpu import AGREE, OMIT, PARAMS
from test_refine_pipeline_gpu import SEEDS, _same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def book():
    """the seven pages, their transcripts with the extra letters, and refine_pages(omit=OMIT) on every page alone"""
    from oracle import ocr_ref_f64 as OR
    from test_forced_gpu import _line_texts, _model, _second_transcript
    from test_page_gpu import _page
    from text_alignment_amd import alignToOCR as atocr, forced, latinSyllabification as latsyl, ocr, page as page_mod
    om = _model(OR)
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    pages = [_page(seed, 3 + k % 2, OR, page_mod)[0] for k, seed in enumerate(SEEDS)]
    one = atocr.process_batch(pages, ["amen"] * len(pages), rec, PARAMS)
    built = [_second_transcript(_line_texts(r[3], pg), latsyl) for r, pg in zip(one, pages)]
    # the extra letters alone, without the space _second_transcript puts behind them (tests/test_refine_omit_gpu.py)
    trs = [tr[:hi + 1] + tr[hi + 2:] for tr, (lo, hi) in built]
    alone = [forced.refine_pages([pg], [tr], rec, PARAMS, min_agreement=AGREE, omit=OMIT) for pg, tr in zip(pages, trs)]
    return dict(rec=rec, pages=pages, trs=trs, alone=alone)


def _run(book, monkeypatch, chunk=2, **kw):
    from text_alignment_amd import alignToOCR as atocr
    monkeypatch.setattr(atocr, "PIPELINE_CHUNK_PAGES", chunk)
    idx, arr = [], []
    res = atocr.process_batch(kw.pop("pages", book["pages"]), kw.pop("trs", book["trs"]), book["rec"], PARAMS,
                              indices_out=idx, arrays_out=arr, **kw)
    return res, idx, arr


def _counts(res):
    """RefineResult.omitted of one page alone, None as -1"""
    return [-1 if g is None else int(g) for g in res.omitted]


def test_the_pipeline_omits_as_refine_pages_does_page_by_page(book, monkeypatch):
    alone = book["alone"]
    # ---- the reference run alone: something is omitted, and on a line that is refined
    assert sum(g for a in alone for g in _counts(a) if g > 0) > 0
    assert any(g > 0 and r for a in alone for g, r in zip(_counts(a), a.refined))
    assert all(a.object_pages == [] for a in alone)
    refined, omitted = [], []
    got = _run(book, monkeypatch, refine=True, min_agreement=AGREE, line_omit=OMIT, refined_out=refined, omitted_out=omitted)
    assert len(refined) == 7 and len(omitted) == 7
    for p, a in enumerate(alone):
        assert omitted[p].dtype == np.int32 and omitted[p].tolist() == _counts(a), p
        assert refined[p].dtype == bool and refined[p].tolist() == np.asarray(a.refined, dtype=bool).tolist(), p
        assert got[1][p] == a.indices[0] and np.array_equal(got[2][p], a.arrays[0]), p
        assert [s.char for s in got[0][p][0]] == [s.char for s in a.results[0][0]]
        assert np.array_equal(got[0][p][0].boxes, a.results[0][0].boxes)
        assert got[0][p][3].chars == a.results[0][3].chars and np.array_equal(got[0][p][3].boxes, a.results[0][3].boxes)
    strict = _run(book, monkeypatch, refine=True, min_agreement=AGREE)
    assert any(not np.array_equal(got[2][p], strict[2][p]) for p in range(7))      # the switch changed boxes
    again = []
    _same(got, _run(book, monkeypatch, refine=True, min_agreement=AGREE, line_omit=OMIT, omitted_out=again))
    assert [g.tolist() for g in again] == [g.tolist() for g in omitted]            # a second call: the same bytes
    whole = []
    _same(got, _run(book, monkeypatch, chunk=16, refine=True, min_agreement=AGREE, line_omit=OMIT, omitted_out=whole))
    assert [g.tolist() for g in whole] == [g.tolist() for g in omitted]            # one chunk for all pages


def test_line_omit_none_is_the_call_without_the_argument(book, monkeypatch):
    from text_alignment_amd import _native, forced
    for entry in ("ta_forced_align_omit_lines", "ta_refine_columns_omit"):
        monkeypatch.setattr(_native.lib, entry, lambda *a, entry=entry: pytest.fail("%s without the switch" % entry))
    monkeypatch.setattr(forced, "present_box_rows", lambda *a, **k: pytest.fail("the row scatter without the switch"))
    omitted = []
    _same(_run(book, monkeypatch, refine=True, min_agreement=AGREE),
          _run(book, monkeypatch, refine=True, min_agreement=AGREE, line_omit=None, omitted_out=omitted))
    assert omitted == []


def test_locate_on_padded_transcripts(book, monkeypatch):
    """every page's transcript with its neighbours' around it: the spans are found first, the refinement runs on them"""
    trs = book["trs"]
    padded = [" ".join(([trs[p - 1]] if p else []) + [trs[p]] + ([trs[p + 1]] if p + 1 < len(trs) else [])) for p in range(7)]
    spans, omitted, own = [], [], []
    got = _run(book, monkeypatch, trs=padded, locate=True, spans_out=spans, refine=True, min_agreement=AGREE,
               line_omit=OMIT, omitted_out=omitted)
    assert [padded[p][a:b] for p, (a, b) in enumerate(spans)] == trs
    _same(got, _run(book, monkeypatch, refine=True, min_agreement=AGREE, line_omit=OMIT, omitted_out=own))
    assert [g.tolist() for g in omitted] == [g.tolist() for g in own] == [_counts(a) for a in book["alone"]]
