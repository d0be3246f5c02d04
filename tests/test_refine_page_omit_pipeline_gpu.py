"""process_batch(..., refine=True, refine_scope="page", page_margin=M, page_scope_omit=BITS): page scope with omission
inside the three-stage pipeline against forced.refine_pages(scope="page", margin=M,
page_omit=BITS) page by page.  The seven interleaved three-line pages of tests/test_refine_page_pipeline_gpu.py (seeds
70 - 73, one PAGE_CLASS0, one PAGE_NOT_PLAIN), their transcripts edited as tests/test_refine_page_omit_gpu.py edits them
(three letters the longest line lacks); PIPELINE_CHUNK_PAGES patched to 2 runs the lead chunk, the steady loop and the
drain."""
import numpy as np
import pytest

from test_refine_page_pipeline_gpu import EDITED, ORDER, PARAMS, _boxes, _run, _same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OMIT, MARGIN = 4.0, 16


def _alone(pages, trs, rec, margin=MARGIN, **kw):
    from text_alignment_amd import forced
    return [forced.refine_pages([pg], [tr], rec, PARAMS, scope="page", margin=margin, page_omit=OMIT, **kw)
            for pg, tr in zip(pages, trs)]


@pytest.fixture(scope="module")
def book():
    """the seven pages, their transcripts, and refine_pages(scope="page", page_omit=4.0) on every page alone -- once"""
    from oracle import ocr_ref_f64 as OR
    from test_forced_gpu import _line_texts, _model, _second_transcript
    from test_page_gpu import _page
    from text_alignment_amd import alignToOCR as atocr, latinSyllabification as latsyl, ocr, page as page_mod
    om = _model(OR)
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    pages = [_page(seed, 3, OR, page_mod)[0] for _, seed in ORDER]
    one = atocr.process_batch(pages, ["amen"] * 7, rec, PARAMS)
    built = [_second_transcript(_line_texts(r[3], pg), latsyl) for r, pg in zip(one, pages)]
    trs = [b[0][:b[1][1] + 1] + b[0][b[1][1] + 2:] for b in built]                  # three letters the longest line lacks
    trs[1] = trs[1][:4] + "é" + trs[1][4:]
    trs[3] = trs[3][:6] + "." + trs[3][6:]
    return dict(om=om, rec=rec, params=PARAMS, pages=pages, trs=trs, alone=_alone(pages, trs, rec))


def _omit_run(book, monkeypatch, margin=MARGIN, **kw):
    refined, scope = [], []
    got = _run(book, monkeypatch, refine=True, refine_scope="page", page_margin=margin, page_scope_omit=OMIT,
               refined_out=refined, page_scope_out=scope, **kw)
    return got, refined, scope


def _equals_alone(got, refined, scope, alone):
    """per page every output of the pipeline against refine_pages(scope="page", page_omit=...) on that page alone"""
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
        assert s.score == a.page_score[0] and s.omitted == a.page_omitted[0], p
        assert (s.omitted is not None) == (s.reason == 0)


def test_the_precondition_from_the_reference_calls_alone(book):
    from text_alignment_amd import forced
    alone = book["alone"]
    reasons = [int(a.page_scope[0]) for a in alone]
    assert sum(r == 0 for r in reasons) >= 5
    for p, name in EDITED.items():
        assert reasons[p] == getattr(forced, name) and not np.asarray(alone[p].refined).any()
    assert sum(a.page_omitted[0] for a in alone if a.page_omitted[0] is not None) >= 1
    assert forced.PAGE_ALL_OMITTED not in reasons
    for a in alone:
        if int(a.page_scope[0]) == 0:
            assert a.page_omitted[0] < len(a.page_frames[0])


def test_the_pipeline_refines_with_omission_as_refine_pages_does_page_by_page(book, monkeypatch):
    got, refined, scope = _omit_run(book, monkeypatch)
    _equals_alone(got, refined, scope, book["alone"])
    again, refined2, scope2 = _omit_run(book, monkeypatch)                      # a second call: the same bytes
    _same(got, again)
    _equals_alone(again, refined2, scope2, book["alone"])
    whole, refined3, scope3 = _omit_run(book, monkeypatch, chunk=16)            # one chunk for all pages
    _same(got, whole)
    _equals_alone(whole, refined3, scope3, book["alone"])
    strict = _run(book, monkeypatch, refine=True, refine_scope="page", page_margin=MARGIN)
    assert any(not np.array_equal(got[2][p], strict[2][p]) for p in range(7))


def test_a_page_with_more_characters_than_frames(book, monkeypatch):
    from text_alignment_amd import forced
    pages, trs, rec = book["pages"], list(book["trs"]), book["rec"]
    frames_all = int(book["alone"][0].T[:3].sum())
    trs[0] = " ".join([trs[0]] * (frames_all // len(trs[0]) + 2))
    assert frames_all < len(trs[0]) <= forced.MAX_TARGET
    scope = []
    _run(book, monkeypatch, trs=trs, refine=True, refine_scope="page", page_margin=1000, page_scope_out=scope)
    assert scope[0].reason == forced.PAGE_FRAMES
    alone = _alone(pages[:2], trs[:2], rec, margin=1000)
    got, refined, scope = _omit_run(book, monkeypatch, margin=1000, pages=pages[:2], trs=trs[:2])
    _equals_alone(got, refined, scope, alone)
    assert scope[0].reason == 0 and scope[0].omitted >= len(trs[0]) - frames_all


def test_the_host_path_is_not_what_ran(book, monkeypatch):
    from text_alignment_amd import forced
    for name in ("page_windows", "page_scope_eligibility", "forced_page_alignment"):
        monkeypatch.setattr(forced, name, lambda *a, _n=name, **k: pytest.fail("forced.%s ran inside the pipeline" % _n))
    got, refined, scope = _omit_run(book, monkeypatch)
    _equals_alone(got, refined, scope, book["alone"])


def test_without_the_price_the_new_entries_do_not_run(book, monkeypatch):
    from text_alignment_amd import _native
    keys = dict(refine=True, refine_scope="page", page_margin=MARGIN)
    before = _run(book, monkeypatch, **keys)

    class Lib(object):
        def __getattr__(self, name):
            if name in ("ta_page_windows_omit", "ta_forced_align_pages_omit_gated", "ta_forced_page_omit_gated_workspace_bytes"):
                pytest.fail("%s ran without page_scope_omit" % name)
            return getattr(before_lib, name)
    before_lib = _native.lib
    monkeypatch.setattr(_native, "lib", Lib())
    _same(before, _run(book, monkeypatch, page_scope_omit=None, **keys))


def test_locate_on_padded_transcripts(book, monkeypatch):
    padded = ["domine deus " + tr + " et in terra" for tr in book["trs"]]
    alone = _alone(book["pages"], padded, book["rec"], locate=True)
    spans = []
    got, refined, scope = _omit_run(book, monkeypatch, trs=padded, locate=True, spans_out=spans)
    assert spans == [a.spans[0] for a in alone]
    _equals_alone(got, refined, scope, alone)
    assert sum(s.reason == 0 for s in scope) >= 4


def test_a_list_of_two_models(book, monkeypatch):
    from text_alignment_amd import ocr
    om = book["om"]
    other = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    recs = [book["rec"] if p % 3 else other for p in range(7)]
    got, refined, scope = _omit_run(book, monkeypatch, rec=recs)
    _equals_alone(got, refined, scope, book["alone"])
