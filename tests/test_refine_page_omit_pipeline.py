"""process_batch's page_scope_omit without a device: every ValueError is raised before any GPU
work -- PageChunk.launch is patched to fail -- and before a recogniser is even looked at; the keyword is not `page_omit`."""
import numpy as np
import pytest

PARAMS = [8, -12, -6, -6, -2, -2]


@pytest.fixture
def atocr(monkeypatch):
    from text_alignment_amd import alignToOCR as atocr
    monkeypatch.setattr(atocr.PageChunk, "launch", lambda *a, **k: pytest.fail("GPU work before the refusal"))
    monkeypatch.setattr(atocr, "_recognizer_for", lambda *a, **k: pytest.fail("a recogniser before the refusal"))
    return atocr


def _call(atocr, **kw):
    return atocr.process_batch([object()], ["amen"], object(), PARAMS, **kw)


def test_page_scope_omit_goes_with_refine_page_scope_and_a_margin(atocr):
    with pytest.raises(ValueError, match="refine=True"):
        _call(atocr, page_scope_omit=4.0)
    with pytest.raises(ValueError, match="refine=True"):
        _call(atocr, refine_scope="page", page_margin=16, page_scope_omit=4.0)
    with pytest.raises(ValueError, match="page scope"):
        _call(atocr, refine=True, page_scope_omit=4.0)
    with pytest.raises(ValueError, match="page scope"):
        _call(atocr, refine=True, refine_scope="line", page_scope_omit=4.0)
    with pytest.raises(ValueError, match="page_margin"):
        _call(atocr, refine=True, refine_scope="page", page_scope_omit=4.0)


def test_page_scope_omit_stands_alone_on_the_lattice_with_omission(atocr):
    page = dict(refine=True, refine_scope="page", page_margin=16)
    with pytest.raises(ValueError, match="line_omit"):
        _call(atocr, page_scope_omit=4.0, line_omit=4.0, **page)
    with pytest.raises(ValueError, match="strict lattice"):
        _call(atocr, page_scope_omit=4.0, confidence=True, **page)
    with pytest.raises(ValueError, match="strict lattice"):
        _call(atocr, page_scope_omit=4.0, posterior=True, **page)


@pytest.mark.parametrize("bad", [True, False, np.bool_(True), "4", (4,), [4], -0.5, -1, 1024.5, 1025, float("nan")])
def test_page_scope_omit_is_a_number_of_bits_in_0_to_1024(atocr, bad):
    with pytest.raises(ValueError, match="omit"):
        _call(atocr, refine=True, refine_scope="page", page_margin=16, page_scope_omit=bad)


def test_the_keyword_is_not_page_omit(atocr):
    with pytest.raises(TypeError):
        _call(atocr, refine=True, refine_scope="page", page_margin=16, page_omit=4.0)
    for name in ("page_confidence", "page_posterior"):
        with pytest.raises(TypeError):
            _call(atocr, refine=True, refine_scope="page", page_margin=16, **{name: True})


def test_the_reason_codes_are_the_headers_and_a_page_scope_has_no_count_by_default():
    from text_alignment_amd import _abi, forced
    assert _abi.CONSTANTS["TA_PAGE_SCOPE_TOO_LONG"] == 8 == forced.PAGE_TOO_LONG
    assert _abi.CONSTANTS["TA_PAGE_SCOPE_ALL_OMITTED"] == 9 == forced.PAGE_ALL_OMITTED
    s = forced.PageScope(5)
    assert (s.reason, s.windows, s.frames, s.score, s.omitted) == (5, None, None, None, None)
    assert forced.PageScope(0, omitted=3).omitted == 3
