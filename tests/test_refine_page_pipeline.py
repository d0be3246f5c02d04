"""process_batch's page-scope keywords without a device: every ValueError of page_margin is
raised before any GPU work -- PageChunk.launch is patched to fail, as tests/test_refine_pipeline_gpu.py::test_refusals_up_front
does -- and before a recogniser is even looked at."""
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


def test_page_scope_without_page_margin_is_the_value_error_it_was(atocr):
    with pytest.raises(ValueError, match="refine_pages"):
        _call(atocr, refine=True, refine_scope="page")
    with pytest.raises(ValueError, match="refine_pages"):
        _call(atocr, refine_scope="page")
    with pytest.raises(ValueError, match="'line' or 'page'"):
        _call(atocr, refine=True, refine_scope="word", page_margin=16)


@pytest.mark.parametrize("bad", [-1, 1.5, 16.0, "16", True, False, np.bool_(True), (16,), np.float32(2)])
def test_page_margin_is_an_integer_of_0_or_more_and_no_bool(atocr, bad):
    with pytest.raises(ValueError, match="page_margin"):
        _call(atocr, refine=True, refine_scope="page", page_margin=bad)


def test_page_margin_goes_with_refine_and_page_scope_alone(atocr):
    with pytest.raises(ValueError, match="refine=True"):
        _call(atocr, refine_scope="page", page_margin=16)
    with pytest.raises(ValueError, match="refine=True"):
        _call(atocr, page_margin=16)
    with pytest.raises(ValueError, match="refine_scope='page'"):
        _call(atocr, refine=True, page_margin=16)
    with pytest.raises(ValueError, match="refine_scope='page'"):
        _call(atocr, refine=True, refine_scope="line", page_margin=0)
    with pytest.raises(ValueError, match="page scope"):
        _call(atocr, refine=True, refine_scope="page", page_margin=16, confidence=True)
    with pytest.raises(ValueError, match="page scope"):
        _call(atocr, refine=True, refine_scope="page", page_margin=np.int64(3), posterior=True)


def test_the_reason_codes_are_the_headers():
    from text_alignment_amd import _abi, forced
    names = ("REFINED", "NOT_PLAIN", "HARVEST", "CLASS0", "NO_TEXT", "WINDOWS", "FRAMES", "NO_PATH")
    assert [_abi.CONSTANTS["TA_PAGE_SCOPE_" + n] for n in names] == list(range(8))
    assert [getattr(forced, "PAGE_" + n) for n in names] == list(range(8))
    assert _abi.CONSTANTS["TA_PAGE_WINDOWS_BOUNDS"] < 0
    s = forced.PageScope(5)
    assert (s.reason, s.windows, s.frames, s.score) == (5, None, None, None)
