"""forced.refine_pages(scope="page", page_confidence=True) end to end on the GPU, on tests/test_refine_page_gpu.py's four
synthetic pages of three short lines: the switch changes nothing else, every value equals the checker
tests/forced_page_conf_ref.py on the run's own windows and downloaded probabilities, the per-syllable values equal a
restatement, and alignToOCR.process and tools/rforced.py --page-confidence hand the same values on."""
import numpy as np
import pytest

import forced_page_conf_ref as R
import forced_page_ref as PR
from test_refine_page_gpu import PARAMS, run  # noqa: F401  (the module's fixture: the four pages and their transcripts)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _same(x, y):
    return (x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y))


def _same_result(a, b):
    assert a.page_scope.tolist() == b.page_scope.tolist() and a.page_score == b.page_score and a.indices == b.indices
    assert np.array_equal(a.refined, b.refined)
    assert all(_same(x, y) for x, y in zip(a.page_frames, b.page_frames)) and all(_same(x, y) for x, y in zip(a.frames, b.frames))
    assert all(np.array_equal(x, y) for x, y in zip(a.arrays, b.arrays))
    for p in range(len(a)):
        assert a.results[p][0].chars == b.results[p][0].chars and np.array_equal(a.results[p][0].boxes, b.results[p][0].boxes)


def test_page_confidence_equals_the_checker_and_changes_nothing_else(run):  # noqa: F811
    from text_alignment_amd import alignToOCR as atocr, forced, page_batch as pb, train
    pages, trs, rec, om = run["pages"], run["trs"], run["rec"], run["om"]
    base = forced.refine_pages(pages, trs, rec, PARAMS, scope="page")
    off = forced.refine_pages(pages, trs, rec, PARAMS, scope="page", page_confidence=False)
    _same_result(off, base)
    for name in ("page_confidence", "page_rival", "confidence", "rival", "char_confidence", "syllable_confidence"):
        assert getattr(off, name) is None
    res = forced.refine_pages(pages, trs, rec, PARAMS, scope="page", page_confidence=True)
    _same_result(res, base)
    h = res.harvest
    P = res.probs.cpu().numpy()
    for p in range(4):
        a, b = int(h.line_first[p]), int(h.line_first[p + 1])
        cs = train.encode_text(om.codec, trs[p])
        assert res.page_scope[p] == 0
        lo, hi = res.windows[p]
        Ps = [P[int(res.row_off[q]):int(res.row_off[q]) + int(res.T[q])] for q in range(a, b)]
        fr = res.page_frames[p]
        conf, rival, own = R.query_tables(R.tables(Ps, cs, lo, hi)[2], lo, hi, fr[:, 0], fr[:, 3])
        assert (own == res.page_score[p]).all() and (conf >= 0).all()
        assert np.array_equal(res.page_confidence[p], conf) and np.array_equal(res.page_rival[p], rival)
        assert res.page_confidence[p].dtype == np.int64 and res.page_rival[p].dtype == np.int32
        assert np.array_equal(res.char_confidence[p], conf)
        for q in range(a, b):
            assert np.array_equal(res.confidence[q], conf[fr[:, 0] == q - a]) and np.array_equal(res.rival[q], rival[fr[:, 0] == q - a])
        # per syllable: the smallest value among the characters the glue forms its box over, restated
        first, last = pb.syllable_spans(trs[p], run_syllables(trs[p]))
        want = [int(conf[int(f):int(l) + 1].min()) for f, l in zip(first, last)]
        assert res.syllable_confidence[p] == [want[i] for i in res.indices[p]]
        pc = forced.result_confidence(res, p)
        assert pc.char_confidence is res.char_confidence[p] and pc.syllable_confidence == res.syllable_confidence[p]
        assert len(pc.confidence) == 3 and all(np.array_equal(x, y) for x, y in zip(pc.rival, res.rival[a:b]))
    # process(...) hands the page's values on
    out = []
    single = atocr.process(pages[1], trs[1], rec, PARAMS, refine=True, refine_scope="page", page_confidence=True,
                           confidence_out=out)
    assert np.array_equal(single[0].boxes, res.results[1][0].boxes) and len(out) == 1
    assert np.array_equal(out[0].char_confidence, res.char_confidence[1])
    assert out[0].syllable_confidence == res.syllable_confidence[1]
    assert all(np.array_equal(x, y) for x, y in zip(out[0].confidence, res.confidence[3:6]))
    assert all(np.array_equal(x, y) for x, y in zip(out[0].rival, res.rival[3:6]))


def run_syllables(tr):
    from text_alignment_amd import latinSyllabification as latsyl
    return latsyl.syllabify_text(tr)


def test_a_page_that_is_not_refined_has_no_values(run):  # noqa: F811
    from text_alignment_amd import forced
    pages, trs, rec = run["pages"], run["trs"], run["rec"]
    tr = [trs[0][:4] + "é" + trs[0][4:], trs[1]]
    res = forced.refine_pages(pages[:2], tr, rec, PARAMS, scope="page", page_confidence=True)
    assert res.page_scope.tolist() == [forced.PAGE_CLASS0, 0]
    assert res.page_confidence[0] is None and res.page_rival[0] is None and res.page_confidence[1] is not None
    assert (res.char_confidence[0] == forced.NO_CONFIDENCE).all() and len(res.char_confidence[0]) == len(tr[0])
    assert res.syllable_confidence[0] == [None] * len(res.indices[0])
    assert res.confidence[:3] == [None] * 3 and res.rival[:3] == [None] * 3
    assert sum(len(c) for c in res.confidence[3:6]) == len(tr[1])


def test_the_value_errors(run):  # noqa: F811
    from text_alignment_amd import alignToOCR as atocr, forced
    pages, trs, rec = run["pages"][:1], run["trs"][:1], run["rec"]
    for kw in (dict(scope="line", page_confidence=True), dict(page_confidence=True),
               dict(scope="page", page_confidence=True, page_omit=2.0), dict(scope="page", page_confidence=1),
               dict(scope="page", page_confidence="yes"), dict(scope="page", page_confidence=None),
               dict(scope="page", confidence=True), dict(scope="page", page_confidence=True, confidence=True)):
        with pytest.raises(ValueError):
            forced.refine_pages(pages, trs, rec, PARAMS, **kw)
    with pytest.raises(ValueError):
        atocr.process(pages[0], trs[0], rec, PARAMS, page_confidence=True)
    with pytest.raises(ValueError):
        atocr.process(pages[0], trs[0], rec, PARAMS, refine=True, page_confidence=True)          # line scope
    with pytest.raises(TypeError):
        atocr.process_batch(pages, trs, rec, PARAMS, refine=True, page_confidence=True)


def test_align_page_lines_and_rforced_write_the_checkers_values(tmp_path):
    """forced.align_page_lines(confidence=True) on three raw line images, and tools/rforced.py --page --page-confidence in
    process: a NAME.conf per line, in --confidence's format, that together hold the page's values"""
    from PIL import Image
    from oracle import ocr_ref_f64 as OR
    from test_errs_gpu import _strip
    from text_alignment_amd import forced, model_io, ocr, train
    from tools import rforced
    om = OR.synthetic_model(7001, no=40)
    path = str(tmp_path / "m.pyrnn.gz")
    model_io.save_pyrnn(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec), path)
    rng = np.random.default_rng(22)
    strips = [_strip(rng, 40, 100), _strip(rng, 48, 80), _strip(rng, 40, 110)]
    for k, img in enumerate(strips):
        Image.fromarray(img).save(str(tmp_path / ("line%d.png" % k)))
    (tmp_path / "page.txt").write_text("gloria in\nexcelsis  deo\n", encoding="utf-8")
    text = "gloria in excelsis deo"
    lines, score, run_, conf = forced.align_page_lines(path, strips, text, want_run=True, confidence=True)
    plain = forced.align_page_lines(path, strips, text)
    assert (lines, score) == plain and conf.shape == (len(text), 2) and conf.dtype == np.int64
    Pd = run_["probs"].cpu().numpy()
    Ps = [Pd[int(r):int(r) + int(t)] for r, t in zip(run_["row_off"], run_["T"])]
    cs = train.encode_text(om.codec, text)
    fr = run_["frames"]
    want, rival, own = R.query_tables(R.tables(Ps, cs, [0] * 3, [len(cs)] * 3)[2], [0] * 3, [len(cs)] * 3, fr[:, 0], fr[:, 3])
    assert np.array_equal(conf[:, 0], want) and np.array_equal(conf[:, 1], rival) and (own == score).all()
    with pytest.raises(ValueError):
        forced.align_page_lines(path, strips, text, omit=2.0, confidence=True)
    written, score2 = rforced.main([str(tmp_path), "-m", path, "--page", str(tmp_path / "page.txt"), "--page-confidence"])
    assert score2 == score
    rows = []
    for k, (out, count) in enumerate(written):
        got = [r.split("\t") for r in open(out[:-len(".llocs")] + ".conf", encoding="utf-8").read().split("\n") if r]
        assert len(got) == count == len(lines[k])
        rows += got
    assert "".join(r[0] for r in rows) == text
    assert [r[1] for r in rows] == ["%.3f" % (c / 65536.0) for c in want]
    assert [r[2] for r in rows] == [text[(int(s) - 1) // 2] if int(s) & 1 else "~" for s in rival]
    with pytest.raises(SystemExit):
        rforced.main([str(tmp_path), "-m", path, "--page-confidence"])
    with pytest.raises(SystemExit):
        rforced.main([str(tmp_path), "-m", path, "--page", str(tmp_path / "page.txt"), "--page-confidence", "--page-omit", "2"])
