"""forced.refine_pages(scope="page", page_posterior=True) end to end on the GPU, on tests/test_refine_page_gpu.py's four
synthetic pages of three short lines: the switch changes nothing else, every value equals the checker
tests/forced_page_post_ref.py bit for bit on the run's own windows and downloaded probabilities, the per-character and
per-syllable values equal a restatement, and alignToOCR.process and tools/rforced.py --page-posterior hand the same values
on."""
import numpy as np
import pytest

import forced_page_post_ref as R
from test_refine_page_conf_gpu import _same_result, run_syllables
from test_refine_page_gpu import PARAMS, run  # noqa: F401  (the module's fixture: the four pages and their transcripts)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NAMES = ("page_posterior", "page_rival_posterior", "page_posterior_rival", "page_loglik_bits", "posterior", "rival_posterior",
         "posterior_rival", "loglik_bits", "char_posterior", "syllable_posterior")


def _checker(res, om, trs, p):
    """the checker's answer for page p on the run's own windows, probabilities and frames, as the host forms the values"""
    from text_alignment_amd import train
    h = res.harvest
    a, b = int(h.line_first[p]), int(h.line_first[p + 1])
    P = res.probs.cpu().numpy()
    Ps = [P[int(res.row_off[q]):int(res.row_off[q]) + int(res.T[q])] for q in range(a, b)]
    lo, hi = res.windows[p]
    fr = res.page_frames[p]
    w = R.query(Ps, train.encode_text(om.codec, trs[p]), lo, hi, fr[:, 0], fr[:, 3])
    assert w["status"] == R.OK
    return (R.posterior(w["own_m"], w["own_x"], w["z_m"], w["z_x"]), R.posterior(w["rival_m"], w["rival_x"], w["z_m"], w["z_x"]),
            w["rival_state"], float(R.loglik_bits(w["z_m"], w["z_x"])), sum(len(x) for x in Ps))


def test_page_posterior_equals_the_checker_and_changes_nothing_else(run):  # noqa: F811
    from text_alignment_amd import alignToOCR as atocr, forced, page_batch as pb
    pages, trs, rec, om = run["pages"], run["trs"], run["rec"], run["om"]
    base = forced.refine_pages(pages, trs, rec, PARAMS, scope="page")
    off = forced.refine_pages(pages, trs, rec, PARAMS, scope="page", page_posterior=False)
    _same_result(off, base)
    for name in NAMES:
        assert getattr(off, name) is None, name
    res = forced.refine_pages(pages, trs, rec, PARAMS, scope="page", page_posterior=True)
    _same_result(res, base)
    assert res.page_confidence is None and res.confidence is None
    h = res.harvest
    for p in range(4):
        a, b = int(h.line_first[p]), int(h.line_first[p + 1])
        assert res.page_scope[p] == 0
        post, rival, state, bits, frames = _checker(res, om, trs, p)
        fr = res.page_frames[p]
        assert R.same_bits(res.page_posterior[p], post) and R.same_bits(res.page_rival_posterior[p], rival)
        assert np.array_equal(res.page_posterior_rival[p], state) and res.page_posterior_rival[p].dtype == np.int32
        assert isinstance(res.page_loglik_bits[p], float) and res.page_loglik_bits[p] == bits and bits < 0
        assert (post > 0).all() and (post <= 1 + 8 * frames * 2.0 ** -53).all() and (rival >= 0).all()
        assert R.same_bits(res.char_posterior[p], post)
        for q in range(a, b):
            on = fr[:, 0] == q - a
            assert R.same_bits(res.posterior[q], post[on]) and R.same_bits(res.rival_posterior[q], rival[on])
            assert np.array_equal(res.posterior_rival[q], state[on]) and res.loglik_bits[q] is None
        # per syllable: the smallest value among the characters the glue forms its box over, restated
        first, last = pb.syllable_spans(trs[p], run_syllables(trs[p]))
        want = [float(post[int(f):int(l) + 1].min()) for f, l in zip(first, last)]
        assert res.syllable_posterior[p] == [want[i] for i in res.indices[p]]
        pp = forced.PagePosterior(res, p)
        assert pp.char_posterior is res.char_posterior[p] and pp.syllable_posterior == res.syllable_posterior[p]
        assert len(pp.posterior) == 3 and pp.loglik_bits == [None] * 3 and pp.page_loglik_bits == bits
        assert all(np.array_equal(x, y) for x, y in zip(pp.posterior_rival, res.posterior_rival[a:b]))
    # together with page_confidence both come back, each as alone
    conf = forced.refine_pages(pages, trs, rec, PARAMS, scope="page", page_confidence=True)
    both = forced.refine_pages(pages, trs, rec, PARAMS, scope="page", page_confidence=True, page_posterior=True)
    _same_result(both, base)
    for p in range(4):
        assert np.array_equal(both.page_confidence[p], conf.page_confidence[p]) and np.array_equal(both.page_rival[p], conf.page_rival[p])
        assert R.same_bits(both.page_posterior[p], res.page_posterior[p]) and both.page_loglik_bits[p] == res.page_loglik_bits[p]
        assert both.syllable_confidence[p] == conf.syllable_confidence[p] and both.syllable_posterior[p] == res.syllable_posterior[p]
    # process(...) hands the page's values on
    out = []
    single = atocr.process(pages[1], trs[1], rec, PARAMS, refine=True, refine_scope="page", page_posterior=True, posterior_out=out)
    assert np.array_equal(single[0].boxes, res.results[1][0].boxes) and len(out) == 1
    assert R.same_bits(out[0].char_posterior, res.char_posterior[1]) and out[0].syllable_posterior == res.syllable_posterior[1]
    assert all(R.same_bits(x, y) for x, y in zip(out[0].posterior, res.posterior[3:6]))
    assert all(np.array_equal(x, y) for x, y in zip(out[0].posterior_rival, res.posterior_rival[3:6]))
    assert out[0].page_loglik_bits == res.page_loglik_bits[1] and out[0].loglik_bits == [None] * 3


def test_the_six_argument_page_posterior_of_stays_valid():
    from text_alignment_amd import forced
    pp = forced.PagePosterior.of(1, 2, 3, 4, 5, 6)
    assert (pp.char_posterior, pp.syllable_posterior, pp.posterior, pp.rival_posterior, pp.posterior_rival, pp.loglik_bits,
            pp.page_loglik_bits) == (1, 2, 3, 4, 5, 6, None)
    assert forced.PagePosterior.of(1, 2, 3, 4, 5, 6, page_loglik_bits=-7.5).page_loglik_bits == -7.5


def test_a_page_that_is_not_refined_has_no_values(run):  # noqa: F811
    from text_alignment_amd import forced
    pages, trs, rec = run["pages"], run["trs"], run["rec"]
    tr = [trs[0][:4] + "é" + trs[0][4:], trs[1]]
    res = forced.refine_pages(pages[:2], tr, rec, PARAMS, scope="page", page_posterior=True)
    assert res.page_scope.tolist() == [forced.PAGE_CLASS0, 0]
    for name in NAMES[:4]:
        assert getattr(res, name)[0] is None and getattr(res, name)[1] is not None, name
    assert np.isnan(res.char_posterior[0]).all() and len(res.char_posterior[0]) == len(tr[0])
    assert res.syllable_posterior[0] == [None] * len(res.indices[0])
    assert res.posterior[:3] == [None] * 3 and res.posterior_rival[:3] == [None] * 3 and res.loglik_bits == [None] * 6
    assert sum(len(c) for c in res.posterior[3:6]) == len(tr[1])
    pp = forced.PagePosterior(res, 0)
    assert pp.page_loglik_bits is None and pp.posterior == [None] * 3


def test_the_value_errors(run):  # noqa: F811
    from text_alignment_amd import alignToOCR as atocr, forced
    pages, trs, rec = run["pages"][:1], run["trs"][:1], run["rec"]
    for kw in (dict(scope="line", page_posterior=True), dict(page_posterior=True),
               dict(scope="page", page_posterior=True, page_omit=2.0), dict(scope="page", page_posterior=1),
               dict(scope="page", page_posterior="yes"), dict(scope="page", page_posterior=None),
               dict(scope="page", posterior=True), dict(scope="page", page_posterior=True, posterior=True)):
        with pytest.raises(ValueError):
            forced.refine_pages(pages, trs, rec, PARAMS, **kw)
    with pytest.raises(ValueError):
        atocr.process(pages[0], trs[0], rec, PARAMS, page_posterior=True)
    with pytest.raises(ValueError):
        atocr.process(pages[0], trs[0], rec, PARAMS, refine=True, page_posterior=True)           # line scope
    with pytest.raises(TypeError):
        atocr.process_batch(pages, trs, rec, PARAMS, refine=True, page_posterior=True)


def test_align_page_lines_and_rforced_write_the_checkers_values(tmp_path, capsys):
    """forced.align_page_lines(posterior=True) on three raw line images, and tools/rforced.py --page --page-posterior in
    process: a NAME.post per line, in --posterior's format, that together hold the page's values, and the page's
    loglik_bits / frames"""
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
    lines, score, run_, post = forced.align_page_lines(path, strips, text, want_run=True, posterior=True)
    assert (lines, score) == forced.align_page_lines(path, strips, text)
    Pd = run_["probs"].cpu().numpy()
    Ps = [Pd[int(r):int(r) + int(t)] for r, t in zip(run_["row_off"], run_["T"])]
    cs = train.encode_text(om.codec, text)
    fr = run_["frames"]
    w = R.query(Ps, cs, [0] * 3, [len(cs)] * 3, fr[:, 0], fr[:, 3])
    want = R.posterior(w["own_m"], w["own_x"], w["z_m"], w["z_x"])
    rival = R.posterior(w["rival_m"], w["rival_x"], w["z_m"], w["z_x"])
    bits = float(R.loglik_bits(w["z_m"], w["z_x"]))
    assert R.same_bits(post.posterior, want) and R.same_bits(post.rival_posterior, rival)
    assert np.array_equal(post.rival_state, w["rival_state"]) and post.loglik_bits == bits
    both = forced.align_page_lines(path, strips, text, confidence=True, posterior=True)
    assert len(both) == 4 and both[2].shape == (len(text), 2) and R.same_bits(both[3].posterior, want)
    with pytest.raises(ValueError):
        forced.align_page_lines(path, strips, text, omit=2.0, posterior=True)
    capsys.readouterr()
    written, score2 = rforced.main([str(tmp_path), "-m", path, "--page", str(tmp_path / "page.txt"), "--page-posterior"])
    assert score2 == score
    frames = int(np.asarray(run_["T"]).sum())
    assert "log2 P(text | page) %.3f bits per frame (%.3f bits on %d frames)" % (bits / frames, bits, frames) in capsys.readouterr().out
    rows = []
    for k, (out, count) in enumerate(written):
        got = [r.split("\t") for r in open(out[:-len(".llocs")] + ".post", encoding="utf-8").read().split("\n") if r]
        assert len(got) == count == len(lines[k])
        rows += got
    assert "".join(r[0] for r in rows) == text
    assert [r[1] for r in rows] == ["%.4f" % v for v in want] and [r[3] for r in rows] == ["%.4f" % v for v in rival]
    assert [r[2] for r in rows] == [text[(int(s) - 1) // 2] if int(s) & 1 else "~" for s in w["rival_state"]]
    with pytest.raises(SystemExit):
        rforced.main([str(tmp_path), "-m", path, "--page-posterior"])
    with pytest.raises(SystemExit):
        rforced.main([str(tmp_path), "-m", path, "--page", str(tmp_path / "page.txt"), "--page-posterior", "--page-omit", "2"])
