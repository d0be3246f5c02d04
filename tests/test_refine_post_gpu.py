"""forced.refine_pages(posterior=True) end to end on the GPU: the four synthetic pages, the seeded model and the
transcripts of tests/test_refine_conf_gpu.py.  Without the switch the result is what it was; with it results, frames and
scores stay what they are, the per-line values equal the checker tests/forced_post_ref.py bit for bit on the run's own
downloaded probabilities, and the per-character and per-syllable values equal a restatement here.  Then process and
tools/rforced.py --posterior."""
import numpy as np
import pytest

import forced_post_ref as R
from test_forced_gpu import _line_texts, _model, _second_transcript
from test_refine_conf_gpu import AGREE, PARAMS, SEEDS, _same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NAMES = ("posterior", "rival_posterior", "posterior_rival", "loglik_bits", "char_posterior", "syllable_posterior")


@pytest.fixture(scope="module")
def run():
    from oracle import ocr_ref_f64 as OR
    from test_page_gpu import _page
    from text_alignment_amd import alignToOCR as atocr, forced, latinSyllabification as latsyl, ocr, page as page_mod
    om = _model(OR)
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    pages = [_page(seed, 3, OR, page_mod)[0] for seed in SEEDS]
    one = atocr.process_batch(pages, ["amen"] * len(pages), rec, PARAMS)
    built = [_second_transcript(_line_texts(r[3], pg), latsyl) for r, pg in zip(one, pages)]
    trs = [b[0][:b[1][1] + 1] + b[0][b[1][1] + 2:] for b in built]       # tests/test_refine_omit_gpu.py's transcripts
    plain = forced.refine_pages(pages, trs, rec, PARAMS, AGREE)
    post = forced.refine_pages(pages, trs, rec, PARAMS, AGREE, posterior=True)
    return {"om": om, "rec": rec, "pages": pages, "trs": trs, "plain": plain, "post": post}


def test_without_the_switch_the_result_is_what_it_was(run):
    from text_alignment_amd import forced
    old = run["plain"]
    new = forced.refine_pages(run["pages"], run["trs"], run["rec"], PARAMS, AGREE, posterior=False)
    _same(new, old)
    for res in (old, new):
        assert all(getattr(res, name) is None for name in NAMES)


def test_with_the_switch_results_frames_and_scores_stay(run):
    _same(run["post"], run["plain"])
    assert run["post"].refined.any() and run["post"].confidence is None


def test_line_values_equal_the_checker_on_the_runs_own_probabilities(run):
    from text_alignment_amd import train
    res, om = run["post"], run["om"]
    P = res.probs.cpu().numpy()
    seen = 0
    for q, ln in enumerate(res.harvest.lines):
        if res.frames[q] is None:
            assert all(getattr(res, name)[q] is None for name in NAMES[:4])
            continue
        T = int(res.T[q])
        Pq = P[int(res.row_off[q]):int(res.row_off[q]) + T]
        want = R.query(Pq, train.encode_text(om.codec, ln.text), res.frames[q][:, 2])
        z = want["z_m"], want["z_x"]
        assert res.posterior[q].dtype == np.float64 and res.posterior_rival[q].dtype == np.int32
        assert R.same_bits(res.posterior[q], R.posterior(want["own_m"], want["own_x"], *z))
        assert R.same_bits(res.rival_posterior[q], R.posterior(want["rival_m"], want["rival_x"], *z))
        assert np.array_equal(res.posterior_rival[q], want["rival_state"])
        assert res.loglik_bits[q] == float(R.loglik_bits(*z)) and res.loglik_bits[q] < 0
        assert (res.posterior[q] > 0).all() and (res.posterior[q] <= 1 + 8 * T * 2.0 ** -53).all()
        seen += len(res.posterior[q])
    assert seen > 0 and all(len(getattr(res, name)) == len(res.frames) for name in NAMES[:4])


def test_character_and_syllable_posteriors_equal_a_restatement(run):
    from text_alignment_amd import latinSyllabification as latsyl, page_batch as pb
    res, trs = run["post"], run["trs"]
    h = res.harvest
    assert res.object_pages == []
    with_value = 0
    for p in range(4):
        want = {}                                        # transcript character -> posterior, the refined lines' kept ones
        for q in range(int(h.line_first[p]), int(h.line_first[p + 1])):
            if res.refined[q]:
                for k, c in enumerate(res.posterior[q].tolist()):
                    want[int(h.table[q][1]) + k] = c
        cp = res.char_posterior[p]
        assert cp.dtype == np.float64 and len(cp) == len(trs[p])
        assert R.same_bits(cp, [want.get(i, np.nan) for i in range(len(trs[p]))])
        first, last = pb.syllable_spans(trs[p], latsyl.syllabify_text(trs[p]))
        per_syl = res.syllable_posterior[p]
        assert len(per_syl) == len(res.results[p][0]) == len(res.indices[p])
        for got, k in zip(per_syl, res.indices[p]):
            have = [want[i] for i in range(int(first[k]), int(last[k]) + 1) if i in want]
            assert got == (min(have) if have else None)
            with_value += got is not None
    assert with_value > 0


def test_posterior_is_refused_with_omit_and_at_page_scope(run):
    from text_alignment_amd import forced
    for over in (dict(omit=2.0), dict(scope="page"), dict(omit=0)):
        with pytest.raises(ValueError):
            forced.refine_pages(run["pages"], run["trs"], run["rec"], PARAMS, AGREE, posterior=True, **over)


def test_process_passes_the_switch_through(run):
    from text_alignment_amd import alignToOCR as atocr, forced
    res = run["post"]
    alone = forced.refine_pages(run["pages"][:1], run["trs"][:1], run["rec"], PARAMS, AGREE, posterior=True)
    mine = []
    got = atocr.process(run["pages"][0], run["trs"][0], run["rec"], PARAMS, refine=True, min_agreement=AGREE, posterior=True,
                        posterior_out=mine)
    assert np.array_equal(got[0].boxes, alone.results[0][0].boxes) and len(mine) == 1
    pp = mine[0]
    assert isinstance(pp, forced.PagePosterior)
    assert R.same_bits(pp.char_posterior, alone.char_posterior[0]) and pp.syllable_posterior == alone.syllable_posterior[0]
    assert pp.loglik_bits == alone.loglik_bits and len(pp.posterior) == int(res.harvest.line_first[1])
    for a, b in zip(pp.posterior + pp.rival_posterior, alone.posterior + alone.rival_posterior):
        assert (a is None and b is None) or R.same_bits(a, b)
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(pp.posterior_rival, alone.posterior_rival))
    out = []
    atocr.process(run["pages"][0], run["trs"][0], run["rec"], PARAMS, refine=True, min_agreement=AGREE, posterior_out=out)
    assert out == []                                     # without the switch the list is left alone
    with pytest.raises(ValueError):
        atocr.process(run["pages"][0], run["trs"][0], run["rec"], PARAMS, posterior=True)
    with pytest.raises(ValueError):
        atocr.process(run["pages"][0], run["trs"][0], run["rec"], PARAMS, refine=True, posterior=True, omit=2.0)


def test_rforced_with_posterior_writes_a_row_per_character(tmp_path, capsys):
    """tools/rforced.py --posterior in process: NAME.post beside NAME.llocs, a row per character with its posterior, its
    rival's character and posterior; the line's log2 P(text | line) per frame in the summary; --omit and --page are
    argparse errors with it; the rows of NAME.llocs are what they are without the switch"""
    from PIL import Image
    from oracle import ocr_ref_f64 as OR
    from test_errs_gpu import _strip
    from text_alignment_amd import forced, model_io, ocr
    from tools import rforced
    om = OR.synthetic_model(7001, no=40)
    model = ocr.LineModel(om.fwd, om.rev, om.W2, om.codec)
    path = str(tmp_path / "m.pyrnn.gz")
    model_io.save_pyrnn(model, path)
    rng = np.random.default_rng(4)
    strips = [_strip(rng, 40, 180), _strip(rng, 52, 260)]
    texts = ["et in terra pax hominibus", "gloria patri et filio"]
    for k, (img, tx) in enumerate(zip(strips, texts)):
        Image.fromarray(img).save(str(tmp_path / ("l%d.png" % k)))
        (tmp_path / ("l%d.gt.txt" % k)).write_text(tx + "\n", encoding="utf-8")
    written = rforced.main([str(tmp_path), "-m", path, "--posterior"])
    io = capsys.readouterr()
    want, run_, post = forced.align_lines(path, strips, texts, want_run=True, posterior=True)
    per_frame = [lp.loglik_bits / int(t) for lp, t in zip(post, run_["T"])]
    for (out, score), (chars, sc), lp, tx, pf in zip(written, want, post, texts, per_frame):
        rows = [r.split("\t") for r in open(out, encoding="utf-8").read().split("\n")[:-1]]
        assert score == sc and [r[0] for r in rows] == list(tx) and [r[1] for r in rows] == ["%.1f" % e[4] for e in chars]
        rows = [r.split("\t") for r in open(out[:-len(".llocs")] + ".post", encoding="utf-8").read().split("\n")[:-1]]
        assert [r[0] for r in rows] == list(tx)
        assert [r[1] for r in rows] == ["%.4f" % v for v in lp.posterior]
        assert [r[2] for r in rows] == [tx[(int(s) - 1) // 2] if int(s) % 2 else "~" for s in lp.rival_state]
        assert [r[3] for r in rows] == ["%.4f" % v for v in lp.rival_posterior]
        assert "log2 P(text | line) %.3f bits per frame" % pf in io.out
    assert "lowest log2 P(text | line) per frame %.3f bits" % min(per_frame) in io.out
    assert "2 of 2 lines written\n" in io.out
    for extra in (["--omit", "0.5"], ["--page", path]):
        with pytest.raises(SystemExit) as e:
            rforced.main([str(tmp_path), "-m", path, "--posterior"] + extra)
        assert e.value.code == 2
    capsys.readouterr()
