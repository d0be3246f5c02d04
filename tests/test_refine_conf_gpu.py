"""forced.refine_pages(confidence=True) end to end on the GPU: the four synthetic pages, the seeded model and the
transcripts of tests/test_refine_omit_gpu.py.  Without the switch the result is what it was; with it results, frames and
scores stay what they are, the per-line confidences and rivals equal the checker tests/forced_conf_ref.py on the run's own
downloaded probabilities, and the per-character and per-syllable values equal a restatement here.  Then
tools/rforced.py --confidence."""
import numpy as np
import pytest

import forced_conf_ref as R
from test_forced_gpu import _line_texts, _model, _second_transcript

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEEDS = (70, 71, 72, 73)
PARAMS = [8, -12, -6, -6, -2, -2]
AGREE = (4, 5)


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
    conf = forced.refine_pages(pages, trs, rec, PARAMS, AGREE, confidence=True)
    return {"om": om, "rec": rec, "pages": pages, "trs": trs, "plain": plain, "conf": conf}


def _same(new, old):
    assert new.page_scope is None and np.array_equal(new.refined, old.refined) and new.indices == old.indices
    assert all(np.array_equal(x, y) for x, y in zip(new.arrays, old.arrays))
    assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(new.frames, old.frames))
    assert new.score == old.score and new.omitted == old.omitted and new.object_pages == old.object_pages
    for a, b in zip(new.columns[:2], old.columns[:2]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(new.columns[2], old.columns[2])
    for p in range(len(old)):
        assert [s.char for s in new.results[p][0]] == [s.char for s in old.results[p][0]]
        assert np.array_equal(new.results[p][0].boxes, old.results[p][0].boxes)


def test_without_the_switch_the_result_is_what_it_was(run):
    from text_alignment_amd import forced
    old = run["plain"]
    new = forced.refine_pages(run["pages"], run["trs"], run["rec"], PARAMS, AGREE, confidence=False)
    _same(new, old)
    for res in (old, new):
        assert res.confidence is None and res.rival is None and res.char_confidence is None
        assert res.syllable_confidence is None


def test_with_the_switch_results_frames_and_scores_stay(run):
    _same(run["conf"], run["plain"])
    assert run["conf"].refined.any()


def test_line_confidences_equal_the_checker_on_the_runs_own_probabilities(run):
    from text_alignment_amd import train
    res, om = run["conf"], run["om"]
    P = res.probs.cpu().numpy()
    seen = 0
    for q, ln in enumerate(res.harvest.lines):
        if res.frames[q] is None:
            assert res.confidence[q] is None and res.rival[q] is None
            continue
        Pq = P[int(res.row_off[q]):int(res.row_off[q]) + int(res.T[q])]
        G = R.tables(Pq, train.encode_text(om.codec, ln.text))[2]
        conf, rival, own = R.query_tables(G, res.frames[q][:, 2])
        assert res.confidence[q].dtype == np.int64 and res.rival[q].dtype == np.int32
        assert np.array_equal(res.confidence[q], conf) and np.array_equal(res.rival[q], rival)
        assert (own == res.score[q]).all() and (conf >= 0).all()
        seen += len(conf)
    assert seen > 0 and len(res.confidence) == len(res.frames) == len(res.rival)


def test_character_and_syllable_confidences_equal_a_restatement(run):
    from text_alignment_amd import forced, latinSyllabification as latsyl, page_batch as pb
    res, trs = run["conf"], run["trs"]
    h = res.harvest
    assert forced.NO_CONFIDENCE == -2 ** 63 and res.object_pages == []
    with_value = without = 0
    for p in range(4):
        want = {}                                        # transcript character -> confidence, the refined lines' kept ones
        for q in range(int(h.line_first[p]), int(h.line_first[p + 1])):
            if res.refined[q]:
                for k, c in enumerate(res.confidence[q].tolist()):
                    want[int(h.table[q][1]) + k] = c
        cc = res.char_confidence[p]
        assert cc.dtype == np.int64 and len(cc) == len(trs[p])
        assert cc.tolist() == [want.get(i, forced.NO_CONFIDENCE) for i in range(len(trs[p]))]
        first, last = pb.syllable_spans(trs[p], latsyl.syllabify_text(trs[p]))
        per_syl = res.syllable_confidence[p]
        assert len(per_syl) == len(res.results[p][0]) == len(res.indices[p])
        for got, k in zip(per_syl, res.indices[p]):
            have = [want[i] for i in range(int(first[k]), int(last[k]) + 1) if i in want]
            assert got == (min(have) if have else None)
            with_value += got is not None
            without += got is None
    assert with_value > 0


def test_confidence_is_refused_with_omit_and_at_page_scope(run):
    from text_alignment_amd import forced
    for over in (dict(omit=2.0), dict(scope="page"), dict(omit=0)):
        with pytest.raises(ValueError):
            forced.refine_pages(run["pages"], run["trs"], run["rec"], PARAMS, AGREE, confidence=True, **over)


def test_rforced_with_confidence_writes_a_row_per_character(tmp_path, capsys):
    """tools/rforced.py --confidence in process: NAME.conf beside NAME.llocs, a row per character with its confidence in
    bits and its rival's character; the summary names the lowest value; --omit and --page are argparse errors with it"""
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
    written = rforced.main([str(tmp_path), "-m", path, "--confidence"])
    io = capsys.readouterr()
    want, conf = forced.align_lines(path, strips, texts, confidence=True)
    lowest = min(int(c[:, 0].min()) for c in conf)
    for (out, score), (chars, sc), c, tx in zip(written, want, conf, texts):
        rows = [r.split("\t") for r in open(out, encoding="utf-8").read().split("\n")[:-1]]
        assert score == sc and [r[0] for r in rows] == list(tx) and [r[1] for r in rows] == ["%.1f" % e[4] for e in chars]
        rows = [r.split("\t") for r in open(out[:-len(".llocs")] + ".conf", encoding="utf-8").read().split("\n")[:-1]]
        assert [r[0] for r in rows] == list(tx)
        assert [r[1] for r in rows] == ["%.3f" % (int(v) / 65536.0) for v in c[:, 0]]
        assert [r[2] for r in rows] == [tx[(int(s) - 1) // 2] if int(s) % 2 else "~" for s in c[:, 1]]
    assert "2 of 2 lines written, lowest confidence %.3f bits" % (lowest / 65536.0) in io.out
    for extra in (["--omit", "0.5"], ["--page", path]):
        with pytest.raises(SystemExit) as e:
            rforced.main([str(tmp_path), "-m", path, "--confidence"] + extra)
        assert e.value.code == 2
    capsys.readouterr()
