"""forced.refine_pages(omit=...) end to end on the GPU: the four synthetic pages and the seeded model of
tests/test_refine_page_gpu.py, each page's transcript built from its own OCR text with three letters its longest line does
not hold inserted in front of one of that line's words.  With `omit` the refined lines' frames, scores and omitted counts must equal the checker tests/forced_omit_ref.py
on the run's own downloaded probabilities, the boxes the per-character rule with the omitted characters having none,
and the letters next to the inserted ones must keep the peaks they have when the insertion is not in the transcript.
Without `omit` everything is what it was."""
import numpy as np
import pytest

import forced_omit_ref as R
import forced_ref as FR
from test_forced_gpu import _line_texts, _model, _second_transcript
from test_forced_omit import _char_boxes_with_gaps

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEEDS = (70, 71, 72, 73)
PARAMS = [8, -12, -6, -6, -2, -2]
AGREE = (4, 5)
# bits: a factor 16 in probability.  Keeping a character the line shows costs next to nothing (the transcripts are built
# from the lines' own decodes, whose characters are the best class of their frames); a frame in a letter the line does
# not hold costs the distance from the frame's best class down to a class the model sees nowhere on the line.
OMIT = 4.0


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
    word = [b[1] for b in built]
    # the extra letters alone, without the space _second_transcript puts behind them: three letters the line does not
    # hold, in front of a word of its text -- nothing of the insertion can pass for something the page shows
    trs = [b[0][:hi + 1] + b[0][hi + 2:] for b, (lo, hi) in zip(built, word)]
    base = [tr[:lo] + tr[hi + 1:] for tr, (lo, hi) in zip(trs, word)]      # the same transcript without them
    strict = forced.refine_pages(pages, trs, rec, PARAMS, AGREE)
    with_word = forced.refine_pages(pages, trs, rec, PARAMS, AGREE, omit=OMIT)
    without = forced.refine_pages(pages, base, rec, PARAMS, AGREE, omit=OMIT)
    return {"om": om, "rec": rec, "pages": pages, "trs": trs, "word": word, "base": base, "strict": strict,
            "with": with_word, "without": without}


def test_omit_none_is_what_refine_pages_was(run):
    from text_alignment_amd import forced
    old = run["strict"]
    new = forced.refine_pages(run["pages"], run["trs"], run["rec"], PARAMS, AGREE, omit=None)
    assert new.page_scope is None and np.array_equal(new.refined, old.refined) and new.indices == old.indices
    assert all(np.array_equal(x, y) for x, y in zip(new.arrays, old.arrays))
    assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(new.frames, old.frames))
    assert new.score == old.score and new.omitted == old.omitted
    for a, b in zip(new.columns[:2], old.columns[:2]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(new.columns[2], old.columns[2])
    for p in range(4):
        assert [s.char for s in new.results[p][0]] == [s.char for s in old.results[p][0]]
        assert np.array_equal(new.results[p][0].boxes, old.results[p][0].boxes)
    # the strict lattice omits nothing: a count of 0 per aligned line, its frames all set
    assert old.refined.any()
    for q in range(len(old.refined)):
        assert (old.omitted[q] is None) == (old.frames[q] is None)
        if old.frames[q] is not None:
            assert old.omitted[q] == 0 and (old.frames[q] >= 0).all()


def test_with_omit_frames_boxes_and_counts_equal_the_checkers(run):
    from text_alignment_amd import forced, latinSyllabification as latsyl, ocr, page_batch as pb, train
    res, om, trs = run["with"], run["om"], run["trs"]
    h = res.harvest
    P = res.probs.cpu().numpy()
    omit_q = forced.omit_units(OMIT)
    assert res.refined.any() and res.object_pages == []
    harvest_ref = __import__("harvest_ref")
    total_gone = 0
    for p in range(4):
        refined = {}
        for q in range(int(h.line_first[p]), int(h.line_first[p + 1])):
            ln = h.lines[q]
            if ln.reason != 0:
                assert res.frames[q] is None and res.score[q] is None and res.omitted[q] is None and not res.refined[q]
                continue
            # ---- frames, score and count: the checker on the probabilities of this very run
            Pq = P[int(res.row_off[q]):int(res.row_off[q]) + int(res.T[q])]
            score, frames, _ = R.align_closed(Pq, train.encode_text(om.codec, ln.text), omit_q)
            assert np.array_equal(res.frames[q], frames) and res.score[q] == score
            gone = frames[:, 0] == R.OMITTED
            assert res.omitted[q] == int(gone.sum()) and bool(res.refined[q]) == bool((~gone).any())
            total_gone += int(gone.sum())
            if not res.refined[q]:
                continue
            # ---- boxes: peak_boxes over the PRESENT characters' peaks, none for an omitted one
            s = ln.source
            new = FR.peak_boxes(frames[~gone, 2], int(res.T[q]), s.width, s.offset_x, s.offset_y, s.offset_y + s.height, ocr.PAD)
            per_char, it = [], iter(new)
            for g in gone:
                per_char.append(None if g else next(it))
            refined[q] = (int(h.table[q][1]), int(h.table[q][2]), per_char)
            # the line's columns: its kept characters in place, a pair column with that box or a transcript character alone
            ops, idx, boxes = res.columns[0][p], res.columns[1][p], res.columns[2]
            got, j = [], 0
            for op in ops:
                if op == 0:
                    got.append(tuple(int(v) for v in boxes[idx[j]]))
                elif op == 1:
                    got.append(None)
                j += op != 1
            a = int(h.table[q][1])
            assert got[a:a + len(per_char)] == per_char
        # ---- the syllables' boxes: the per-character rule on the run's own harvest table, columns and frames
        tra, oc = harvest_ref.aligned_from_ops(h.ops[p].tolist(), list(trs[p]), list(h.ocr[p]))
        chars = res.results[p][3]
        cb = _char_boxes_with_gaps(tra, oc, h.o_line[p].tolist(), [tuple(int(v) for v in b) for b in chars.boxes], refined)
        syls = latsyl.syllabify_text(trs[p])
        named = [s for s in syls if len(s) >= 1]
        first, last = pb.syllable_spans(trs[p], syls)
        want = {k: FR.syllable_box(cb, int(a), int(b)) for k, (a, b) in enumerate(zip(first, last))}
        have = {k: b for k, b in want.items() if b is not None}
        assert res.indices[p] == sorted(have)
        assert [tuple(r) for r in res.arrays[p].tolist()] == [have[k] for k in sorted(have)]
        assert [s.char for s in res.results[p][0]] == [named[k] for k in sorted(have)]
    assert total_gone > 0


def test_the_neighbours_of_the_extra_word_keep_their_peaks(run):
    """the letter in front of the extra word and the one behind it: with the word in the transcript and omission allowed
    their frames are those of the run whose transcript does not hold the word"""
    a_run, b_run = run["without"], run["with"]
    seen = 0
    for p, (lo, hi) in enumerate(run["word"]):
        hb, ha = b_run.harvest, a_run.harvest
        for q in range(int(hb.line_first[p]), int(hb.line_first[p + 1])):
            t0, L = int(hb.table[q][1]), int(hb.table[q][2])
            if not (b_run.refined[q] and a_run.refined[q] and t0 <= lo and hi < t0 + L):
                continue
            tr_b, tr_a = run["trs"][p], run["base"][p]
            ta0, La = int(ha.table[q][1]), int(ha.table[q][2])
            before = lo - 1                              # positions in the transcript WITH the word
            while before >= 0 and tr_b[before] == " ":
                before -= 1
            after = hi + 1
            while after < len(tr_b) and tr_b[after] == " ":
                after += 1
            for x_b, x_a in ((before, before), (after, after - (hi - lo + 1))):
                if t0 <= x_b < t0 + L and ta0 <= x_a < ta0 + La:
                    assert tr_b[x_b] == tr_a[x_a] != " "
                    fb, fa = b_run.frames[q][x_b - t0].tolist(), a_run.frames[q][x_a - ta0].tolist()
                    print("page %d line %d: '%s' with the word %s, without %s" % (p, q, tr_b[x_b], fb, fa))
                    assert fb[2] == fa[2]
                    seen += 1
    assert seen >= 4


def test_process_passes_omit_through_and_page_scope_refuses_it(run):
    from text_alignment_amd import alignToOCR as atocr, forced
    pages, trs, rec, res = run["pages"], run["trs"], run["rec"], run["with"]
    one = forced.refine_pages(pages[1:2], trs[1:2], rec, PARAMS, AGREE, omit=OMIT)
    single = atocr.process(pages[1], trs[1], rec, PARAMS, refine=True, min_agreement=AGREE, omit=OMIT)
    assert np.array_equal(single[0].boxes, one.results[0][0].boxes) and single[0].chars == one.results[0][0].chars
    assert np.array_equal(single[0].boxes, res.results[1][0].boxes) and single[0].chars == res.results[1][0].chars
    with pytest.raises(ValueError, match="page scope has no omission"):
        forced.refine_pages(pages[:1], trs[:1], rec, PARAMS, scope="page", omit=OMIT)
    with pytest.raises(ValueError):
        forced.refine_pages(pages[:1], trs[:1], rec, PARAMS, AGREE, omit=-1.0)
    with pytest.raises(ValueError):
        atocr.process(pages[1], trs[1], rec, PARAMS, refine=False, omit=OMIT)
    with pytest.raises(TypeError):
        atocr.process_batch(pages[:1], trs[:1], rec, PARAMS, refine=True, omit=OMIT)
