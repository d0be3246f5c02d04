"""The forced-alignment kernel (csrc/ta_forced.hip) on the GPU against the checker tests/forced_ref.py: the cases of
tests/forced_cases.py through the library with real device pointers, then forced.align_lines and forced.refine_pages end
to end.  Every output is an integer and is compared for equality."""
import numpy as np
import pytest

import forced_cases as C
import forced_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class _Device(object):
    """a packed case's arrays on the device"""

    def __init__(self, pk):
        self.pk = pk
        self.t = {name: torch.from_numpy(getattr(pk, name)).cuda() for name in C.INPUTS + C.OUTPUTS + ("ws",)}

    def ptr(self, name):
        return self.t[name].data_ptr()

    def call(self, lib, **over):
        return C.call(lib, self.pk, self.ptr, torch.cuda.current_stream().cuda_stream, **over)

    def host(self, name):
        return self.t[name].cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    from text_alignment_amd import _native
    return _native.lib


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_kernel_equals_the_checker(lib, case):
    name, no, lines = case
    d = _Device(C.pack(lib, lines, no))
    assert d.call(lib) == 0
    frames, score = C.want(name, lines)
    assert d.host("status").tolist() == [R.OK] * len(lines)
    assert np.array_equal(C.gather(d.pk, d.host("frames")), frames)
    assert np.array_equal(d.host("score"), score)


def test_a_line_refused_through_its_data_leaves_its_neighbours_alone(lib):
    rng = np.random.default_rng(5)
    lines = [(C.probs(rng, 30, 6), C.text(rng, 7, 6)), (C.probs(rng, 21, 6), C.text(rng, 5, 6)),
             (C.probs(rng, 140, 6), C.text(rng, 66, 6))]
    frames, score = R.align_batch(lines)
    keep = np.r_[0:7, 12:78]
    for edit, status in ((dict(labels_edit={1: (2, 6)}), R.LABEL), (dict(L_dev={1: 11}), R.BOUNDS)):
        d = _Device(C.pack(lib, lines, 6, **edit))
        assert d.call(lib) == 0
        assert d.host("status").tolist() == [R.OK, status, R.OK]
        got = C.gather(d.pk, d.host("frames"))
        assert np.array_equal(got[keep], frames[keep]) and (got[7:12] == C.POISON32).all()
        sc = d.host("score")
        assert sc[1] == C.POISON64 and np.array_equal(sc[[0, 2]], score[[0, 2]])
    for name, k, v in (("row_off", 2, 10 ** 9), ("lab_off", 1, -1), ("ws_off", 0, 8), ("ws_off", 2, 10 ** 12)):
        pk = C.pack(lib, lines, 6)
        getattr(pk, name)[k] = v
        d = _Device(pk)
        assert d.call(lib) == 0
        want = [R.OK] * 3
        want[k] = R.BOUNDS
        assert d.host("status").tolist() == want, (name, v)


def test_host_side_refusals_touch_nothing_and_the_good_call_then_runs(lib):
    from text_alignment_amd import _native
    rng = np.random.default_rng(6)
    lines = [(C.probs(rng, 30, 6), C.text(rng, 7, 6)), (C.probs(rng, 21, 6), C.text(rng, 5, 6))]
    d = _Device(C.pack(lib, lines, 6))
    for what, code, over in C.refusals(d.pk):
        if over == "misalign":
            over = dict(workspace=d.ptr("ws") + 4)
        assert d.call(lib, **over) == code, what
    with pytest.raises(_native.NativeArgumentError):
        _native.check(d.call(lib, no=1), "ta_forced_align")
    torch.cuda.synchronize()
    assert (d.host("frames") == C.POISON32).all() and (d.host("score") == C.POISON64).all()
    assert (d.host("status") == C.POISON32).all() and (d.host("ws") == C.POISON_BYTE).all()
    assert d.call(lib) == 0
    assert d.host("status").tolist() == [0, 0]
    assert np.array_equal(C.gather(d.pk, d.host("frames")), R.align_batch(lines)[0])


def test_forced_alignment_python_call():
    """the device-level Python call: its own workspace layout, poisoned, labels from the host and from the device"""
    from text_alignment_amd import forced
    rng = np.random.default_rng(8)
    lines = [(C.probs(rng, T, 30), C.text(rng, L, 30)) for T, L in ((90, 30), (300, 70), (40, 1), (171, 85))]
    frames, score = R.align_batch(lines)
    T = [len(P) for P, _ in lines]
    L = [len(cs) for _, cs in lines]
    probs = torch.from_numpy(np.concatenate([P for P, _ in lines])).cuda()
    labels = np.concatenate([cs for _, cs in lines])
    row_off, lab_off = np.cumsum([0] + T[:-1]), np.cumsum([0] + L[:-1])
    got = forced.forced_alignment(probs, row_off, T, labels, lab_off, L, host=True, _fill=0xEE)
    assert got["status"].tolist() == [0] * 4 and np.array_equal(got["frames"], frames) and np.array_equal(got["score"], score)
    f2, s2, st2 = forced.forced_alignment(probs, row_off, T, torch.from_numpy(labels).cuda(), lab_off, L)
    assert np.array_equal(f2.cpu().numpy(), frames) and np.array_equal(s2.cpu().numpy(), score)
    for bad in (dict(T=[90, 300, 2, 171]), dict(L=[30, 70, 0, 85]), dict(L=[30, 70, 1, 86]), dict(row_off=[0, 90, 390, 600])):
        a = dict(row_off=row_off, T=T, lab_off=lab_off, L=L)
        a.update(bad)
        with pytest.raises(ValueError):
            forced.forced_alignment(probs, a["row_off"], a["T"], labels, a["lab_off"], a["L"])
    with pytest.raises(ValueError):
        forced.forced_alignment(probs.double(), row_off, T, labels, lab_off, L)


def test_align_lines_equals_the_checker_on_the_runs_own_probabilities():
    """~20 lines of a synthetic model: whatever its probabilities are, frames and scores equal the checker's on the
    probabilities downloaded from that very run; x is the .llocs position of t_peak"""
    from oracle import ocr_ref_f64 as OR
    from text_alignment_amd import forced, ocr
    om = OR.synthetic_model(7001, no=40)
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    rng = np.random.default_rng(12)
    lines = [OR.synthetic_line(5200 + k, width=60 + 17 * k) for k in range(20)]
    letters = [c for c in om.codec[1:] if c and c != "~"]
    texts = ["".join(rng.choice(letters, size=int(rng.integers(1, (len(xs) - 1) // 2 + 1)))) for xs in lines]
    texts[3] = "aab aa"
    got, run = forced.align_lines(rec, lines, texts, want_run=True)
    P = run["probs"].cpu().numpy()
    from text_alignment_amd import train
    for b, (xs, tx) in enumerate(zip(lines, texts)):
        T = len(xs)
        assert int(run["T"][b]) == T
        score, frames, _ = R.align(P[int(run["row_off"][b]):int(run["row_off"][b]) + T], train.encode_text(om.codec, tx))
        chars, sc = got[b]
        assert sc == score and [c[0] for c in chars] == list(tx)
        assert np.array_equal(np.asarray([c[1:4] for c in chars], dtype=np.int32), frames)
        assert [c[4] for c in chars] == R.peak_x(frames[:, 2], T, T - 2 * ocr.PAD, ocr.PAD).tolist()
    with pytest.raises(ValueError):
        forced.align_lines(rec, lines[:1], ["é"])
    with pytest.raises(ValueError):
        forced.align_lines(rec, lines[:1], ["a" * ((len(lines[0]) - 1) // 2 + 1)])


# ---- refine_pages end to end -------------------------------------------------------------------------------------------

def _model(OR):
    """a synthetic model that reads many different characters -- the output layer listens to the hidden state three times
    as hard, blanks are favoured (short runs) and spaces a little -- and letters and spaces only"""
    om = OR.synthetic_model(7001, no=40)
    om.W2[:, 1:] *= 3.0
    om.W2[0, 0] += 4.0
    om.W2[1, 0] += 2.0
    om.W2[2, 0] -= 30.0                                  # '~'
    om.W2[29:, 0] -= 30.0                                # punctuation and digits: characters a transcript does not hold
    return om


def _second_transcript(line_texts, latsyl):
    """a page's transcript built from its OWN OCR text, line by line: letters and spaces only, runs of spaces collapsed,
    the lines joined by a space -- and one extra word in the middle of the longest line, of letters that line does not
    have.  Returns (transcript, (first, last) positions of the inserted word's letters)."""
    clean = [" ".join("".join(ch if "a" <= ch <= "z" else " " for ch in tx).split()) for tx in line_texts]
    m = max(range(len(clean)), key=lambda k: len(clean[k]))
    absent = [ch for ch in "aeioubcdfghlmnprst" if ch not in clean[m]]
    word = (absent[0] + absent[-1] + absent[0]) if absent else "zzz"
    spaces = [i for i, ch in enumerate(clean[m]) if ch == " "]
    at = min(spaces, key=lambda i: abs(i - len(clean[m]) // 2)) + 1 if spaces else 0
    first = sum(len(c) + 1 for c in clean[:m]) + at
    clean[m] = clean[m][:at] + word + " " + clean[m][at:]
    return " ".join(clean), (first, first + len(word) - 1)


def _line_texts(chars_seq, page):
    """the OCR text of every line of a page, from process_batch's fourth element (a character's uly is its strip's)"""
    rows = {s.offset_y: k for k, s in enumerate(page.strips)}
    out = [""] * len(page.strips)
    for ch, box in zip(chars_seq.chars, chars_seq.boxes):
        out[rows[int(box[1])]] += ch
    return out


def _rule_syllable_boxes(res, p, transcript, syls):
    """the checker's syllable boxes of page p from the run's own harvest table, columns and frames: {syllable: box}"""
    from text_alignment_amd import ocr, page_batch as pb
    h = res.harvest
    tra, oc = __import__("harvest_ref").aligned_from_ops(h.ops[p].tolist(), list(transcript), list(h.ocr[p]))
    chars = res.results[p][3]
    refined = {}
    for q in range(int(h.line_first[p]), int(h.line_first[p + 1])):
        if res.refined[q]:
            s = h.lines[q].source
            new = R.peak_boxes(res.frames[q][:, 2], int(res.T[q]), s.width, s.offset_x, s.offset_y, s.offset_y + s.height, ocr.PAD)
            refined[q] = (int(h.table[q][1]), int(h.table[q][2]), new)
    cb = R.char_boxes(tra, oc, h.o_line[p].tolist(), [tuple(int(v) for v in b) for b in chars.boxes], refined)
    first, last = pb.syllable_spans(transcript, syls)
    return {k: R.syllable_box(cb, int(a), int(b)) for k, (a, b) in enumerate(zip(first, last))}, (first, last)


def test_refine_pages_end_to_end():
    """two small synthetic pages (3 and 4 lines) in two passes.  Pass one is process_batch; each page's transcript for
    pass two is built from its own OCR text with one extra word inside the longest line.  With the float64 restatement
    of the recogniser, the C aligner and tests/harvest_ref.py alone (seeds 70 / 71, min_agreement 4/5) all 7 of 7 lines
    are accepted and every inserted letter stands in an op-1 column."""
    from oracle import ocr_ref_f64 as OR
    from test_page_gpu import _page
    from text_alignment_amd import alignToOCR as atocr, forced, latinSyllabification as latsyl, ocr, page as page_mod, train
    om = _model(OR)
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    params = [8, -12, -6, -6, -2, -2]              # a mismatch costs more than a short gap: the extra word stays unpaired
    pages = [_page(70 + k, 3 + k, OR, page_mod)[0] for k in range(2)]
    one = atocr.process_batch(pages, ["amen"] * 2, rec, params)
    built = [_second_transcript(_line_texts(r[3], pg), latsyl) for r, pg in zip(one, pages)]
    trs = [b[0] for b in built]
    idx_plain, arr_plain = [], []
    plain = atocr.process_batch(pages, trs, rec, params, indices_out=idx_plain, arrays_out=arr_plain)
    res = forced.refine_pages(pages, trs, rec, params, min_agreement=(4, 5))
    nlines = 7
    assert len(res) == 2 and len(res.refined) == nlines and res.object_pages == [] and res.spans is None
    assert int(np.sum(res.refined)) * 2 >= nlines
    assert [bool(r) for r in res.refined] == [ln.reason == 0 for ln in res.harvest.lines]
    # frames and scores: the checker on the probabilities of this very run
    P = res.probs.cpu().numpy()
    for q in range(nlines):
        if res.refined[q]:
            ln = res.harvest.lines[q]
            score, frames, _ = R.align(P[int(res.row_off[q]):int(res.row_off[q]) + int(res.T[q])],
                                       train.encode_text(om.codec, ln.text))
            assert np.array_equal(res.frames[q], frames) and res.score[q] == score
        else:
            assert res.frames[q] is None and res.score[q] is None
    for p in range(2):
        syls = latsyl.syllabify_text(trs[p])
        named = [s for s in syls if len(s) >= 1]
        want, (first, last) = _rule_syllable_boxes(res, p, trs[p], syls)
        have = {k: b for k, b in want.items() if b is not None}
        # boxes: the per-character rule on the run's own harvest table, columns and frames (angle 0: no rotation)
        assert res.indices[p] == sorted(have)
        assert [tuple(r) for r in res.arrays[p].tolist()] == [have[k] for k in sorted(have)]
        assert [s.char for s in res.results[p][0]] == [named[k] for k in sorted(have)]
        # the page's OCR characters are what they were
        assert res.results[p][3].chars == plain[p][3].chars and np.array_equal(res.results[p][3].boxes, plain[p][3].boxes)
        # every syllable lying wholly on refined lines has a box
        h = res.harvest
        for q in range(int(h.line_first[p]), int(h.line_first[p + 1])):
            if res.refined[q]:
                a, b = int(h.table[q][1]), int(h.table[q][1]) + int(h.table[q][2])
                inside = [k for k in range(len(first)) if a <= first[k] and last[k] < b]
                assert inside and all(k in have for k in inside)
        # the inserted word: boxes under refinement, none without
        lo, hi = built[p][1]
        word = [k for k in range(len(first)) if lo <= first[k] and last[k] <= hi]
        assert word and all(k in have for k in word) and not any(k in idx_plain[p] for k in word)
    # one substituted character per line and full agreement demanded: refined nowhere, equal to process_batch exactly
    tr3 = trs[0]
    for q in range(3):
        r = res.harvest.table[q]
        at = int(r[1]) + int(r[2]) // 2
        while tr3[at] == " ":
            at += 1
        tr3 = tr3[:at] + ("x" if tr3[at] != "x" else "y") + tr3[at + 1:]
    idx3, arr3 = [], []
    plain3 = atocr.process_batch(pages[:1], [tr3], rec, params, indices_out=idx3, arrays_out=arr3)
    res3 = forced.refine_pages(pages[:1], [tr3], rec, params, min_agreement=(1, 1))
    assert not res3.refined.any() and res3.indices == idx3 and np.array_equal(res3.arrays[0], arr3[0])
    assert [s.char for s in res3.results[0][0]] == [s.char for s in plain3[0][0]]
    assert np.array_equal(res3.results[0][0].boxes, plain3[0][0].boxes)
    # process(..., refine=True): one page through refine_pages
    single = atocr.process(pages[1], trs[1], rec, params, refine=True, min_agreement=0.8)
    assert np.array_equal(single[0].boxes, res.results[1][0].boxes) and single[0].chars == res.results[1][0].chars
    with pytest.raises(ValueError):
        forced.refine_pages(pages, trs[:1], rec, params)
    with pytest.raises(ValueError):
        forced.refine_pages(pages, trs, rec, [8.5, -12, -6, -6, -2, -2])


def test_rforced_writes_llocs_for_line_images_with_known_texts(tmp_path):
    """tools/rforced.py in process: NAME.png + NAME.gt.txt -> NAME.llocs, one row per character of the text, the
    positions those of align_lines on the same raw strips (pixels of the line image); a text the model cannot take is
    skipped, not fatal"""
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
    strips = [_strip(rng, 40, 180), _strip(rng, 52, 260), _strip(rng, 40, 150)]
    texts = ["et in terra", "gloria patri", "café"]
    for k, (img, tx) in enumerate(zip(strips, texts)):
        Image.fromarray(img).save(str(tmp_path / ("l%d.png" % k)))
        (tmp_path / ("l%d.gt.txt" % k)).write_text(tx + "\n", encoding="utf-8")
    written = rforced.main([str(tmp_path), "-m", path])
    assert [w[0] for w in written] == [str(tmp_path / "l0.llocs"), str(tmp_path / "l1.llocs")]
    want = forced.align_lines(path, strips[:2], texts[:2])
    for (out, score), (chars, sc), tx, img in zip(written, want, texts, strips):
        rows = [r.split("\t") for r in open(out, encoding="utf-8").read().split("\n")[:-1]]
        assert [r[0] for r in rows] == list(tx) and score == sc
        assert [r[1] for r in rows] == ["%.1f" % c[4] for c in chars]
        xs = [c[4] for c in chars]
        assert xs == sorted(xs) and len(set(xs)) == len(xs)            # one peak per character, left to right
