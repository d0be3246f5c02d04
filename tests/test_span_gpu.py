"""The span search on the GPU: every (i0, i1, score) the kernel gives equals the checker tests/span_ref.py -- strip, group
and LDS edges, ties everywhere (2 letters) and few (25), planted and absent spans, all six scoring systems per batch and
per problem, a shared transcript, poisoned outputs -- then the aligner on the located spans against the CPU aligner, and
the `locate` switch of the page pipeline end to end."""
import numpy as np
import pytest

import span_cases as C
import span_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NS = (0, 1, 63, 64, 65, 255, 256, 257, 513, 2100)       # 2100 > 8 * 64 * 4 rows: a wave's second strip, the row re-used
MS = (0, 1, 2, 63, 64, 65, 300)
_cases, _refs = {}, {}


def _problems(alphabet):
    """all NS x MS shapes: spans planted at the head, in the middle and at the tail (a few substitutions), and absent"""
    if alphabet not in _cases:
        rng = np.random.RandomState(900 + alphabet)
        out = []
        for k, (n, m) in enumerate((n, m) for n in NS for m in MS):
            t = rng.randint(0, alphabet, size=n).astype(np.int32)
            o = rng.randint(0, alphabet, size=m).astype(np.int32)
            kind = k % 4
            if n > m + 10 and m > 0 and kind < 3:
                a = (0, (n - m) // 2, n - m)[kind]
                o = t[a:a + m].copy()
                o[rng.randint(0, m, size=m // 8)] = rng.randint(0, alphabet)
            out.append((t, o))
        _cases[alphabet] = out
    return _cases[alphabet]


def _ref(alphabet, k, system):
    key = (alphabet, k, tuple(system))
    if key not in _refs:
        t, o = _problems(alphabet)[k]
        _refs[key] = R.span_numpy(t, o, system)
    return _refs[key]


def _run(t_list, o_list, params):
    from text_alignment_amd import textSeqCompare as tsc
    batch = tsc.SpanBatch(t_list, o_list, params)
    assert batch.cells < 1e7
    batch.out.fill_(-77)                                  # poison: every word of the result is the kernel's
    batch.run()
    batch.fetch_begin()
    got = batch.results()
    assert got.shape == (len(t_list), 3) and got.dtype == np.int32
    return [tuple(int(v) for v in row) for row in got], batch


@pytest.mark.parametrize("alphabet", [2, 25])
@pytest.mark.parametrize("sys_k", range(len(C.SYSTEMS)))
def test_one_system_per_batch(alphabet, sys_k):
    probs = _problems(alphabet)
    picks = [(k % len(NS)) * len(MS) + (k + sys_k) % len(MS) for k in range(24)]      # every n, every m
    assert {p // len(MS) for p in picks} == set(range(len(NS))) and {p % len(MS) for p in picks} == set(range(len(MS)))
    got, _ = _run([probs[p][0] for p in picks], [probs[p][1] for p in picks], C.SYSTEMS[sys_k])
    want = [_ref(alphabet, p, C.SYSTEMS[sys_k]) for p in picks]
    assert got == want


@pytest.mark.parametrize("alphabet", [2, 25])
def test_one_system_per_problem_every_shape(alphabet):
    probs = _problems(alphabet)
    systems = [C.SYSTEMS[(k + k // len(MS)) % len(C.SYSTEMS)] for k in range(len(probs))]
    got, _ = _run([p[0] for p in probs], [p[1] for p in probs], systems)
    want = [_ref(alphabet, k, s) for k, s in enumerate(systems)]
    assert got == want
    planted = [k for k, (t, o) in enumerate(probs) if len(t) > len(o) + 10 and len(o) >= 63 and k % 4 < 3]
    assert len(planted) >= 8                              # the batch does hold planted spans of every kind


def test_widest_ocr_string_and_one_beyond():
    from text_alignment_amd import _native, textSeqCompare as tsc
    big = _native.lib.ta_nw_span_max_m()
    rng = np.random.RandomState(11)
    o = rng.randint(0, 25, size=big).astype(np.int32)
    t = np.concatenate([rng.randint(0, 25, size=30), o[100:160], rng.randint(0, 25, size=300)]).astype(np.int32)
    for system in (C.SYSTEMS[0], C.SYSTEMS[3]):
        got, _ = _run([t, t[:7]], [o, o[:50]], system)
        assert got == [R.span_numpy(t, o, system), R.span_numpy(t[:7], o[:50], system)]
    with pytest.raises(OverflowError):
        tsc.SpanBatch([t], [np.zeros(big + 1, np.int32)], C.SYSTEMS[0])
    with pytest.raises(OverflowError):
        tsc.SpanBatch([t], [o[:10]], [1 << 20, -1, -1, -1, -1, -1])
    with pytest.raises(OverflowError):
        tsc.SpanBatch([np.zeros(9000, np.int32)], [o[:4000]], [300, -300, -300, -300, -300, -300])   # score bound


def test_pages_of_one_book_share_its_upload():
    tr, _, _ = C.planted(77, 900, 200, 900, 0.8)
    rng = np.random.RandomState(3)
    ocrs, where = [], []
    for a in (0, 310, 777, len(tr) - 180):
        ocrs.append(C.noisy(rng, tr[a:a + 180], 0.8))
        where.append(a)
    coded = C.codes(tr, *ocrs)
    book = coded[0]
    other = book[:500].copy()
    got, batch = _run([book, book, other, book, book], [coded[1], coded[2], coded[2], coded[3], coded[4]], C.SYSTEMS[0])
    assert batch.uploaded_tokens == len(book) + len(other)
    assert batch.t_start.cpu().tolist() == [0, 0, len(book), 0, 0]
    want = [R.span_numpy(t, o, C.SYSTEMS[0]) for t, o in
            ((book, coded[1]), (book, coded[2]), (other, coded[2]), (book, coded[3]), (book, coded[4]))]
    assert got == want
    for (i0, i1, _), a in zip([got[0], got[1], got[3], got[4]], where):
        assert abs(i0 - a) <= 12 and abs(i1 - (a + 180)) <= 12          # and they are where the text was taken from


def test_located_spans_then_the_aligner_equal_the_cpu_aligner_on_the_spans():
    from oracle import nw_oracle
    from text_alignment_amd import textSeqCompare as tsc
    pairs = []
    for seed, (before, after) in enumerate([(0, 300), (250, 250), (400, 0)]):
        tr, ocr, _ = C.planted(40 + seed, before, 150, after, 0.75)
        pairs.append((list(tr), list(ocr)))
    pairs.append((list("alleluia alleluia"), list("")))
    book = pairs[1][0]
    pairs.append((book, pairs[1][1][20:90]))                # the same transcript OBJECT again
    for systems in (None, [10, -5, -7, -2], [C.SYSTEMS[k % 6] for k in range(len(pairs))]):
        spans = tsc.locate_spans(pairs, systems)
        per_pair = systems if isinstance(systems, list) and isinstance(systems[0], list) else [systems] * len(pairs)
        for (t, o), s, got in zip(pairs, per_pair, spans):
            tc, oc = (np.array([ord(c) for c in x], dtype=np.int32) for x in (t, o))
            assert got == R.span_numpy(tc, oc, tsc.parse_scoring_system(s)[0])
        assert tsc.locate_span(pairs[0][0], pairs[0][1], per_pair[0]) == spans[0]
        cut = [(t[i0:i1], o) for (t, o), (i0, i1, _) in zip(pairs, spans)]
        aligned = tsc.perform_alignment_batch(cut, systems)
        for (t, o), s, al in zip(cut, per_pair, aligned):
            want = nw_oracle.perform_alignment(t, o, s)
            assert (list(al[0]), list(al[1])) == (list(want[0]), list(want[1]))
    assert spans[3] == (0, 0, 0)


def _json(atocr, res):
    return atocr.to_JSON_dict(res[0], res[2])


def test_pages_locate_their_own_text_end_to_end():
    """synthetic pages, a fresh (untrained) model whose OCR is noise: nothing is asserted about accuracy -- the spans are
    the checker's on the pages' own OCR text, and everything behind them is the pipeline without the switch on the
    trimmed transcripts"""
    from oracle import ocr_ref_f64 as OR
    from test_page_gpu import VOCAB, _page
    from text_alignment_amd import alignToOCR as atocr, harvest, page as page_mod, train
    charset = "".join(VOCAB) + " "
    built = [_page(170 + k, 3 + k, OR, page_mod) for k in range(3)]
    pages, own = [b[0] for b in built], [b[1] for b in built]
    junk = " ".join(VOCAB[(7 * k) % len(VOCAB)] for k in range(40))
    book = " ".join(own)                                   # ONE string for pages 0 and 1: each finds its part
    trs = [book, book, junk + " " + own[2] + " " + junk, "     "]
    pages.append(_page(190, 2, OR, page_mod)[0])           # its transcript is spaces: an empty span
    params = [8, -1, -9, -9, -4, -4]
    model = train.LineTrainer(charset=charset, seed=3).model()

    spans, idx, arr = [], [], []
    res = atocr.process_batch(pages, trs, model, params, indices_out=idx, arrays_out=arr, locate=True, spans_out=spans)
    assert len(res) == len(spans) == len(arr) == 4
    for k, (tr, r) in enumerate(zip(trs, res)):
        ocr_text = "".join(c for c in r[3].chars)
        t, o = (np.array([ord(c) for c in x], dtype=np.int32) for x in (tr, ocr_text))
        i0, i1, _ = R.span_numpy(t, o, params)
        assert spans[k] == R.snap_to_words(tr, i0, i1), k
        a, b = spans[k]
        idx1, arr1 = [], []
        alone = atocr.process_batch([pages[k]], [tr[a:b]], model, params, indices_out=idx1, arrays_out=arr1)
        assert _json(atocr, r) == _json(atocr, alone[0]) and idx[k] == idx1[0] and np.array_equal(arr[k], arr1[0])
        s1 = []
        single = atocr.process(pages[k], tr, model, seq_align_params=params, locate=True, spans_out=s1)
        assert s1 == [spans[k]] and _json(atocr, single) == _json(atocr, r)
    assert spans[3][0] == spans[3][1] and len(res[3][0]) == 0 and len(arr[3]) == 0          # an empty span: no boxes
    print("spans", spans, "of transcripts of", [len(t) for t in trs], "characters; boxes", [len(a) for a in arr])

    hv = harvest.harvest_pages(pages, trs, model, params, min_agreement=0.8, locate=True)
    assert hv.spans == spans
    trimmed = [tr[a:b] for tr, (a, b) in zip(trs, spans)]
    plain = harvest.harvest_pages(pages, trimmed, model, params, min_agreement=0.8)
    assert hv.table.tolist() == plain.table.tolist() and plain.spans is None
    for ln, ref_ln in zip(hv.lines, plain.lines):
        assert ln.text == ref_ln.text and (ln.text is None or ln.text in trimmed[ln.page])

    # without the switch nothing changes: the argument's default is the old call
    a0, a1 = [], []
    r0 = atocr.process_batch(pages[:3], trimmed[:3], model, params, arrays_out=a0)
    r1 = atocr.process_batch(pages[:3], trimmed[:3], model, params, arrays_out=a1, locate=False, spans_out=[])
    assert [_json(atocr, x) for x in r0] == [_json(atocr, x) for x in r1] and all(np.array_equal(x, y) for x, y in zip(a0, a1))
    assert _json(atocr, atocr.process(pages[0], trimmed[0], model, seq_align_params=params, locate=False)) == _json(atocr, r0[0])
    for bad in ([lambda x, y: 1, -1, -1, -1, -1], [8.5, -1, -9, -9, -4, -4]):
        with pytest.raises(ValueError):
            atocr.process_batch(pages[:1], trs[:1], model, bad, locate=True)
        with pytest.raises(ValueError):
            atocr.process(pages[0], trs[0], model, seq_align_params=bad, locate=True)


def test_one_book_for_every_page_through_five_chunks_of_the_pipeline(monkeypatch):
    """locate=True through the chunk pipeline: nine pages of three lines, two recognisers in turn, ONE book string (the
    pages' own texts joined) as every page's transcript, chunks of two pages -- 1, 2, 2 pages of the first recogniser,
    2, 2 of the second: steady state and the drain.  Per page the span, JSON, indices and box array are those of the page
    alone against the book; a second call returns the same."""
    from oracle import ocr_ref_f64 as OR
    from test_page_gpu import VOCAB, _page
    from text_alignment_amd import alignToOCR as atocr, page as page_mod, train
    charset = "".join(VOCAB) + " "
    built = [_page(240 + k, 3, OR, page_mod) for k in range(9)]
    pages = [b[0] for b in built]
    book = " ".join(b[1] for b in built)
    trs = [book] * 9
    params = [8, -1, -9, -9, -4, -4]
    two = [train.LineTrainer(charset=charset, seed=3 + k).model() for k in range(2)]
    models = [two[k % 2] for k in range(9)]
    monkeypatch.setattr(atocr, "PIPELINE_CHUNK_PAGES", 2)
    chunks = []
    launch = atocr.PageChunk.launch
    monkeypatch.setattr(atocr.PageChunk, "launch",
                        lambda chunk, *a, **kw: (chunks.append(len(chunk.pages)), launch(chunk, *a, **kw))[1])

    def call():
        spans, idx, arr = [], [], []
        res = atocr.process_batch(pages, trs, models, params, locate=True, spans_out=spans, indices_out=idx, arrays_out=arr)
        return [_json(atocr, r) for r in res], spans, idx, arr
    got, spans, idx, arr = call()
    assert chunks == [1, 2, 2, 2, 2]
    again = call()
    assert again[:3] == (got, spans, idx) and all(np.array_equal(x, y) for x, y in zip(arr, again[3]))
    monkeypatch.undo()
    assert len(got) == len(spans) == len(idx) == len(arr) == 9
    for k in range(9):
        s1, i1, a1 = [], [], []
        alone = atocr.process_batch([pages[k]], [book], models[k], params, locate=True, spans_out=s1, indices_out=i1,
                                    arrays_out=a1)
        assert spans[k] == s1[0] and got[k] == _json(atocr, alone[0]) and idx[k] == i1[0] and np.array_equal(arr[k], a1[0]), k
    print("spans", spans, "in a book of", len(book), "characters; boxes", [len(a) for a in arr])
