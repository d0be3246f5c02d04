"""The harvest kernels (csrc/ta_harvest.hip) on the GPU, through harvest.harvest_alignment, against the plain-Python
checker tests/harvest_ref.py: batches built from host id arrays (tests/harvest_cases.py), aligned by the GPU aligner on
both of its paths; every output is an integer and is compared for equality.  Then harvest_pages and
LineTrainer.train_from_pages end to end on two small synthetic pages."""
import numpy as np
import pytest

import harvest_cases as C
import harvest_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = 0xEE


def _aligned_batch(pages, params, two_phase):
    """the pages through the aligner; the region in front of each right-aligned alignment poisoned afterwards"""
    from text_alignment_amd import textSeqCompare as tsc
    batch = tsc.NWBatch([pg["t"] for pg in pages], [pg["o"] for pg in pages], params, two_phase=two_phase)
    batch.run()
    ops = batch.results()
    mask = np.zeros(batch.ops.numel(), dtype=bool)
    for k, o in enumerate(ops):
        mask[int(batch.ops_off_host[k]):int(batch.ops_off_host[k] + batch.cap_host[k]) - len(o)] = True
    batch.ops[torch.from_numpy(mask).to(batch.ops.device)] = POISON
    return batch, ops


@pytest.fixture(scope="module")
def batches():
    """(pages, batch, alignment columns, assembled arrays, the checker's results) per (kind, aligner path): computed once"""
    out = {}
    for kind, pages, params in (("sized", C.sized_pages(), C.STIFF), ("random", C.random_pages(), C.DEFAULT)):
        for two_phase in (False, True):
            batch, ops = _aligned_batch(pages, params, two_phase)
            asm = C.assemble(pages, ops)
            out[kind, two_phase] = (pages, batch, ops, asm, C.expected(asm))
    return out


def _harvest(batch, asm, o_line=None, ratio=(C.NUM, C.DEN)):
    from text_alignment_amd import harvest
    return harvest.harvest_alignment(batch, asm["o_line"] if o_line is None else o_line, asm["line_first"], asm["t_class"],
                                     asm["T"], ratio, host=True, _fill=POISON)


@pytest.mark.parametrize("two_phase", [False, True])
@pytest.mark.parametrize("kind", ["sized", "random"])
def test_kernel_equals_the_checker(batches, kind, two_phase):
    """every row, every status word and the packed accepted lines; the outputs and the workspace were poisoned before the
    call and the two batches have different offsets"""
    from text_alignment_amd import train
    pages, batch, ops, asm, (want_table, refused, want_pack) = batches[kind, two_phase]
    if kind == "sized":
        cols = [len(o) for o in ops]
        assert cols[:len(C.SIZES)] == list(C.SIZES)                   # 0, 1 and the chunk edges, ~700
        shapes = pages[len(C.SIZES):]
        assert shapes[0]["lines"] == 1 and shapes[1]["lines"] == 5 and 2 not in shapes[1]["o_line"]
        assert set(ops[len(C.SIZES) + 2][:6]) == {1} and set(ops[len(C.SIZES) + 2][-6:]) == {1}     # seams at both page ends
        assert set(ops[-2]) == {1} and set(ops[-1]) == {2}
    got = _harvest(batch, asm)
    assert not any(refused) and (got["status"] == 0).all()
    assert np.array_equal(got["table"], want_table)
    acc_line, L, lab_off, labels = want_pack
    assert got["count"].tolist() == [len(acc_line), len(labels)]
    assert got["acc_line"].tolist() == acc_line and got["L"].tolist() == L
    assert got["lab_off"].tolist() == lab_off and got["labels"].tolist() == labels
    # ... which are train.encode_text of the checker's accepted texts
    first = asm["line_first"]
    encoded = []
    for p, pg in enumerate(pages):
        codec = train.make_codec(pg["charset"])
        for l in range(int(first[p]), int(first[p + 1])):
            r = want_table[l]
            if r[0] == 0:
                encoded.append(train.encode_text(codec, "".join(C.LETTERS[i] for i in pg["t"][r[1]:r[1] + r[2]])))
    assert [len(e) for e in encoded] == got["L"].tolist() and [c for e in encoded for c in e] == got["labels"].tolist()
    assert len(acc_line) > 0 and len(acc_line) < len(want_table)
    if kind == "random":
        assert len({int(r) for r in want_table[:, 0]}) > 6           # many different reason sets were reached


def test_another_threshold_and_device_inputs(batches):
    """agreement 1/1 and 1/3, with o_line / t_class / T handed over as device tensors"""
    from text_alignment_amd import harvest
    pages, batch, ops, asm, _ = batches["random", False]
    dev = batch.device
    for ratio in ((1, 1), (1, 3)):
        want_table, _, want_pack = C.expected(asm, *ratio)
        got = harvest.harvest_alignment(batch, torch.from_numpy(asm["o_line"]).to(dev), asm["line_first"],
                                        torch.from_numpy(asm["t_class"]).to(dev), torch.from_numpy(asm["T"]).to(dev),
                                        ratio, _fill=POISON).host()
        assert np.array_equal(got["table"], want_table)
        assert (got["acc_line"].tolist(), got["L"].tolist(), got["lab_off"].tolist(), got["labels"].tolist()) == tuple(want_pack)


def test_pages_are_refused_through_their_data_and_their_neighbours_are_not(batches):
    """an ops_len of -1, a decreasing o_line, a line index outside the page: PAGE on that page's lines, a status word, and
    every other page's rows equal to the checker's"""
    pages, batch, ops, asm, _ = batches["random", True]
    first = asm["line_first"]
    o_first = np.concatenate([[0], np.cumsum([len(pg["o"]) for pg in pages])])
    a, b = [p for p, pg in enumerate(pages) if p > 0 and len(pg["o"]) >= 4 and pg["lines"] >= 2][:2]
    o_line = asm["o_line"].copy()
    o_line[o_first[a]] = first[a] + 1                                 # the page's second line, then its first
    o_line[o_first[a] + 1:o_first[a + 1]] = first[a]
    o_line[o_first[b] + 2] = first[b + 1]                             # the first line of the NEXT page
    ref = [dict(pg) for pg in asm["ref"]]
    ref[0]["unfinished"] = True
    for p in (a, b):
        ref[p]["o_line"] = o_line[o_first[p]:o_first[p + 1]].tolist()
    want_table, refused = R.harvest_batch(ref, asm["T"].tolist(), C.NUM, C.DEN)
    assert [p for p, r in enumerate(refused) if r] == [0, a, b]
    saved = batch.ops_len.clone()
    try:
        batch.ops_len[0] = -1
        got = _harvest(batch, asm, o_line=o_line)
    finally:
        batch.ops_len.copy_(saved)
    assert np.array_equal(got["table"], want_table)
    assert got["status"].tolist() == [1 if p == 0 else (3 if p in (a, b) else 0) for p in range(len(pages))]
    for p in (0, a, b):
        assert (got["table"][first[p]:first[p + 1]] == [R.PAGE, 0, 0, 0, 0, 0, 0, 0]).all()
    acc_line, L, lab_off, labels = R.pack(want_table, ref)
    assert got["acc_line"].tolist() == acc_line and got["labels"].tolist() == labels and got["lab_off"].tolist() == lab_off


def test_host_side_refusals_raise_before_anything_is_launched(batches):
    from text_alignment_amd import _native, harvest
    pages, batch, ops, asm, _ = batches["sized", False]
    for bad in ((6, 5), 0, 1.01, (1, 10 ** 6 + 1)):
        with pytest.raises(ValueError):
            harvest.harvest_alignment(batch, asm["o_line"], asm["line_first"], asm["t_class"], asm["T"], bad)
    with pytest.raises(ValueError):
        harvest.harvest_alignment(batch, asm["o_line"], asm["line_first"][:-1], asm["t_class"], asm["T"])
    with pytest.raises(ValueError):
        harvest.harvest_alignment(batch, asm["o_line"][:-1], asm["line_first"], asm["t_class"], asm["T"])
    with pytest.raises(ValueError):
        harvest.harvest_alignment(batch, asm["o_line"], asm["line_first"][::-1].copy(), asm["t_class"], asm["T"])
    # the library itself, with real device pointers: TA_EINVAL / TA_ELIMIT and not one word of the outputs touched
    lib = _native.lib
    dev = batch.device
    nprob, nlines = batch.nprob, int(asm["line_first"][-1])
    t_off = np.concatenate([[0], np.cumsum(batch.n)]).astype(np.int64)
    o_off = np.concatenate([[0], np.cumsum(batch.m)]).astype(np.int64)
    lf = asm["line_first"].astype(np.int64)
    d_ol, d_cls, d_T, d_lf = (torch.from_numpy(a).to(dev) for a in (asm["o_line"], asm["t_class"], asm["T"], lf))
    ws = torch.full((int(lib.ta_harvest_workspace_bytes(nlines, int(t_off[-1]), int(o_off[-1]))),), POISON, dtype=torch.uint8, device=dev)
    table = torch.full((nlines, R.FIELDS), -7, dtype=torch.int32, device=dev)
    status = torch.full((nprob,), -7, dtype=torch.int32, device=dev)

    def call(num=4, den=5, t_off=t_off, lf=lf, ws_bytes=ws.numel(), nlines=nlines):
        return lib.ta_harvest_lines(
            batch.ops.data_ptr(), batch.ops_off.data_ptr(), batch.ops_len.data_ptr(), batch.ops.numel(),
            batch.t_codes.data_ptr(), batch.t_off.data_ptr(), batch.o_codes.data_ptr(), batch.o_off.data_ptr(), nprob,
            d_ol.data_ptr(), d_lf.data_ptr(), d_cls.data_ptr(), d_T.data_ptr(), nlines, num, den, t_off.ctypes.data,
            o_off.ctypes.data, lf.ctypes.data, ws.data_ptr(), ws_bytes, table.data_ptr(), status.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream)
    big = t_off.copy()
    big[-1] += 1 << 25
    for rc, want in ((call(num=0), _native.TA_EINVAL), (call(num=6), _native.TA_EINVAL), (call(ws_bytes=64), _native.TA_EINVAL),
                     (call(t_off=t_off[::-1].copy()), _native.TA_EINVAL), (call(nlines=nlines + 1), _native.TA_EINVAL),
                     (call(t_off=big), _native.TA_ELIMIT)):
        assert rc == want
    with pytest.raises(_native.NativeArgumentError):
        _native.check(call(den=0), "ta_harvest_lines")
    with pytest.raises(RuntimeError):
        _native.check(call(t_off=big), "ta_harvest_lines")
    torch.cuda.synchronize()
    assert bool((table == -7).all()) and bool((status == -7).all()) and bool((ws == POISON).all())
    assert call() == 0                                                # the same call with good arguments runs
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy(), batches["sized", False][4][0])


def test_harvest_pages_and_train_from_pages_end_to_end():
    """two small synthetic pages, a fresh (untrained) model whose OCR is noise: every line's row equals the checker's row
    computed from the alignment columns and line indices process_batch's own stages produced -- whatever those are; the
    assertion is equality with the checker, not an acceptance rate -- and train_from_pages returns the same result and
    trains on exactly the accepted lines"""
    from oracle import ocr_ref_f64 as OR
    from test_page_gpu import VOCAB, _page
    from text_alignment_amd import harvest, page as page_mod, train
    charset = "".join(VOCAB) + " "
    built = [_page(70 + k, 3 + k, OR, page_mod) for k in range(2)]
    pages, trs = [b[0] for b in built], [b[1] for b in built]
    params = [8, -1, -9, -9, -4, -4]
    trainer = train.LineTrainer(charset=charset, seed=3)
    res = harvest.harvest_pages(pages, trs, trainer.model(), params, min_agreement=0.8)
    assert len(res) == 7 and [(ln.page, ln.line) for ln in res.lines] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (1, 3)]
    assert res.line_first.tolist() == [0, 3, 7] and (res.status == 0).all()
    rows = []
    for p in range(2):
        tra, ocr = R.aligned_from_ops(res.ops[p].tolist(), list(trs[p]), list(res.ocr[p]))
        got = R.harvest_page(tra, ocr, res.o_line[p].tolist(), int(res.line_first[p]), int(res.line_first[p + 1]),
                             train.encode_text(trainer.codec, trs[p]), res.T.tolist(), 4, 5)
        rows.extend(got[l] for l in range(int(res.line_first[p]), int(res.line_first[p + 1])))
    assert res.table.tolist() == rows
    for ln, r in zip(res.lines, rows):
        assert ln.reason == r[0] and ln.counts == dict(zip(("equal", "unequal", "interior", "op2", "seam"), r[3:]))
        assert ln.text == (trs[ln.page][r[1]:r[1] + r[2]] if r[2] else None)
        assert ln.strip is pages[ln.page].strips[ln.line].prepared
    accepted = list(res.accepted())
    assert [t for _, t in accepted] == [ln.text for ln in res.lines if ln.reason == 0]
    print("end to end: %d of %d lines accepted; reasons %s" % (len(accepted), len(res), [ln.reasons() for ln in res.lines]))
    again = trainer.train_from_pages(pages, trs, params, min_agreement=(4, 5))
    assert again.table.tolist() == rows and trainer.lines_seen == len(accepted) == len(again.trained)
    # a scoring system the integer aligner refuses is a ValueError, as in the sweep
    with pytest.raises(ValueError):
        harvest.harvest_pages(pages, trs, trainer.model(), [8.5, -1, -9, -9, -4, -4])
    with pytest.raises(ValueError):
        harvest.harvest_pages(pages, trs, trainer.model(), params, min_agreement=1.5)
