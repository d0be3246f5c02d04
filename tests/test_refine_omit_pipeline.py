"""process_batch(..., line_omit=...) without a GPU: the refusals that stand in front of everything else, the host's
row scatter (forced.present_box_rows) on hand-made frames against refine_pages' construction, and the cut of a finished
chunk's `omitted` into pages."""
import numpy as np
import pytest


def test_the_refusals_come_before_a_recogniser_and_before_the_gpu(monkeypatch):
    from text_alignment_amd import alignToOCR as atocr
    monkeypatch.setattr(atocr, "_recognizer_for", lambda *a, **k: pytest.fail("a recogniser before the refusal"))
    monkeypatch.setattr(atocr.PageChunk, "launch", lambda *a, **k: pytest.fail("GPU work before the refusal"))
    call = lambda **kw: atocr.process_batch([], [], None, **kw)                                     # noqa: E731
    with pytest.raises(ValueError, match="refine=True"):
        call(line_omit=4.0)                              # a ValueError, not the TypeError of an unknown keyword
    with pytest.raises(ValueError, match="refine=True"):
        call(line_omit=4.0, refine=False)
    for scope in (dict(refine_scope="page"), dict(refine_scope="page", page_margin=3), dict(page_margin=3)):
        with pytest.raises(ValueError, match="line scope"):
            call(line_omit=4.0, refine=True, **scope)
    for more in (dict(confidence=True), dict(posterior=True), dict(confidence=True, posterior=True)):
        with pytest.raises(ValueError, match="strict lattice"):
            call(line_omit=4.0, refine=True, **more)
    for bad in (True, False, np.bool_(True), "4", [4.0], -0.5, 1024.5, float("nan"), float("inf"), 1 << 20):
        with pytest.raises(ValueError, match="omit"):
            call(line_omit=bad, refine=True)
        with pytest.raises(ValueError, match="omit"):
            call(line_omit=bad)
    # the names that are not the keyword stay what they were
    with pytest.raises(TypeError):
        call(omit=4.0, refine=True)


def _frames(masks, rng):
    """frames of slots with the given present masks: rising peaks for the present characters, -1 thrice for the others"""
    rows, T = [], []
    for here in masks:
        t = np.sort(rng.choice(np.arange(8, 8 + 3 * len(here)), size=len(here), replace=False)).astype(np.int32)
        fr = np.stack([t - 1, t + 1, t], axis=1)
        fr[~np.asarray(here)] = -1
        rows.append(fr)
        T.append(16 + 3 * len(here) + 16)
    return rows, np.asarray(T, np.int64)


def test_the_row_scatter_is_peak_boxes_over_the_present_characters():
    """omitted characters at the start, in the middle and at the end; a slot without a present character; a slot that was
    not aligned (its rows hold whatever they held); gaps between the slots' rows"""
    from text_alignment_amd import forced, ocr
    rng = np.random.default_rng(3)
    b = lambda s: np.asarray([c == "x" for c in s])                                                 # noqa: E731
    masks = [b("..xxx"), b("xx..xxx.x"), b("xxxx.."), b("...."), b("x"), b("."), b("xxxxx"), b(".x.x.x.")]
    per_slot, T = _frames(masks, rng)
    L = np.asarray([len(m) for m in masks], np.int64)
    lab_off = np.cumsum(L + 2) - L                       # two rows between the slots, two in front
    frames = np.full((int(lab_off[-1] + L[-1]) + 3, 3), 4242, np.int32)
    for o, fr in zip(lab_off, per_slot):
        frames[o:o + len(fr)] = fr
    done = np.ones(len(masks), bool)
    done[6] = False                                      # not aligned: every field "present", none may be used
    raw_w = 100 + 7 * np.arange(len(masks))
    x_min, y_min = 5 + np.arange(len(masks)), 11 * np.arange(len(masks))
    y_max = y_min + 30
    rows = forced.present_box_rows(frames, L, lab_off, T, raw_w, x_min, y_min, y_max, ocr.PAD, done=done)
    assert rows.shape == (len(frames), 4) and rows.dtype == np.int64
    used = np.zeros(len(frames), bool)
    for k, here in enumerate(masks):
        at = lab_off[k] + np.flatnonzero(here)
        if not done[k] or not here.any():
            continue
        # refine_pages' construction: the line's present peaks alone, a box from the previous present position on
        want = forced.peak_boxes(per_slot[k][here, 2], [int(here.sum())], T[k:k + 1], raw_w[k:k + 1], x_min[k:k + 1],
                                 y_min[k:k + 1], y_max[k:k + 1], ocr.PAD)
        assert np.array_equal(rows[at], want), k
        assert rows[at[0], 0] == x_min[k] and (rows[at[1:], 0] == rows[at[:-1], 2]).all()
        used[at] = True
    assert used.sum() == sum(int(m.sum()) for k, m in enumerate(masks) if done[k]) and (rows[~used] == 0).all()
    # all slots in ONE peak_boxes call, as refine_pages forms them, give the same rows
    live = [k for k in range(len(masks)) if done[k] and masks[k].any()]
    together = forced.peak_boxes(np.concatenate([per_slot[k][masks[k], 2] for k in live]), [int(masks[k].sum()) for k in live],
                                 T[live], raw_w[live], x_min[live], y_min[live], y_max[live], ocr.PAD)
    assert np.array_equal(rows[used], together)
    # without `done` every slot counts; a negative first field other than -1 is omitted as well
    frames[lab_off[4], 0] = -9
    rows = forced.present_box_rows(frames, L, lab_off, T, raw_w, x_min, y_min, y_max, ocr.PAD)
    assert (rows[lab_off[4]] == 0).all() and (rows[lab_off[6]:lab_off[6] + 5] != 0).any()
    # no slot at all
    assert forced.present_box_rows(np.zeros((0, 3), np.int32), [], [], [], [], [], [], [], ocr.PAD).shape == (0, 4)


class _Chunk(object):
    """what PageChunk.omitted_pages reads of a finished chunk"""

    def __init__(self, lines_per_page, omitted):
        self.strips_per_page = [[None] * n for n in lines_per_page]
        self.pages = [None] * len(lines_per_page)
        self.omitted = omitted

    def first_line(self):
        from text_alignment_amd import alignToOCR as atocr
        return atocr.PageChunk.first_line(self)


def test_omitted_is_cut_into_pages_as_refined_is():
    from text_alignment_amd import alignToOCR as atocr
    cut = lambda lines, omitted: atocr.PageChunk.omitted_pages(_Chunk(lines, omitted))              # noqa: E731
    whole = np.asarray([0, -1, 3, 0, -1, 7], np.int32)
    got = cut([2, 0, 3, 1], whole)
    assert [g.tolist() for g in got] == [[0, -1], [], [3, 0, -1], [7]] and all(g.dtype == np.int32 for g in got)
    got[0][0] = 99                                       # copies: the chunk's array stays
    assert whole[0] == 0
    assert [g.tolist() for g in cut([0, 0], np.zeros(0, np.int32))] == [[], []]
    assert cut([], np.zeros(0, np.int32)) == []


def test_the_switch_is_off_by_default_in_every_layer():
    import inspect
    from text_alignment_amd import alignToOCR as atocr, forced
    assert "omit_q" in atocr.PageChunk.__slots__ and "omitted" in atocr.PageChunk.__slots__
    sig = inspect.signature(atocr.process_batch)
    assert sig.parameters["line_omit"].default is None and sig.parameters["omitted_out"].default is None
    assert inspect.signature(atocr.PageChunk.__init__).parameters["omit_q"].default is None
    assert inspect.signature(forced.Refining.__init__).parameters["omit_q"].default is None
    assert forced.OMIT_DOWNLOAD == ("omitted",) and "omitted" not in forced.DOWNLOAD
