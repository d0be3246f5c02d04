"""The harvesting rule on hand-checked cases, through the plain-Python checker
tests/harvest_ref.py -- the reference every kernel test compares with -- and the host-side pieces of
text_alignment_amd.harvest that need no GPU."""
import os

import numpy as np
import pytest

import harvest_ref as R


def _classes(text, unknown=""):
    """space 1, a character of `unknown` 0, any other character 2 + its rank among the lower-case letters and digits"""
    return [1 if ch == " " else (0 if ch in unknown else 2 + "abcdefghijklmnopqrstuvwxyz0123456789".index(ch)) for ch in text]


def _page(segments, nlines, T, num=4, den=5, unknown="", line0=0):
    """segments (transcript, OCR, line) in the issue's notation, '#' for a gap: the rows of the page's lines and the
    kept texts"""
    tra = "".join(s[0] for s in segments)
    ocr = "".join(s[1] for s in segments)
    o_line = [line0 + s[2] for s in segments for ch in s[1] if ch != "#"]
    transcript = tra.replace("#", "")
    tr_al, oc_al = R.aligned_from_strings(tra, ocr)
    rows = R.harvest_page(tr_al, oc_al, o_line, line0, line0 + nlines, _classes(transcript, unknown),
                          {line0 + k: t for k, t in enumerate(T)}, num, den)
    rows = [rows[line0 + k] for k in range(nlines)]
    return rows, [transcript[r[1]:r[1] + r[2]] if r[2] else None for r in rows]


WORKED = [("xy ", "###", 0), ("in principio", "in principi0", 0), (" ", "#", 0), ("erat ver", "erat#v#r", 1),
          ("bum", "###", 1), ("#et verbum", " et ver8um", 3), (" ", "#", 3)]


def test_the_worked_example_exactly():
    rows, texts = _page(WORKED, 4, [40, 40, 40, 19])
    assert rows == [[12, 3, 12, 11, 1, 0, 0, 2],
                    [6, 16, 8, 6, 0, 2, 0, 3],
                    [3, 0, 0, 0, 0, 0, 0, 0],
                    [4, 27, 9, 8, 1, 0, 1, 3]]
    assert texts == ["in principio", "erat ver", None, "et verbum"]
    assert rows[0][0] == R.SEAM | R.UNANCHORED and rows[1][0] == R.LOW | R.SEAM
    assert rows[2][0] == R.EMPTY | R.LOW and rows[3][0] == R.SEAM
    # the same page further down a batch: only the line numbering moves
    assert _page(WORKED, 4, [40, 40, 40, 19], line0=17)[0] == rows


def test_an_accepted_line_and_every_reason_bit_alone():
    rows, texts = _page([("amen amen", "amen amen", 0)], 1, [19])
    assert rows == [[0, 0, 9, 9, 0, 0, 0, 0]] and texts == ["amen amen"]
    # EMPTY alone cannot be: a line without kept characters has no equal pair, so LOW comes with it
    rows, _ = _page([("amen", "amen", 0), ("###", "xyz", 1)], 2, [40, 40])
    assert rows[1] == [R.EMPTY | R.LOW, 0, 0, 0, 0, 0, 3, 0] and rows[0][0] == 0
    # LOW: 3 of 5 columns agree, below 4/5; both ends anchored
    rows, texts = _page([("abcde", "axcye", 0)], 1, [40])
    assert rows == [[R.LOW, 0, 5, 3, 2, 0, 0, 0]] and texts == ["abcde"]
    # SEAM: a word between two lines that neither line's OCR covers counts for both
    rows, texts = _page([("amen", "amen", 0), (" et ", "####", 0), ("deus", "deus", 1)], 2, [40, 40])
    assert rows == [[R.SEAM, 0, 4, 4, 0, 0, 0, 2], [R.SEAM, 8, 4, 4, 0, 0, 0, 2]] and texts == ["amen", "deus"]
    # ... spaces alone on a seam count for nothing
    rows, _ = _page([("amen", "amen", 0), ("  ", "##", 0), ("deus", "deus", 1)], 2, [40, 40])
    assert [r[0] for r in rows] == [0, 0] and [r[7] for r in rows] == [0, 0]
    # UNANCHORED: the last kept character stands over a different one (8 of 9 agree: not LOW)
    rows, _ = _page([("amen amex", "amen amen", 0)], 1, [40])
    assert rows == [[R.UNANCHORED, 0, 9, 8, 1, 0, 0, 0]]
    # ... or the first one
    rows, _ = _page([("xmen amen am", "amen amen am", 0)], 1, [40])
    assert rows[0][0] == R.UNANCHORED
    # CODEC: a kept character the codec lacks
    rows, _ = _page([("amen amen amen", "amen amen amen", 0)], 1, [40], unknown="e")
    assert rows == [[R.CODEC, 0, 14, 14, 0, 0, 0, 0]]
    # TOO_LONG: 2 L + 1 against T
    assert _page([("amen", "amen", 0)], 1, [9])[0][0][0] == 0
    assert _page([("amen", "amen", 0)], 1, [8])[0][0][0] == R.TOO_LONG
    long_text = "ab" * 513                                           # 1026 characters: over MAX_TARGET whatever T is
    assert _page([(long_text, long_text, 0)], 1, [5000])[0][0][0] == R.TOO_LONG
    assert _page([(long_text[:1024], long_text[:1024], 0)], 1, [2049])[0][0][0] == 0
    # PAGE: a refused page, all of its lines
    tr_al, oc_al = R.aligned_from_strings("amen", "amen")
    for o_line, unfinished in (([0, 1, 0, 1], False), ([0, 0, 0, 2], False), ([0, 0, 0, 0], True), ([-1, 0, 0, 0], False)):
        rows = R.harvest_page(tr_al, oc_al, o_line, 0, 2, _classes("amen"), [40, 40], 4, 5, unfinished)
        assert rows == {0: [R.PAGE, 0, 0, 0, 0, 0, 0, 0], 1: [R.PAGE, 0, 0, 0, 0, 0, 0, 0]}


def test_counts_cover_every_column_before_trimming_and_interior_spaces_stay():
    # the line's run starts and ends with spaces (paired with OCR spaces): trimmed from the text, counted in field 3
    rows, texts = _page([(" in deo ", " in deo ", 0)], 1, [40])
    assert rows == [[0, 1, 6, 8, 0, 0, 0, 0]] and texts == ["in deo"]
    # interior op-1 columns belong to the line, the op-1 columns behind its last OCR character do not
    rows, texts = _page([("a", "a", 0), ("bc", "##", 0), ("d", "d", 0), ("ef", "##", 0)], 1, [40], num=1, den=2)
    assert rows == [[R.SEAM, 0, 4, 2, 0, 2, 0, 2]] and texts == ["abcd"]


def test_abbreviation_donors_keep_their_line():
    """an abbreviation's expansion takes the line of the character that lent its box: o_line simply repeats it, also
    where the expansion stands at a line's end"""
    rows, texts = _page([("dominus", "dominus", 0), (" ", "#", 0), ("deus", "deus", 1)], 2, [40, 40])
    # "dns" expanded to "dominus": d, o..i from the n, u..s from the s -- all on line 0 like their donors
    assert rows == [[0, 0, 7, 7, 0, 0, 0, 0], [0, 8, 4, 4, 0, 0, 0, 0]] and texts == ["dominus", "deus"]
    tr_al, oc_al = R.aligned_from_strings("dominus deus", "dominus#deus")
    o_line = [5] * 7 + [6] * 4
    got = R.harvest_page(tr_al, oc_al, o_line, 5, 7, _classes("dominus deus"), {5: 40, 6: 40}, 9, 10)
    assert [got[5], got[6]] == rows


def test_a_line_trimmed_to_nothing_a_page_without_ocr_and_an_empty_transcript():
    # the line's OCR pairs with spaces only
    rows, texts = _page([("amen", "amen", 0), ("   ", "   ", 1), ("deus", "deus", 2)], 3, [40, 40, 40])
    assert rows[1] == [R.EMPTY, 0, 0, 3, 0, 0, 0, 0] and texts == ["amen", None, "deus"]
    assert rows[0][0] == 0 and rows[2][0] == 0
    # no OCR character at all: every transcript character is on a seam that borders no line
    rows, texts = _page([("amen deus", "#########", 0)], 3, [40, 0, 40])
    assert rows == [[R.EMPTY | R.LOW, 0, 0, 0, 0, 0, 0, 0], [R.EMPTY | R.LOW | R.TOO_LONG, 0, 0, 0, 0, 0, 0, 0],
                    [R.EMPTY | R.LOW, 0, 0, 0, 0, 0, 0, 0]] and texts == [None, None, None]
    # an empty transcript: op-2 columns only
    rows, _ = _page([("####", "amen", 0), ("##", "et", 1)], 2, [40, 40])
    assert rows == [[R.EMPTY | R.LOW, 0, 0, 0, 0, 0, 4, 0], [R.EMPTY | R.LOW, 0, 0, 0, 0, 0, 2, 0]]
    # no columns at all
    assert _page([], 2, [40, 40])[0] == [[R.EMPTY | R.LOW, 0, 0, 0, 0, 0, 0, 0]] * 2


def test_the_two_thresholds_at_their_edges():
    # 2 L + 1 == T is accepted, 2 L + 1 == T + 1 refused
    assert _page([("et verbum", "et verbum", 0)], 1, [19])[0][0][0] == 0
    assert _page([("et verbum", "et verbum", 0)], 1, [18])[0][0][0] == R.TOO_LONG
    # agreement exactly at the threshold: 8 equal of 10 columns at 4/5 is accepted, 7 of 9 is not, 8 of 10 at 81/100 is not
    rows, _ = _page([("abcdefghab", "abxdefyhab", 0)], 1, [40], 4, 5)
    assert rows == [[0, 0, 10, 8, 2, 0, 0, 0]]                                   # 8 * 5 == 4 * 10
    assert _page([("abcdefghab", "abxdefyhab", 0)], 1, [40], 81, 100)[0][0][0] == R.LOW
    assert _page([("abcdefgha", "abxdefyha", 0)], 1, [40], 4, 5)[0][0][0] == R.LOW   # 7 * 5 < 4 * 9


def test_min_agreement_conversions_and_refusals():
    from text_alignment_amd import harvest
    assert harvest.agreement_ratio(0.9) == (9, 10)            # through str(): not the binary fraction next to 0.9
    assert harvest.agreement_ratio(0.8) == (4, 5) and harvest.agreement_ratio(1) == (1, 1)
    assert harvest.agreement_ratio("0.875") == (7, 8) and harvest.agreement_ratio(1.0) == (1, 1)
    assert harvest.agreement_ratio((4, 5)) == (4, 5) and harvest.agreement_ratio([90, 100]) == (90, 100)
    assert harvest.agreement_ratio(0.000001) == (1, 10 ** 6)
    for bad in (0, 0.0, -0.5, 1.5, (6, 5), (0, 5), (1, 0), (-1, -2), 0.1234567, (1, 10 ** 6 + 1), float("nan"), "x",
                (1, 2, 3), (0.5, 1), None, (True, 1)):
        with pytest.raises(ValueError):
            harvest.agreement_ratio(bad)
    assert harvest.reason_names(0) == [] and harvest.reason_names(12) == ["SEAM", "UNANCHORED"]
    assert harvest.reason_names(127) == [n for n, _ in harvest.REASONS]
    assert (harvest.EMPTY, harvest.LOW, harvest.SEAM, harvest.UNANCHORED, harvest.CODEC, harvest.TOO_LONG, harvest.PAGE,
            harvest.FIELDS) == (R.EMPTY, R.LOW, R.SEAM, R.UNANCHORED, R.CODEC, R.TOO_LONG, R.PAGE, R.FIELDS)


def test_transcript_classes_number_characters_as_the_trainer_does():
    from text_alignment_amd import harvest, train
    codec = train.make_codec("abc de")
    text = "a bed cab"
    assert harvest.transcript_classes(codec, text).tolist() == train.encode_text(codec, text)
    assert harvest.transcript_classes(codec, "a?b ").tolist() == [codec.index("a"), 0, codec.index("b"), 1]
    assert harvest.transcript_classes(codec, "").tolist() == []
    with pytest.raises(ValueError):
        harvest.transcript_classes(["", "~", " ", "a"], "a")
    assert train.MAX_TARGET == R.MAX_TARGET


def test_library_refuses_bad_arguments_before_any_launch():
    """validation comes before any HIP call: safe without a GPU"""
    from text_alignment_amd import _native
    lib = _native.lib
    one = np.zeros(4, dtype=np.int64)
    p = one.ctypes.data
    ws = np.zeros(4096 + 16, dtype=np.uint8)
    wp = ws.ctypes.data + (-ws.ctypes.data) % 16

    def call(nprob=1, nlines=0, num=4, den=5, t_off=(0, 0), o_off=(0, 0), lf=(0, 0), ws_bytes=4096, wsp=wp):
        t_off, o_off, lf = (np.asarray(a, dtype=np.int64) for a in (t_off, o_off, lf))
        return lib.ta_harvest_lines(p, p, p, 16, p, p, p, p, nprob, p, p, p, p, nlines, num, den, t_off.ctypes.data,
                                    o_off.ctypes.data, lf.ctypes.data, wsp, ws_bytes, p, p, None)
    E, LIM = _native.TA_EINVAL, _native.TA_ELIMIT
    assert call(nprob=-1) == E and call(nlines=-1) == E and call(nprob=0, nlines=0) == 0 and call(nprob=0, nlines=1) == E
    assert call(num=0) == E and call(den=0) == E and call(num=6, den=5) == E and call(num=1, den=10 ** 6 + 1) == E
    assert call(t_off=(5, 3)) == E and call(o_off=(0, -1)) == E and call(lf=(0, 1)) == E and call(lf=(1, 0)) == E
    assert call(nlines=2, lf=(0, 2), ws_bytes=8) == E and call(wsp=wp + 4) == E and call(wsp=None) == E
    assert b"null" in lib.ta_last_error()
    assert call(t_off=(0, (1 << 24) + 1)) == LIM and call(nlines=(1 << 24) + 1, lf=(0, (1 << 24) + 1)) == LIM
    assert lib.ta_harvest_workspace_bytes(-1, 0, 0) == E and lib.ta_harvest_workspace_bytes((1 << 24) + 1, 0, 0) == LIM
    assert lib.ta_harvest_workspace_bytes(10, 100, 80) >= 10 * 8 + 80 * 5 + 100
    assert lib.ta_harvest_pack(p, wp, 64, p, 0, -1, 1, p, p, p, p, p, None) == E
    assert lib.ta_harvest_pack(p, None, 64, p, 0, 0, 1, p, p, p, p, p, None) == E
    assert lib.ta_harvest_pack(p, wp, 8, p, 0, 4, 1, p, p, p, p, p, None) == E
    assert lib.ta_harvest_pack(p, wp, 1 << 30, p, 0, (1 << 24) + 1, 1, p, p, p, p, p, None) == LIM


def test_rharvest_finds_pages_and_writes_report_rows(tmp_path):
    """tools/rharvest.py, the parts that need no GPU: which files are pages, --min-agreement, a report row"""
    from text_alignment_amd import harvest
    from tools import rharvest
    for name in ("b.png", "b.txt", "a.JPG", "a.txt", "c.png", "d.txt", "e.gt.txt"):
        (tmp_path / name).write_bytes(b"")
    found = rharvest.find_pages(str(tmp_path))
    assert [(n, os.path.basename(i), os.path.basename(t)) for n, i, t in found] == [("a", "a.JPG", "a.txt"), ("b", "b.png", "b.txt")]
    assert harvest.agreement_ratio(rharvest.parse_agreement("0.85")) == (17, 20)
    assert harvest.agreement_ratio(rharvest.parse_agreement("9/10")) == (9, 10)
    ln = harvest.HarvestLine(0, 3, None, None, "in\tprincipio", 12, {"equal": 11, "unequal": 1, "interior": 0, "op2": 0, "seam": 2})
    row = rharvest.report_row("folio_012", ln, 3)
    assert len(row) == len(rharvest.HEADER)
    assert row == ["folio_012", "3", "12", "SEAM,UNANCHORED", "3", "12", "11", "1", "0", "0", "2", "in principio"]
    ok = harvest.HarvestLine(0, 0, None, None, None, 3, dict.fromkeys(harvest.COUNT_NAMES, 0))
    assert rharvest.report_row("p", ok, 0)[3] == "EMPTY,LOW" and rharvest.report_row("p", ok, 0)[-1] == ""
