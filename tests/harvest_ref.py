"""Plain-Python checker of the harvesting rule (TEST ONLY).

It works from the two ALIGNED sequences of a page, column by column, the way one would do it by hand on paper: one loop
over the columns that remembers the line of the last OCR character seen, no prefix counts, no masks, no searches.  A gap
is the object GAP (None); the tokens are whatever the caller aligned (characters, ids) and are only compared with ==.
"""
import numpy as np

GAP = None
FIELDS = 8
EMPTY, LOW, SEAM, UNANCHORED, CODEC, TOO_LONG, PAGE = 1, 2, 4, 8, 16, 32, 64
MAX_TARGET = 1024


def aligned_from_ops(ops, t_tokens, o_tokens):
    """the alignment columns (0 pair, 1 transcript over a gap, 2 gap over OCR) as the two aligned lists"""
    tra, ocr, i, j = [], [], 0, 0
    for op in ops:
        if op == 0:
            tra.append(t_tokens[i]); ocr.append(o_tokens[j]); i += 1; j += 1
        elif op == 1:
            tra.append(t_tokens[i]); ocr.append(GAP); i += 1
        else:
            tra.append(GAP); ocr.append(o_tokens[j]); j += 1
    assert i == len(t_tokens) and j == len(o_tokens)
    return tra, ocr


def aligned_from_strings(tra, ocr, gap="#"):
    """two equally long strings with `gap` for a gap (the worked example's notation)"""
    assert len(tra) == len(ocr)
    return [GAP if c == gap else c for c in tra], [GAP if c == gap else c for c in ocr]


def page_refused(o_line, line0, line1, unfinished=False):
    """what the kernel must refuse of a page's data: an unfinished traceback, an o_line that decreases or leaves the
    page's lines (the column counts cannot disagree here: the aligned lists ARE the columns)"""
    if unfinished:
        return True
    prev = line0
    for l in o_line:
        if l < line0 or l >= line1 or l < prev:
            return True
        prev = l
    return False


def harvest_page(tra, ocr, o_line, line0, line1, t_class, T, num, den, unfinished=False):
    """rows {line: [reason, t_first, L, equal, unequal, interior, op2, seam]} for the lines line0 .. line1 - 1 of one
    page.  o_line: the batch-wide line of every OCR character (gaps not counted), t_class: the class of every transcript
    character, T: indexable by batch-wide line."""
    assert len(tra) == len(ocr)
    if page_refused(o_line, line0, line1, unfinished):
        return {l: [PAGE, 0, 0, 0, 0, 0, 0, 0] for l in range(line0, line1)}
    assert sum(1 for o in ocr if o is not GAP) == len(o_line)
    assert sum(1 for t in tra if t is not GAP) == len(t_class)
    # the last OCR-carrying column of every line
    last_col, j = {}, 0
    for c, o in enumerate(ocr):
        if o is not GAP:
            last_col[o_line[j]] = c
            j += 1
    acc = {l: {"chars": [], "eq": 0, "ne": 0, "in": 0, "g2": 0, "seam": 0} for l in range(line0, line1)}
    cur = None                      # the line of the last OCR character seen
    waiting = 0                     # seam characters (no spaces) since then
    i = j = 0
    for c in range(len(tra)):
        t, o = tra[c], ocr[c]
        if o is not GAP:
            l = o_line[j]
            j += 1
            if waiting:
                acc[l]["seam"] += waiting
                if cur is not None:
                    acc[cur]["seam"] += waiting
                waiting = 0
            cur = l
            if t is not GAP:
                acc[l]["chars"].append((i, t == o))
                acc[l]["eq" if t == o else "ne"] += 1
                i += 1
            else:
                acc[l]["g2"] += 1
        else:
            if cur is not None and c < last_col[cur]:
                acc[cur]["chars"].append((i, False))
                acc[cur]["in"] += 1
            elif t_class[i] != 1:
                waiting += 1
            i += 1
    if waiting and cur is not None:
        acc[cur]["seam"] += waiting
    rows = {}
    for l in range(line0, line1):
        a = acc[l]
        chars = list(a["chars"])
        while chars and t_class[chars[0][0]] == 1:
            chars.pop(0)
        while chars and t_class[chars[-1][0]] == 1:
            chars.pop()
        assert [i for i, _ in chars] == list(range(chars[0][0], chars[0][0] + len(chars))) if chars else True
        L = len(chars)
        reason = 0
        if L == 0:
            reason |= EMPTY
        total = a["eq"] + a["ne"] + a["in"] + a["g2"]
        if total == 0 or a["eq"] * den < num * total:
            reason |= LOW
        if a["seam"] > 0:
            reason |= SEAM
        if L and not (chars[0][1] and chars[-1][1]):
            reason |= UNANCHORED
        if any(t_class[i] == 0 for i, _ in chars):
            reason |= CODEC
        if 2 * L + 1 > T[l] or L > MAX_TARGET:
            reason |= TOO_LONG
        rows[l] = [reason, chars[0][0] if L else 0, L, a["eq"], a["ne"], a["in"], a["g2"], a["seam"]]
    return rows


def harvest_batch(pages, T, num, den):
    """pages: dicts with "tra", "ocr" (aligned lists), "o_line", "t_class" and optionally "unfinished"; their lines
    follow one another: "lines" = how many each has.  Returns (table [nlines, 8] int32, refused page flags)."""
    rows, refused, line0 = [], [], 0
    for pg in pages:
        line1 = line0 + pg["lines"]
        r = harvest_page(pg["tra"], pg["ocr"], pg["o_line"], line0, line1, pg["t_class"], T, num, den,
                         pg.get("unfinished", False))
        rows.extend(r[l] for l in range(line0, line1))
        refused.append(page_refused(pg["o_line"], line0, line1, pg.get("unfinished", False)))
        line0 = line1
    return np.asarray(rows, dtype=np.int32).reshape(-1, FIELDS), refused


def texts_of(table, pages, transcripts):
    """per line the kept text (None for a line with none), from the table's t_first / L"""
    out, l = [], 0
    for pg, tr in zip(pages, transcripts):
        for _ in range(pg["lines"]):
            r = table[l]
            out.append(tr[r[1]:r[1] + r[2]] if r[2] > 0 else None)
            l += 1
    return out


def pack(table, pages):
    """the accepted lines in ascending order: (acc_line, L, lab_off, labels) as lists"""
    acc_line, Ls, lab_off, labels, l = [], [], [], [], 0
    for pg in pages:
        for _ in range(pg["lines"]):
            r = table[l]
            if r[0] == 0:
                acc_line.append(l)
                Ls.append(int(r[2]))
                lab_off.append(len(labels))
                labels.extend(int(c) for c in pg["t_class"][r[1]:r[1] + r[2]])
            l += 1
    return acc_line, Ls, lab_off, labels
