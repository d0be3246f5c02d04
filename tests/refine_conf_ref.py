"""Plain-Python checker of record for ta_confidence_pages ("Inside the pipeline"; TEST ONLY).

It states the rule forced.refine_pages implements behind its confidence call -- every kept character of a refined line
takes the line's confidence at its place among the page's transcript characters, a syllable takes the smallest value among
its characters that have one -- plus the refusals of the device call.  Lists and loops.
"""
NO_CONFIDENCE = -(1 << 63)
OK, BOUNDS, RANGE, TABLE, SLOT, STATUS = 0, 1, 2, 3, 4, 5
FORCED_OK = 0


def confidence_page(n, line0, line1, table, refined, slot, slots, filled, confidence, label_cap, syl_first, syl_last):
    """one page: (status, char_conf [n], syl_conf [syllables]); with a non-zero status the two are None -- nothing of the
    page is written.  n: the page's transcript characters; table: rows [reason, t_first, L, ...] by chunk-wide line;
    refined, slot: per chunk-wide line, as ta_refine_columns wrote them; slots: per packed slot (L, lab_off, confidence
    status); filled: the slots that are filled; confidence: per label; syl_first / syl_last: per syllable of the page the
    inclusive range of its characters inside the page."""
    for f, l in zip(syl_first, syl_last):
        if f < 0 or l < f or l >= n:
            return RANGE, None, None
    mine = [q for q in range(line0, line1) if refined[q] != 0]
    for q in mine:                                       # a row that leaves the page's characters, labels outside label_cap
        k = slot[q]
        if 0 <= k < filled and slots[k][2] == FORCED_OK:
            L, off, _ = slots[k]
            tf = table[q][1]
            if L < 1 or off < 0 or off + L > label_cap or tf < 0 or tf + L > n:
                return TABLE, None, None
    if any(not 0 <= slot[q] < filled for q in mine):
        return SLOT, None, None
    if any(slots[slot[q]][2] != FORCED_OK for q in mine):
        return STATUS, None, None
    cc = [NO_CONFIDENCE] * n
    written = set()
    for q in mine:
        L, off, _ = slots[slot[q]]
        a = table[q][1]
        if written & set(range(a, a + L)):
            raise ValueError("two refined lines keep the same character: ta_refine_columns never leaves that")
        written |= set(range(a, a + L))
        cc[a:a + L] = [int(c) for c in confidence[off:off + L]]
    sc = []
    for f, l in zip(syl_first, syl_last):
        have = [c for c in cc[f:l + 1] if c != NO_CONFIDENCE]
        sc.append(min(have) if have else NO_CONFIDENCE)
    return OK, cc, sc
