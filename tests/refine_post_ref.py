"""Plain-numpy checker of record for ta_posterior_pages ("Inside the pipeline"; TEST ONLY).

It states the rule forced.refine_pages implements behind its posterior call -- every kept character of a refined line
takes ldexp(own_m / z_m, own_x - z_x) of its line (forced.posterior_values: ONE float64 division, one ldexp) at its place
among the page's transcript characters, a syllable takes the smallest value among its characters that have one -- plus
the refusals of the device call, which are ta_confidence_pages' (tests/refine_conf_ref.py).  "No value" is numpy's np.nan.
"""
import numpy as np

NO_POSTERIOR_BITS = 0x7FF8000000000000
OK, BOUNDS, RANGE, TABLE, SLOT, STATUS = 0, 1, 2, 3, 4, 5
FORCED_OK = 0
assert np.array([np.nan]).view(np.int64)[0] == NO_POSTERIOR_BITS


def posterior_page(n, line0, line1, table, refined, slot, slots, filled, own_m, own_x, z_m, z_x, label_cap, syl_first, syl_last):
    """one page: (status, char_post [n] float64, syl_post [syllables] float64); with a non-zero status the two are None --
    nothing of the page is written.  n: the page's transcript characters; table: rows [reason, t_first, L, ...] by
    chunk-wide line; refined, slot: per chunk-wide line, as ta_refine_columns wrote them; slots: per packed slot (L,
    lab_off, posterior status); filled: the slots that are filled; own_m / own_x: per label; z_m / z_x: per slot;
    syl_first / syl_last: per syllable of the page the inclusive range of its characters inside the page."""
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
    cp = np.full(n, np.nan, dtype=np.float64)
    written = set()
    for q in mine:
        k = slot[q]
        L, off, _ = slots[k]
        a = table[q][1]
        if written & set(range(a, a + L)):
            raise ValueError("two refined lines keep the same character: ta_refine_columns never leaves that")
        written |= set(range(a, a + L))
        cp[a:a + L] = np.ldexp(np.asarray(own_m[off:off + L], dtype=np.float64) / np.float64(z_m[k]),
                               np.asarray(own_x[off:off + L], dtype=np.int64) - np.int64(z_x[k]))
    sp = np.full(len(syl_first), np.nan, dtype=np.float64)
    for j, (f, l) in enumerate(zip(syl_first, syl_last)):
        have = cp[f:l + 1]
        have = have[~np.isnan(have)]
        if len(have):
            sp[j] = have.min()
    return OK, cp, sp
