"""Plain-Python checker of record for ta_refine_columns ("Realisation on the device"; TEST ONLY).

It holds three things: WHICH lines are refined (the predicate), the rule of forced.refine_columns for the columns of a
refined line -- written the way that function writes it: the run from the line's first to its last OCR-carrying column
is cut out and op-1 columns, L pairs, op-1 columns are put in its place -- and the numbering of the new box rows, kept
character i of packed slot k at box_base + lab_off[k] + i.  Lists and loops, no prefix counts over masks, no compaction.
"""
OK, HARVEST, BOUNDS, COLUMNS, CONTAIN = 0, 1, 2, 3, 4
MAX_TARGET = 1023               # TA_FORCED_MAX_TARGET
FORCED_OK = 0


def refined_lines(table, line0, line1, slots, plain):
    """{line: k} of the page's refined lines.  table: rows [reason, t_first, L, ...] by chunk-wide line; slots: {line:
    (k, L[k], lab_off[k], forced status[k])} of the FILLED packed slots; plain: the page's flag"""
    out = {}
    for l in range(line0, line1):
        if table[l][0] == 0 and l in slots and slots[l][3] == FORCED_OK and slots[l][1] <= MAX_TARGET and plain:
            out[l] = slots[l][0]
    return out


def refine_page(ops, idx, o_line, n, line0, line1, table, slots, plain, box_base, label_cap, harvest_ok=True):
    """one page: (status, new ops, new idx, {line: k} of its refined lines).  ops: the columns (0 pair, 1 transcript
    character alone, 2 OCR character alone), idx: per OCR character its old box row, o_line: per OCR character its
    chunk-wide line, n: the page's transcript characters.  A page that fails keeps its columns and refines nothing."""
    ops, idx, o_line = [int(v) for v in ops], [int(v) for v in idx], [int(v) for v in o_line]
    m = len(o_line)
    keep = lambda status: (status, list(ops), list(idx), {})                                     # noqa: E731
    if not harvest_ok:
        return keep(HARVEST)
    prev = line0
    for l in o_line:
        if l < line0 or l >= line1 or l < prev:
            return keep(COLUMNS)
        prev = l
    mine = refined_lines(table, line0, line1, slots, plain)
    for l, k in mine.items():
        _, Lk, off, _ = slots[l]
        tf = table[l][1]
        if Lk < 1 or Lk != table[l][2] or off < 0 or off + Lk > label_cap or tf < 0 or tf + Lk > n:
            return keep(CONTAIN)
    if any(op > 2 for op in ops) or sum(op != 2 for op in ops) != n or sum(op != 1 for op in ops) != m:
        return keep(COLUMNS)
    col_of_o = [c for c, op in enumerate(ops) if op != 1]
    t_before, t = [], 0
    for op in ops:
        t_before.append(t)
        t += op != 2
    new_ops, new_idx, c_done, j_done = [], [], 0, 0
    for l in sorted(mine):
        js = [j for j in range(m) if o_line[j] == l]
        if not js:
            return keep(CONTAIN)
        jlo, jhi = js[0], js[-1]
        c0, c1 = col_of_o[jlo], col_of_o[jhi]
        ta, tb = t_before[c0], t_before[c1] + (ops[c1] != 2)
        tf, L = int(table[l][1]), int(table[l][2])
        if not (jhi - jlo + 1 == len(js) and c0 >= c_done and ta <= tf and tf + L <= tb):
            return keep(CONTAIN)
        row = box_base + slots[l][2]
        new_ops += ops[c_done:c0] + [1] * (tf - ta) + [0] * L + [1] * (tb - tf - L)
        new_idx += idx[j_done:jlo] + list(range(row, row + L))
        c_done, j_done = c1 + 1, jhi + 1
    return OK, new_ops + ops[c_done:], new_idx + idx[j_done:], mine
