"""Plain-Python checker of record for ta_refine_columns_omit (TEST ONLY).

ta_refine_columns behind a forced alignment that may leave characters of a line's text out.  It states

  present   character i of packed slot k is PRESENT iff the first field of its row of frames, row lab_off[k] + i, is not
            negative (-1 is what the aligner writes; any negative value counts as omitted);
  omitted   per line the number of its slot's characters that are not present -- for a line with a FILLED slot whose
            forced status is OK, whose L is at most MAX_TARGET and whose rows lie inside frames (L >= 1, 0 <= lab_off,
            lab_off + L <= label_cap), whether or not its page is plain; -1 for every other line, and for every line of
            a page whose status is not OK;
  refined   a line of refine_ref.refined_lines' predicate (the CANDIDATES, on which the containment checks stay) that has
            at least one present character.  A candidate with none keeps its run, op-2 columns included;
  columns   refine_ref.refine_page's cut-and-replace form: the run from the line's first to its last OCR-carrying column
            becomes op-1 columns, then per kept character a pair (op 0) if it is present and an op-1 column if not, then
            op-1 columns; the box row of present character i stays box_base + lab_off[k] + i, the strict numbering, and
            the rows of omitted characters are never referenced.

Lists and loops, no prefix counts over masks, no compaction.  It imports neither the package's kernels nor
forced.refine_columns.
"""
from refine_ref import BOUNDS, COLUMNS, CONTAIN, FORCED_OK, HARVEST, MAX_TARGET, OK, refined_lines      # noqa: F401


def present_of(frames, off, L):
    """a bool per character of a slot: the first field of its row of frames is not negative"""
    return [int(frames[off + i][0]) >= 0 for i in range(L)]


def omitted_counts(line0, line1, slots, frames, label_cap):
    """{line: characters its path left out} of the page's lines that have a count"""
    out = {}
    for l in range(line0, line1):
        if l in slots:
            _, Lk, off, fst = slots[l]
            if fst == FORCED_OK and 1 <= Lk <= MAX_TARGET and off >= 0 and off + Lk <= label_cap:
                out[l] = Lk - sum(present_of(frames, off, Lk))
    return out


def refine_page(ops, idx, o_line, n, line0, line1, table, slots, plain, box_base, label_cap, frames, harvest_ok=True):
    """one page: (status, new ops, new idx, {line: k} of its refined lines, omitted per line of the page).  The arguments
    are refine_ref.refine_page's plus frames: the rows [t_first, t_last, t_peak] the aligner wrote, by label row.  A page
    that fails keeps its columns, refines nothing and has -1 for every line."""
    ops, idx, o_line = [int(v) for v in ops], [int(v) for v in idx], [int(v) for v in o_line]
    m = len(o_line)
    keep = lambda status: (status, list(ops), list(idx), {}, [-1] * (line1 - line0))              # noqa: E731
    if not harvest_ok:
        return keep(HARVEST)
    prev = line0
    for l in o_line:
        if l < line0 or l >= line1 or l < prev:
            return keep(COLUMNS)
        prev = l
    candidates = refined_lines(table, line0, line1, slots, plain)
    for l, k in candidates.items():
        _, Lk, off, _ = slots[l]
        tf = table[l][1]
        if Lk < 1 or Lk != table[l][2] or off < 0 or off + Lk > label_cap or tf < 0 or tf + Lk > n:
            return keep(CONTAIN)
    gone = omitted_counts(line0, line1, slots, frames, label_cap)
    mine = dict((l, k) for l, k in candidates.items() if gone[l] < slots[l][1])
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
        present = present_of(frames, slots[l][2], L)
        new_ops += ops[c_done:c0] + [1] * (tf - ta) + [0 if here else 1 for here in present] + [1] * (tb - tf - L)
        new_idx += idx[j_done:jlo] + [row + i for i in range(L) if present[i]]
        c_done, j_done = c1 + 1, jhi + 1
    return OK, new_ops + ops[c_done:], new_idx + idx[j_done:], mine, [gone.get(l, -1) for l in range(line0, line1)]
