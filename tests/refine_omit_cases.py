"""The cases of ta_refine_columns_omit that tests/test_refine_omit_sim.py (the host build of csrc/ta_refine.hip) and
tests/test_refine_omit_columns_gpu.py (the real kernel) share: the pages and the layout of tests/refine_cases.py with the
forced alignment's FRAMES attached, and the answers of the checker tests/refine_omit_ref.py.

A case is (name, chunk) as in refine_cases, and the chunk says besides which characters the path left out:
  "gone"     {slot: [characters] or "all"}, the slots counted from the case's own first page as refine_cases counts them;
  "scatter"  a probability: every character of every slot is left out with it (the chunk's own generator);
  "field"    the first field an omitted character's row holds (default -1, what the aligner writes).
The row of a present character is (i, i, i) -- character 0 has the frame 0, the edge of "not negative" -- and every row of
frames that no FILLED slot with forced status OK owns is LIVE (7777, 7777, 7777): a kernel that reads one of them takes
its character for present.  The front page's slot (refine_cases.front) has every character present.
"""
import numpy as np

import refine_cases as RC
import refine_omit_ref as R
from text_alignment_amd import _abi

POISON8, POISON32 = RC.POISON8, RC.POISON32
LIVE = 7777


def bind(lib):
    return _abi.bind(lib, ["ta_refine_columns", "ta_refine_columns_omit"])


def _long_line(L):
    """the codes of ONE line whose run holds exactly L transcript characters: pairs, an op-1 column now and then inside,
    an op-2 column behind every 50th"""
    codes = []
    for i in range(L):
        codes.append("1" if 0 < i < L - 1 and i % 37 == 36 else "0")
        if i % 50 == 49:
            codes.append("2")
    return "".join(codes)


class _NoRows(object):
    """refine_cases._finish draws a page's old box rows as a permutation of BOX_BASE cut to m: none here"""

    @staticmethod
    def permutation(n):
        return np.zeros(0, np.int64)


def _seg_page(rng, segs):
    """refine_cases.seg_page, also for a page of more than BOX_BASE OCR characters: its old box rows drawn with repeats"""
    ops = np.asarray([int(ch) for _, codes in segs for ch in codes], np.uint8)
    o_line = np.asarray([line for line, codes in segs for ch in codes if ch != "1"], np.int32)
    if len(o_line) <= RC.BOX_BASE:
        return RC.seg_page(rng, segs)
    pg = RC._finish(_NoRows, ops, o_line, 1 + int(o_line.max()), lambda l: True, None)
    pg["idx"] = rng.integers(0, RC.BOX_BASE, size=len(o_line)).astype(np.int32)
    return pg


def cases():
    rng = np.random.default_rng(1416)
    every = lambda l: True                                                                           # noqa: E731
    two = lambda: RC.seg_page(rng, [(0, "0010200"), (None, "1"), (1, "02000")])                      # noqa: E731
    out = [("the first kept character omitted", dict(pages=[two()], gone={0: [0], 1: [0]})),
           ("the last kept character omitted", dict(pages=[two()], gone={0: [5], 1: [3]})),
           ("the first and the last omitted", dict(pages=[two()], gone={0: [0, 5], 1: [0, 3]})),
           ("nothing omitted", dict(pages=[two()], gone={}))]
    one = RC.seg_page(rng, [(0, "0"), (None, "11"), (1, "202"), (2, "00")], accept=lambda l: l < 2, trim=lambda l: (0, 0))
    out.append(("L = 1 present and L = 1 omitted", dict(pages=[one], gone={1: "all"})))
    out.append(("L = 1 omitted and L = 1 present", dict(pages=[dict(one)], gone={0: "all"})))
    three = lambda: RC.seg_page(rng, [(0, "0020"), (None, "1"), (1, "0201020"), (2, "000")])         # noqa: E731
    out.append(("a line with every character omitted between refined neighbours", dict(pages=[three()], gone={1: "all"})))
    out.append(("every line with every character omitted", dict(pages=[three()], gone={0: "all", 1: "all", 2: "all"})))
    out.append(("all but one omitted", dict(pages=[three()], gone={1: [0, 1, 3, 4], 2: [1, 2], 0: [0, 1]})))
    # a run over the tile edge: line 1 keeps the transcript characters 60 .. 69 = the page's columns 60 .. 69
    edge = lambda: RC.seg_page(rng, [(0, "0" * 60), (1, "0" * 10), (2, "0" * 70)])                   # noqa: E731
    out.append(("omitted in column 63", dict(pages=[edge()], gone={1: [3]})))
    out.append(("omitted in column 64", dict(pages=[edge()], gone={1: [4]})))
    out.append(("omitted in columns 63 and 64", dict(pages=[edge()], gone={1: [3, 4], 2: [57, 58]})))
    for L in (64, 65, 1023):
        out.append(("L = %d scattered" % L, dict(pages=[_seg_page(rng, [(0, _long_line(L))])], scatter=0.3)))
    out.append(("L = 1023 beside short lines", dict(pages=[_seg_page(rng, [(0, "000"), (1, _long_line(1023)), (2, "00")])],
                                                    scatter=0.5)))
    out.append(("a slot the forced alignment refused carries live frames",
                dict(pages=[RC.rand_page(rng, 130, 4, accept=every)], f_status={2: 1, 3: 2}, scatter=0.3)))
    out.append(("a negative first field that is not -1", dict(pages=[two()], gone={0: [1, 2], 1: [0]}, field=-7)))
    out.append(("the most negative first field", dict(pages=[two()], gone={0: [1, 2], 1: [0]}, field=-2 ** 31)))
    pg = RC.rand_page(rng, 90, 3, accept=every)
    pg["plain"] = 0
    out.append(("an object-path page", dict(pages=[pg, RC.rand_page(rng, 66, 2, accept=every)], scatter=0.3)))
    pg = RC.rand_page(rng, 100, 3, accept=every)
    pg["harvest"] = 2
    pg["rows"] = [[RC.PAGE, 0, 0]] * 3
    out.append(("a page the harvest refused", dict(pages=[RC.rand_page(rng, 40, 2, accept=every), pg,
                                                          RC.rand_page(rng, 64, 2, accept=every)], scatter=0.3)))
    pg = RC.seg_page(rng, [(0, "000000"), (1, "00000")])
    pg["rows"][1][1] -= 1                                   # line 1 claims a character in front of its run
    out.append(("a CONTAIN page", dict(pages=[RC.rand_page(rng, 40, 2, accept=every), pg, RC.rand_page(rng, 64, 2, accept=every)],
                                       gone={2: [1], 3: [0, 4]})))
    pg = RC.seg_page(rng, [(0, "000000"), (1, "00000")])
    pg["rows"][1][1] -= 1                                   # ... but has no present character: not refined, its run not held
    out.append(("kept characters in front of the run of a line with every character omitted", dict(pages=[pg], gone={1: "all"})))
    pg = RC.seg_page(rng, [(0, "000000"), (1, "00000")])    # the slot against the table: held for every candidate
    out.append(("a slot whose L is not the table's, every character omitted", dict(pages=[pg], L_edit={1: 4}, gone={1: "all"})))
    more = 150 * 7 + 3                                      # more than one tile of lines on a page
    out.append(("70 lines on a page", dict(pages=[RC.rand_page(rng, more, 70)], scatter=0.4)))
    # refine_cases' own cases, every one with a scattered mask
    for name, chunk in RC.cases():
        out.append(("refine_cases: " + name, dict(chunk, scatter=0.25)))
    return out


def pack(chunk, seed=0):
    """refine_cases.pack's arrays plus frames [label_cap][3] and the poisoned output omitted [nlines + 1]"""
    pk = RC.pack(chunk, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    filled = max(0, min(int(pk.count[0]), pk.nslots))
    shift = int((pk.acc_line[:pk.nslots - 2] < pk.line_first[1]).sum())        # the front page's slots
    pk.frames = np.full((pk.label_cap, 3), LIVE, np.int32)
    pk.present = {}                                                             # slot -> bool per character
    gone, field = chunk.get("gone", {}), chunk.get("field", -1)
    for k in range(pk.nslots - 2):
        L, off = int(pk.L[k]), int(pk.lab_off[k])
        here = np.ones(max(L, 0), bool)
        if k >= shift and "scatter" in chunk:
            here = rng.random(len(here)) >= chunk["scatter"]
        if k - shift in gone:
            here[:] = True
            which = gone[k - shift]
            here[list(range(len(here))) if which == "all" else [i for i in which if i < len(here)]] = False
        if k < filled and pk.f_status[k] == 0 and L >= 1 and off >= 0 and off + L <= pk.label_cap:
            pk.present[k] = here
            rows = np.repeat(np.arange(L, dtype=np.int32)[:, None], 3, axis=1)
            rows[~here] = (field, -1 if field == -1 else 5, -1 if field == -1 else 5)
            pk.frames[off:off + L] = rows
    pk.omitted = np.full(pk.nlines + 1, POISON32, np.int32)
    return pk


INPUTS = RC.INPUTS + ("frames",)
OUTPUTS = RC.OUTPUTS + ("omitted",)


def call(lib, pk, ptr, stream=None, **over):
    """ta_refine_columns_omit on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to replace"""
    a = dict(ops_bytes=pk.ops_bytes, t_len=pk.t_len, o_len=pk.o_len, nprob=pk.nprob, nlines=pk.nlines, nslots=pk.nslots,
             label_cap=pk.label_cap, box_base=pk.box_base)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    return lib.ta_refine_columns_omit(a["ops"], a["ops_off"], a["ops_len"], a["ops_bytes"], a["t_off"], a["o_off"], a["t_len"],
                                      a["o_len"], a["nprob"], a["o_line"], a["line_first"], a["idx"], a["table"], a["h_status"],
                                      a["nlines"], a["acc_line"], a["L"], a["lab_off"], a["count"], a["nslots"], a["label_cap"],
                                      a["f_status"], a["frames"], a["plain"], a["box_base"], a["ops_new"], a["ops_new_len"],
                                      a["idx_new"], a["idx_new_len"], a["refined"], a["slot"], a["omitted"], a["status"], stream)


def slots_of(pk):
    filled = max(0, min(int(pk.count[0]), pk.nslots))
    return {int(pk.acc_line[k]): (k, int(pk.L[k]), int(pk.lab_off[k]), int(pk.f_status[k])) for k in range(filled)}


def want(pk):
    """the checker's answer for a packed chunk: [(status, ops, idx)] per page, refined, slot and omitted [nlines]"""
    slots, table, frames = slots_of(pk), pk.table.tolist(), pk.frames.tolist()
    per_page, refined, slot = [], np.zeros(pk.nlines, np.int32), np.full(pk.nlines, -1, np.int32)
    omitted = np.full(pk.nlines, -1, np.int32)
    for p, pg in enumerate(pk.pages):
        o_line = pk.o_line[pk.o_off[p]:pk.o_off[p + 1]]
        l0, l1 = int(pk.line_first[p]), int(pk.line_first[p + 1])
        st, ops, idx, mine, gone = R.refine_page(pg["ops"], pg["idx"], o_line, pg["n"], l0, l1, table, slots, bool(pg["plain"]),
                                                 pk.box_base, pk.label_cap, frames, pg["harvest"] == 0)
        per_page.append((st, np.asarray(ops, np.uint8), np.asarray(idx, np.int32)))
        omitted[l0:l1] = gone
        for l, k in mine.items():
            refined[l], slot[l] = 1, k
    return per_page, refined, slot, omitted


def compare(pk, answer=None):
    """every output word against the checker, omitted included, poison elsewhere (refine_cases.compare's rules)"""
    per_page, refined, slot, omitted = answer or want(pk)
    RC.compare(pk, answer=(per_page, refined, slot))
    assert pk.omitted[:pk.nlines].tolist() == omitted.tolist()
    assert pk.omitted[pk.nlines] == POISON32
