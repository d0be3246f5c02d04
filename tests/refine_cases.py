"""The cases of ta_refine_columns that tests/test_refine_sim.py (the host build of csrc/ta_refine.hip) and
tests/test_refine_gpu.py (the real kernel) share, the layout both drive it with, and the checker's answers.

A case is (name, chunk); a chunk is a list of pages {"ops", "o_line" (page-relative lines), "idx", "lines", "rows"
(per line [reason, t_first, L]), "plain", "harvest" (the harvest's status of the page)} plus what the packed slots say.
`pack` lays a chunk out the way an NWBatch and the harvest leave it -- columns right-aligned in regions of n + m bytes,
the packed arrays ascending -- but with no offset at 0: a small page with one refined line stands in FRONT of every
case's pages, t_off / o_off / ops_off / lab_off start above 0, and every output is poisoned.
"""
import numpy as np

import refine_ref as R
from text_alignment_amd import _abi

POISON8, POISON32 = 0xEE, -0x21212122
BOX_BASE = 1000
EMPTY, LOW, PAGE = 1, 2, 64


def bind(lib):
    return _abi.bind(lib, ["ta_refine_columns"])


# ---- pages -----------------------------------------------------------------------------------------------------------------

def _run_range(ops, o_line, l):
    """(ta, tb) of line l's run: the transcript characters from its first to its last OCR-carrying column; None without"""
    cols = np.flatnonzero(ops != 1)
    js = np.flatnonzero(o_line == l)
    if not len(js):
        return None
    has_t = ops != 2
    t_before = np.cumsum(has_t) - has_t
    c0, c1 = cols[js[0]], cols[js[-1]]
    return int(t_before[c0]), int(t_before[c1]) + int(has_t[c1])


def _finish(rng, ops, o_line, nl, accept, trim):
    """rows of a page: line l is accepted (reason 0) where accept(l) says so and its run has a transcript character;
    trim(l) = (characters dropped in front, behind) of the run's transcript range"""
    ops, o_line = np.asarray(ops, np.uint8), np.asarray(o_line, np.int32)
    rows = []
    for l in range(nl):
        rg = _run_range(ops, o_line, l)
        if rg is None or rg[1] - rg[0] < 1:
            rows.append([EMPTY | LOW, 0, 0])
            continue
        ta, tb = rg
        a, b = trim(l) if trim else (0, 0)
        a = min(a, tb - ta - 1)
        b = min(b, tb - ta - 1 - a)
        rows.append([0 if accept(l) else LOW, ta + a, tb - ta - a - b])
    m = len(o_line)
    return {"ops": ops, "o_line": o_line, "idx": rng.permutation(BOX_BASE)[:m].astype(np.int32), "lines": nl, "rows": rows,
            "plain": 1, "harvest": 0, "n": int((ops != 2).sum())}


def seg_page(rng, segs, accept=lambda l: True, trim=None):
    """a page from segments (line or None, "column codes"): the OCR characters of a segment lie on its line; a segment
    without a line holds op-1 columns only"""
    ops, o_line = [], []
    for line, codes in segs:
        for ch in codes:
            op = int(ch)
            assert line is not None or op == 1
            ops.append(op)
            if op != 1:
                o_line.append(line)
    nl = 1 + max(l for l, _ in segs if l is not None)
    return _finish(rng, ops, o_line, nl, accept, trim)


def rand_page(rng, ncols, nl, accept=None, trim=None):
    """ncols random columns, their OCR characters dealt to nl lines in order"""
    ops = rng.choice(3, size=ncols, p=[0.7, 0.15, 0.15]).astype(np.uint8)
    m = int((ops != 1).sum())
    o_line = np.sort(rng.integers(0, nl, size=m)).astype(np.int32)
    flags = rng.random(nl) < 0.7
    trims = rng.integers(0, 3, size=(nl, 2))
    return _finish(rng, ops, o_line, nl, accept or (lambda l: bool(flags[l])), trim or (lambda l: tuple(int(v) for v in trims[l])))


def front(rng):
    return seg_page(rng, [(0, "00200"), (None, "1"), (1, "02")], accept=lambda l: l == 0)


def cases():
    rng = np.random.default_rng(2207)
    out = []
    for ncols in (0, 1, 63, 64, 65, 127, 128, 129, 1025):
        out.append(("%d columns" % ncols, dict(pages=[rand_page(rng, ncols, 1 + ncols // 40)])))
    every, none = (lambda l: True), (lambda l: False)
    out.append(("no line refined", dict(pages=[rand_page(rng, 150, 4, accept=none)])))
    out.append(("every line refined", dict(pages=[rand_page(rng, 150, 4, accept=every)])))
    out.append(("only the first line", dict(pages=[rand_page(rng, 150, 4, accept=lambda l: l == 0)])))
    out.append(("only the last line", dict(pages=[rand_page(rng, 150, 4, accept=lambda l: l == 3)])))
    out.append(("L = 1", dict(pages=[seg_page(rng, [(0, "0"), (None, "11"), (1, "202"), (2, "00")], accept=lambda l: l < 2,
                                              trim=lambda l: (0, 0))])))
    out.append(("pairs only", dict(pages=[seg_page(rng, [(0, "0000000"), (1, "000")])])))
    out.append(("op-2 at both ends and in the middle", dict(pages=[seg_page(rng, [(0, "2200201022"), (1, "2"), (2, "20102")])])))
    out.append(("trimmed at both ends", dict(pages=[seg_page(rng, [(0, "0010000100"), (None, "1"), (1, "000000")],
                                                             trim=lambda l: ((2, 0), (0, 3))[l])])))
    out.append(("trimmed to the run's op-1 columns", dict(pages=[seg_page(rng, [(0, "0111110")], trim=lambda l: (1, 1))])))
    pg = seg_page(rng, [(0, "00000100"), (1, "0000")])
    pg["idx"][3] = pg["idx"][2]                            # an expanded abbreviation: two characters, one box row
    pg["idx"][9] = pg["idx"][8]
    out.append(("an expanded abbreviation", dict(pages=[pg], only=[1])))
    out.append(("the abbreviation inside a refined line", dict(pages=[dict(pg)])))
    out.append(("neighbours with op-1 columns between", dict(pages=[seg_page(rng, [(0, "00100"), (None, "111"), (1, "0200"),
                                                                                    (None, "1"), (2, "00")])])))
    out.append(("three pages", dict(pages=[rand_page(rng, 70, 3), rand_page(rng, 5, 1, accept=every), rand_page(rng, 200, 6)])))
    pg = rand_page(rng, 90, 3, accept=every)
    pg["plain"] = 0
    out.append(("a page that is not plain", dict(pages=[pg, rand_page(rng, 66, 2, accept=every)])))
    out.append(("a slot the forced alignment refused", dict(pages=[rand_page(rng, 130, 4, accept=every)], f_status={2: 1, 3: 2})))
    out.append(("count -1", dict(pages=[rand_page(rng, 130, 4, accept=every)], count=-1)))
    out.append(("count below the slots", dict(pages=[rand_page(rng, 130, 4, accept=every)], count=2)))
    pg = rand_page(rng, 100, 3, accept=every)
    pg["harvest"] = 2
    pg["rows"] = [[PAGE, 0, 0]] * 3
    out.append(("a page the harvest refused", dict(pages=[rand_page(rng, 40, 2, accept=every), pg, rand_page(rng, 64, 2, accept=every)])))
    pg = seg_page(rng, [(0, "000000"), (1, "00000")])
    pg["rows"][1][1] -= 1                                   # line 1 claims a character in front of its run
    out.append(("kept characters in front of the run", dict(pages=[rand_page(rng, 40, 2, accept=every), pg,
                                                                    rand_page(rng, 64, 2, accept=every)])))
    pg = seg_page(rng, [(0, "000000"), (None, "11"), (1, "00000")])
    pg["rows"][0][2] += 1                                   # line 0 claims one behind it
    out.append(("kept characters behind the run", dict(pages=[pg, rand_page(rng, 64, 2, accept=every)])))
    pg = seg_page(rng, [(0, "000000"), (1, "00000")])
    out.append(("a slot whose L is not the table's", dict(pages=[pg, rand_page(rng, 64, 2, accept=every)], L_edit={1: 4})))
    pg = seg_page(rng, [(0, "000"), (2, "00")])
    pg["rows"][1] = [0, 3, 1]                               # an accepted line without an OCR character
    out.append(("a refined line without OCR characters", dict(pages=[pg])))
    pg = rand_page(rng, 80, 3, accept=every)
    pg["o_line"] = pg["o_line"][::-1].copy()
    out.append(("o_line decreases", dict(pages=[pg, rand_page(rng, 64, 2, accept=every)])))
    pg = rand_page(rng, 80, 3, accept=every)
    pg["ops"][40] = 3
    out.append(("a column code above 2", dict(pages=[pg, rand_page(rng, 64, 2, accept=every)])))
    return out


# ---- layout --------------------------------------------------------------------------------------------------------------

class Packed(object):
    pass


def pack(chunk, seed=0):
    """host arrays of one call, the front page first.  chunk: pages, and optionally f_status {slot: status}, count,
    L_edit {slot: L}, only [slots that stay: the others' lines are accepted but have no slot]"""
    rng = np.random.default_rng(seed)
    pages = [front(rng)] + list(chunk["pages"])
    pk = Packed()
    pk.pages, pk.nprob = pages, len(pages)
    n = np.asarray([pg["n"] for pg in pages], np.int64)
    m = np.asarray([len(pg["o_line"]) for pg in pages], np.int64)
    t_base, o_base, r_base = 3, 5, 7
    pk.t_off = np.concatenate([[t_base], t_base + np.cumsum(n)]).astype(np.int64)
    pk.o_off = np.concatenate([[o_base], o_base + np.cumsum(m)]).astype(np.int64)
    pk.ops_off = (r_base + np.concatenate([[0], np.cumsum(n + m)])).astype(np.int64)
    pk.t_len, pk.o_len, pk.ops_bytes = int(pk.t_off[-1]) + 2, int(pk.o_off[-1]) + 2, int(pk.ops_off[-1]) + 9
    pk.ops = np.full(pk.ops_bytes, POISON8, np.uint8)
    pk.ops_len = np.zeros(pk.nprob + 1, np.int32)
    pk.o_line = np.full(pk.o_len, -5, np.int32)
    pk.idx = np.full(pk.o_len, -9, np.int32)
    pk.line_first = np.concatenate([[0], np.cumsum([pg["lines"] for pg in pages])]).astype(np.int64)
    pk.nlines = int(pk.line_first[-1])
    pk.table = np.full((pk.nlines + 1, 8), 7, np.int32)
    for p, pg in enumerate(pages):
        end = int(pk.ops_off[p + 1])
        pk.ops[end - len(pg["ops"]):end] = pg["ops"]
        pk.ops_len[p] = len(pg["ops"])
        pk.o_line[pk.o_off[p]:pk.o_off[p + 1]] = pg["o_line"] + pk.line_first[p]
        pk.idx[pk.o_off[p]:pk.o_off[p + 1]] = pg["idx"]
        for l, row in enumerate(pg["rows"]):
            pk.table[pk.line_first[p] + l, :3] = row
    pk.h_status = np.asarray([pg["harvest"] for pg in pages] + [0], np.int32)
    pk.plain = np.asarray([pg["plain"] for pg in pages] + [1], np.uint8)
    acc = [q for q in range(pk.nlines) if pk.table[q, 0] == 0]
    if "only" in chunk:                                    # slots count from the case's own first page
        own = [q for q in acc if q >= pk.line_first[1]]
        acc = [q for q in acc if q < pk.line_first[1]] + [own[k] for k in chunk["only"]]
    shift = len([q for q in acc if q < pk.line_first[1]])  # the front page's slots
    Ls = [int(pk.table[q, 2]) for q in acc]
    for k, v in chunk.get("L_edit", {}).items():
        Ls[k + shift] = v
    pk.nslots = len(acc) + 2
    pk.acc_line = np.asarray(acc + [0x7FFFFFF0] * 2, np.int32)
    pk.L = np.asarray(Ls + [3, 3], np.int32)
    pk.lab_off = np.asarray([4 + sum(Ls[:k]) + k for k in range(len(acc))] + [1 << 40] * 2, np.int64)
    pk.label_cap = 4 + sum(Ls) + len(acc) + 3
    pk.f_status = np.zeros(pk.nslots, np.int32)
    pk.f_status[len(acc):] = POISON32
    for k, v in chunk.get("f_status", {}).items():
        pk.f_status[k + shift] = v
    filled = chunk.get("count", len(acc))
    pk.count = np.asarray([filled if filled < 0 else min(filled + shift, len(acc)), filled if filled < 0 else sum(Ls)], np.int64)
    pk.box_base = BOX_BASE
    pk.ops_new = np.full(pk.ops_bytes, POISON8, np.uint8)
    pk.idx_new = np.full(pk.ops_bytes, POISON32, np.int32)
    for name in ("ops_new_len", "idx_new_len", "status"):
        setattr(pk, name, np.full(pk.nprob + 1, POISON32, np.int32))
    for name in ("refined", "slot"):
        setattr(pk, name, np.full(pk.nlines + 1, POISON32, np.int32))
    return pk


INPUTS = ("ops", "ops_off", "ops_len", "t_off", "o_off", "o_line", "line_first", "idx", "table", "h_status", "acc_line", "L",
          "lab_off", "count", "f_status", "plain")
OUTPUTS = ("ops_new", "ops_new_len", "idx_new", "idx_new_len", "refined", "slot", "status")


def call(lib, pk, ptr, stream=None, **over):
    """ta_refine_columns on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to replace"""
    a = dict(ops_bytes=pk.ops_bytes, t_len=pk.t_len, o_len=pk.o_len, nprob=pk.nprob, nlines=pk.nlines, nslots=pk.nslots,
             label_cap=pk.label_cap, box_base=pk.box_base)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    return lib.ta_refine_columns(a["ops"], a["ops_off"], a["ops_len"], a["ops_bytes"], a["t_off"], a["o_off"], a["t_len"],
                                 a["o_len"], a["nprob"], a["o_line"], a["line_first"], a["idx"], a["table"], a["h_status"],
                                 a["nlines"], a["acc_line"], a["L"], a["lab_off"], a["count"], a["nslots"], a["label_cap"],
                                 a["f_status"], a["plain"], a["box_base"], a["ops_new"], a["ops_new_len"], a["idx_new"],
                                 a["idx_new_len"], a["refined"], a["slot"], a["status"], stream)


def want(pk):
    """the checker's answer for a packed chunk, page by page: [(status, ops, idx)], refined [nlines], slot [nlines]"""
    filled = max(0, min(int(pk.count[0]), pk.nslots))
    slots = {int(pk.acc_line[k]): (k, int(pk.L[k]), int(pk.lab_off[k]), int(pk.f_status[k])) for k in range(filled)}
    table = pk.table.tolist()
    per_page, refined, slot = [], np.zeros(pk.nlines, np.int32), np.full(pk.nlines, -1, np.int32)
    for p, pg in enumerate(pk.pages):
        o_line = pk.o_line[pk.o_off[p]:pk.o_off[p + 1]]
        st, ops, idx, mine = R.refine_page(pg["ops"], pg["idx"], o_line, pg["n"], int(pk.line_first[p]), int(pk.line_first[p + 1]),
                                           table, slots, bool(pg["plain"]), pk.box_base, pk.label_cap, pg["harvest"] == 0)
        per_page.append((st, np.asarray(ops, np.uint8), np.asarray(idx, np.int32)))
        for l, k in mine.items():
            refined[l], slot[l] = 1, k
    return per_page, refined, slot


def compare(pk, answer=None):
    """every output word against the checker; what lies outside the pages' results must still be poison (behind the idx
    rows of a page that was refused the region's contents are not specified)"""
    per_page, refined, slot = answer or want(pk)
    assert pk.status[:pk.nprob].tolist() == [st for st, _, _ in per_page]
    assert pk.refined[:pk.nlines].tolist() == refined.tolist() and pk.slot[:pk.nlines].tolist() == slot.tolist()
    assert pk.refined[pk.nlines] == POISON32 and pk.slot[pk.nlines] == POISON32
    for name in ("ops_new_len", "idx_new_len", "status"):
        assert getattr(pk, name)[pk.nprob] == POISON32
    seen8, seen32 = np.zeros(pk.ops_bytes, bool), np.zeros(pk.ops_bytes, bool)
    for p, (st, ops, idx) in enumerate(per_page):
        r0, r1 = int(pk.ops_off[p]), int(pk.ops_off[p + 1])
        assert pk.ops_new_len[p] == len(ops) and pk.idx_new_len[p] == len(idx), p
        assert np.array_equal(pk.ops_new[r0:r0 + len(ops)], ops), p
        assert np.array_equal(pk.idx_new[r0:r0 + len(idx)], idx), p
        seen8[r0:r0 + len(ops)] = True
        seen32[r0:(r1 if st else r0 + len(idx))] = True
    assert (pk.ops_new[~seen8] == POISON8).all() and (pk.idx_new[~seen32] == POISON32).all()
