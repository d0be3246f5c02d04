"""The cases of ta_confidence_pages that tests/test_refine_conf_sim.py (the host build of csrc/ta_refine_conf.hip) and
tests/test_forced_conf_lines_gpu.py (the real kernel) share, the layout both drive it with, and the checker's answers.

A case is (name, [page, ...]); a page is {"n": transcript characters, "lines": [{"refined", "tf", "L", "slot" (False: the
line has no packed slot), "status" (its slot's confidence status), "conf" (None: seeded values)}], "syls": [(first,
last)]}.  `pack` lays a chunk out with a small good page in FRONT of the case's pages, no offset at 0, gaps between the
slots' labels, two slots behind count[0] whose arrays are poison, and every output poisoned.
"""
import numpy as np

import refine_conf_ref as R
from text_alignment_amd import _abi

POISON32, POISON64 = -0x21212122, -0x2121212121212122
NO = R.NO_CONFIDENCE


def bind(lib):
    return _abi.bind(lib, ["ta_confidence_pages"])


def line(refined, tf, L, slot=True, status=0, conf=None):
    return dict(refined=refined, tf=tf, L=L, slot=slot, status=status, conf=conf)


def rand_page(rng, nl, lmax, p_refined=0.7):
    """nl lines of 1 .. lmax kept characters one after the other with gaps, syllables of 1 .. 4 characters with gaps"""
    lines, at = [], int(rng.integers(0, 3))
    for _ in range(nl):
        L = int(rng.integers(1, lmax + 1))
        lines.append(line(bool(rng.random() < p_refined), at, L))
        at += L + int(rng.integers(0, 4))
    n = at + int(rng.integers(0, 3))
    syls, at = [], 0
    while at < n:
        w = int(rng.integers(1, 5))
        if at + w <= n and rng.random() < 0.85:
            syls.append((at, at + w - 1))
        at += w
    return dict(n=n, lines=lines, syls=syls)


def front():
    return dict(n=6, lines=[line(True, 1, 3, conf=[7, -2, 9]), line(False, 4, 2)], syls=[(0, 1), (2, 4), (5, 5)])


def good(rng):
    return rand_page(rng, 3, 9)


def cases():
    rng = np.random.default_rng(1411)
    out = [("no refined line", [dict(n=9, lines=[line(False, 0, 4), line(False, 5, 3)], syls=[(0, 3), (5, 7)])]),
           # characters 0 - 3 on a refined line, 5 - 7 on one that is not: the syllable 3 .. 5 spans both
           ("a syllable across a refined and an unrefined line",
            [dict(n=9, lines=[line(True, 0, 4, conf=[50, 40, 30, 20]), line(False, 5, 3)], syls=[(0, 1), (3, 5), (6, 7)])]),
           ("a syllable with no valued character",
            [dict(n=9, lines=[line(True, 0, 4), line(False, 5, 3)], syls=[(4, 4), (5, 7), (0, 3)])]),
           ("an empty transcript", [dict(n=0, lines=[line(False, 0, 0, slot=False)], syls=[]), good(rng)]),
           ("a page without lines", [dict(n=5, lines=[], syls=[(0, 4)]), good(rng)]),
           ("a page off the array path", [dict(n=12, lines=[line(False, 0, 5), line(False, 6, 6)], syls=[]), good(rng)]),
           ("zero and negative values",
            [dict(n=8, lines=[line(True, 0, 3, conf=[0, 5, -3]), line(True, 4, 4, conf=[-(1 << 40), 0, 0, NO + 1])],
                  syls=[(0, 0), (1, 2), (0, 2), (3, 3), (4, 4), (5, 6), (4, 7), (7, 7)])]),
           ("an unrefined line with a refused slot", [dict(n=9, lines=[line(True, 0, 4), line(False, 5, 3, status=5)],
                                                           syls=[(0, 8)])]),
           ("more than 64 lines, syllables and characters", [rand_page(rng, 70, 3), rand_page(rng, 3, 150)]),
           ("three pages", [rand_page(rng, 5, 20), rand_page(rng, 1, 4, p_refined=1.0), rand_page(rng, 9, 30)])]
    for name, bad in (("a syllable behind the page's characters", dict(n=9, lines=[line(True, 0, 4)], syls=[(0, 3), (7, 9)])),
                      ("a syllable in front of the page's characters", dict(n=9, lines=[line(True, 0, 4)], syls=[(-1, 3)])),
                      ("a syllable whose range is turned round", dict(n=9, lines=[line(True, 0, 4)], syls=[(0, 3), (6, 5)])),
                      ("a table row behind the page's characters", dict(n=9, lines=[line(True, 0, 4), line(True, 6, 4)],
                                                                        syls=[(0, 3)])),
                      ("a table row in front of the page's characters", dict(n=9, lines=[line(True, -1, 4)], syls=[(0, 3)])),
                      ("a refined line without a slot", dict(n=9, lines=[line(True, 0, 4), line(True, 5, 3, slot=False)],
                                                             syls=[(0, 3)])),
                      ("a refined line the confidence skipped", dict(n=9, lines=[line(True, 0, 4), line(True, 5, 3, status=5)],
                                                                     syls=[(0, 3)])),
                      ("a refined line the confidence refused", dict(n=9, lines=[line(True, 0, 4, status=1)], syls=[(0, 3)]))):
        out.append((name, [good(rng), bad, good(rng)]))
    return out


class Packed(object):
    pass


def pack(pages, seed=0, count=None):
    """host arrays of one call, the front page first.  count: the device's count[0] if not the number of slots"""
    rng = np.random.default_rng(seed)
    pages = [front()] + list(pages)
    pk = Packed()
    pk.pages, pk.nprob = pages, len(pages)
    n = np.asarray([pg["n"] for pg in pages], np.int64)
    ns = np.asarray([len(pg["syls"]) for pg in pages], np.int64)
    pk.t_off = np.concatenate([[3], 3 + np.cumsum(n)]).astype(np.int64)
    pk.syl_off = np.concatenate([[2], 2 + np.cumsum(ns)]).astype(np.int64)
    pk.t_len, pk.nsyl = int(pk.t_off[-1]) + 2, int(pk.syl_off[-1]) + 3
    pk.line_first = np.concatenate([[0], np.cumsum([len(pg["lines"]) for pg in pages])]).astype(np.int64)
    pk.nlines = int(pk.line_first[-1])
    pk.table = np.full((pk.nlines + 1, 8), 7, np.int32)
    pk.refined = np.full(pk.nlines + 1, POISON32, np.int32)
    pk.slot = np.full(pk.nlines + 1, POISON32, np.int32)
    pk.syl_first = np.full(pk.nsyl, -9, np.int32)
    pk.syl_last = np.full(pk.nsyl, 1 << 30, np.int32)
    Ls, offs, status, conf, off = [], [], [], [], 4
    for p, pg in enumerate(pages):
        for j, (f, l) in enumerate(pg["syls"]):
            pk.syl_first[pk.syl_off[p] + j], pk.syl_last[pk.syl_off[p] + j] = f, l
        for j, ln in enumerate(pg["lines"]):
            q = int(pk.line_first[p]) + j
            pk.table[q, :3] = [0 if ln["refined"] else 2, ln["tf"], ln["L"]]
            pk.refined[q], pk.slot[q] = int(ln["refined"]), -1
            if ln["slot"]:
                pk.slot[q] = len(Ls) if ln["refined"] else -1
                Ls.append(ln["L"])
                offs.append(off)
                status.append(ln["status"])
                conf.append((off, ln["conf"] if ln["conf"] is not None else
                             rng.integers(-5, 1 << 22, size=ln["L"]) * rng.integers(0, 2, size=ln["L"])))
                off += ln["L"] + 1
    pk.label_cap = off + 3
    pk.confidence = np.full(pk.label_cap, POISON64, np.int64)
    for o, c in conf:
        pk.confidence[o:o + len(c)] = c
    pk.nslots = len(Ls) + 2
    pk.L = np.asarray(Ls + [3, 3], np.int32)
    pk.lab_off = np.asarray(offs + [1 << 40] * 2, np.int64)
    pk.c_status = np.asarray(status + [POISON32] * 2, np.int32)
    pk.count = np.asarray([len(Ls) if count is None else count, int(sum(Ls))], np.int64)
    pk.char_conf = np.full(pk.t_len, POISON64, np.int64)
    pk.syl_conf = np.full(pk.nsyl, POISON64, np.int64)
    pk.status = np.full(pk.nprob + 1, POISON32, np.int32)
    return pk


INPUTS = ("confidence", "lab_off", "L", "count", "c_status", "table", "line_first", "refined", "slot", "t_off", "syl_first",
          "syl_last", "syl_off")
OUTPUTS = ("char_conf", "syl_conf", "status")


def call(lib, pk, ptr, stream=None, **over):
    """ta_confidence_pages on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to replace"""
    a = dict(nslots=pk.nslots, label_cap=pk.label_cap, nlines=pk.nlines, t_len=pk.t_len, nsyl=pk.nsyl, nprob=pk.nprob)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    return lib.ta_confidence_pages(a["confidence"], a["lab_off"], a["L"], a["count"], a["c_status"], a["nslots"], a["label_cap"],
                                   a["table"], a["line_first"], a["refined"], a["slot"], a["nlines"], a["t_off"], a["t_len"],
                                   a["syl_first"], a["syl_last"], a["syl_off"], a["nsyl"], a["nprob"], a["char_conf"],
                                   a["syl_conf"], a["status"], stream)


def want(pk):
    """the checker's answer for a packed chunk, page by page: [(status, char_conf, syl_conf)]"""
    filled = max(0, min(int(pk.count[0]), pk.nslots))
    slots = [(int(pk.L[k]), int(pk.lab_off[k]), int(pk.c_status[k])) for k in range(pk.nslots)]
    out = []
    for p, pg in enumerate(pk.pages):
        a, b = int(pk.syl_off[p]), int(pk.syl_off[p + 1])
        out.append(R.confidence_page(pg["n"], int(pk.line_first[p]), int(pk.line_first[p + 1]), pk.table.tolist(),
                                     pk.refined.tolist(), pk.slot.tolist(), slots, filled, pk.confidence.tolist(), pk.label_cap,
                                     pk.syl_first[a:b].tolist(), pk.syl_last[a:b].tolist()))
    return out


def compare(pk, answer=None, skip=()):
    """every output word against the checker; a refused page's words, the words of the pages in `skip` and everything
    outside the pages must still be poison"""
    answer = answer or want(pk)
    cc, sc = np.full(pk.t_len, POISON64, np.int64), np.full(pk.nsyl, POISON64, np.int64)
    st = np.full(pk.nprob + 1, POISON32, np.int32)
    for p, (status, c, s) in enumerate(answer):
        if p in skip:
            continue
        st[p] = status
        if status == R.OK:
            cc[pk.t_off[p]:pk.t_off[p + 1]] = c
            sc[pk.syl_off[p]:pk.syl_off[p + 1]] = s
    for p in skip:
        st[p] = pk.status[p]                               # the caller checks these
    assert pk.status.tolist() == st.tolist()
    assert np.array_equal(pk.char_conf, cc) and np.array_equal(pk.syl_conf, sc)
