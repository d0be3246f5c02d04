"""The cases of ta_page_windows (csrc/ta_page_windows.hip) that tests/test_page_windows_sim.py
(the host build of the kernel) and tests/test_page_windows_gpu.py (the real kernel) share, the layout they drive it with
and the expected answers: forced.page_scope_eligibility / forced.page_windows, which tests/test_forced_page.py pins to the
checker tests/forced_page_ref.py.

A page is a dict: plain (bool), status (the harvest's), classes (int32 per transcript character), rows (lines, 8) int32
harvest rows, T (timesteps per line).  A case is (name, margin, [page, ...]).  `pack` lays a case out behind a page in
front, so that no page of the case has an offset of 0, with every output poisoned.
"""
import numpy as np

from text_alignment_amd import _abi

POISON32 = -0x35353536                  # 0xCACACACA
C = _abi.CONSTANTS
FIELDS, EMPTY, PAGE = C["TA_HARVEST_FIELDS"], C["TA_HARVEST_EMPTY"], C["TA_HARVEST_PAGE"]
MAX_TARGET = C["TA_FORCED_MAX_TARGET"]
BOUNDS = C["TA_PAGE_WINDOWS_BOUNDS"]
EXAMPLE = [[12, 3, 12], [6, 16, 8], [3, 0, 0], [4, 27, 9]]          # DESIGN.md section 14.6's worked example: n = 37


def bind(lib):
    return _abi.bind(lib, ["ta_page_windows"])


def page(rows3, n, T=None, plain=True, status=0, classes=None):
    rows3 = np.asarray(rows3, dtype=np.int32).reshape(-1, 3)
    rows = np.zeros((len(rows3), FIELDS), np.int32)
    rows[:, :3] = rows3
    rows[:, 3:] = 7                     # counts the kernel must not read
    T = np.full(len(rows), max(2 * n // max(len(rows), 1) + 3, 1), np.int32) if T is None else np.asarray(T, np.int32)
    classes = np.full(n, 5, np.int32) if classes is None else np.asarray(classes, np.int32)
    return dict(plain=bool(plain), status=int(status), classes=classes, rows=rows, T=T)


def chain(nl, L=2, gap=0):
    """nl lines whose cores follow each other: L characters each, `gap` characters between them; (rows, n)"""
    rows = [[0, k * (L + gap), L] for k in range(nl)]
    return rows, nl * (L + gap)


def random_page(rng):
    nl, n = int(rng.integers(1, 9)), int(rng.integers(1, 2500))
    rows = np.zeros((nl, 3), np.int64)
    rows[:, 0] = rng.choice([0, 1, 2, 4, 8, 64, 65, 6], size=nl)
    rows[:, 1] = np.sort(rng.integers(0, n, size=nl)) if rng.integers(2) else rng.integers(0, n, size=nl)
    rows[:, 2] = np.minimum(rng.integers(0, 700, size=nl), n - rows[:, 1])
    T = rng.integers(1, 2 * n // nl + 40, size=nl)
    classes = np.full(n, 3, np.int32)
    if rng.integers(8) == 0:
        classes[int(rng.integers(n))] = 0
    return page(rows, n, T=T, plain=rng.integers(8) != 0, status=int(rng.integers(8) == 0) * 2, classes=classes)


def cases():
    out = []
    for margin in (0, 2, 16):
        out.append(("the worked example, margin %d" % margin, margin, [page(EXAMPLE, 37, T=[40, 40, 40, 19])]))
    for nl in (1, 63, 64, 65, 128, 129):                  # the tile carries
        rows, n = chain(nl, L=2, gap=1)
        out.append(("%d lines" % nl, 1, [page(rows, n)]))
        # every fifth line EMPTY, and a late line that starts early: the latest core and both running bounds cross the tiles
        rows = [[EMPTY if k % 5 == 4 else 0, r[1], r[2]] for k, r in enumerate(rows)]
        if nl > 2:
            rows[nl - 2] = [0, 1, 2]
        out.append(("%d lines with empty ones" % nl, 3, [page(rows, n)]))
    rows, n = chain(6, L=3, gap=2)
    e = lambda ks: [[EMPTY if k in ks else r[0], r[1], r[2]] for k, r in enumerate(rows)]            # noqa: E731
    out.append(("leading, trailing and all-EMPTY lines", 2, [page(e({0, 1}), n), page(e({4, 5}), n), page(e(set(range(6))), n),
                                                             page(e({0, 2, 5}), n)]))
    out.append(("a PAGE row", 2, [page([[0, 0, 5], [PAGE, 0, 0], [PAGE | EMPTY, 3, 3], [0, 9, 4]], 13)]))
    out.append(("a margin above n", 500, [page(rows, n), page(EXAMPLE, 37, T=[40, 40, 40, 19])]))
    # the widest window: 1023 characters pass, 1024 do not
    out.append(("widths 1023 and 1024", 0, [page([[0, 0, 1023], [0, 1023, 10]], 1033, T=[2100, 30]),
                                           page([[0, 0, 1024], [0, 1024, 10]], 1034, T=[2100, 30]),
                                           page([[0, 0, 1000], [0, 1000, 10]], 1010, T=[2100, 30])]))
    out.append(("widths 1023 and 1024 through the margin", 7, [page([[0, 0, 1016], [0, 1016, 100]], 1116, T=[2100, 300]),
                                                              page([[0, 0, 1017], [0, 1017, 100]], 1117, T=[2100, 300])]))
    out.append(("n against the frames", 2, [page(EXAMPLE, 37, T=[9, 9, 10, 9]), page(EXAMPLE, 37, T=[9, 9, 9, 9])]))
    cls0 = np.full(37, 5, np.int32)
    cls0[36] = 0
    T = [40, 40, 40, 19]
    wide = [[0, 0, 1024], [0, 1024, 10]]
    alone = [page(EXAMPLE, 37, T=T, plain=False), page(EXAMPLE, 37, T=T, status=2), page(EXAMPLE, 37, T=T, classes=cls0),
             page(EXAMPLE, 0, T=T), page(np.zeros((0, 3)), 37, T=[]), page(wide, 1034, T=[2100, 30]),
             page(EXAMPLE, 37, T=[9, 9, 9, 9])]
    out.append(("each reason alone", 2, alone))
    cls0w = np.full(1034, 5, np.int32)
    cls0w[0] = 0
    pairs = [page(EXAMPLE, 37, T=T, plain=False, status=2),                        # NOT_PLAIN over HARVEST
             page(EXAMPLE, 37, T=T, status=3, classes=cls0),                       # HARVEST over CLASS0
             page(np.zeros((0, 3)), 37, T=[], classes=cls0),                       # CLASS0 over WINDOWS (no lines); a text
             page(np.zeros((0, 3)), 0, T=[]),                                     # without characters has no class 0: NO_TEXT over WINDOWS
             page(wide, 1034, T=[20, 3]),                                         # WINDOWS (width) over FRAMES
             page(EXAMPLE, 37, T=[9, 9, 9, 9], plain=False),                      # NOT_PLAIN over FRAMES
             page(wide, 1034, T=[20, 3], classes=cls0w)]                          # CLASS0 over WINDOWS and FRAMES
    out.append(("adjacent reasons together", 2, pairs))
    rng = np.random.default_rng(1414)
    for k in range(0, 300, 25):
        out.append(("random tables %d" % k, int(rng.choice([0, 1, 16, 300])), [random_page(rng) for _ in range(25)]))
    return out


def want(pages, margin):
    """[(reason, (lo, hi) or None)] from forced.page_scope_eligibility"""
    from text_alignment_amd import forced
    return [forced.page_scope_eligibility(pg["plain"], pg["status"], pg["classes"], pg["rows"], pg["T"], margin)
            for pg in pages]


class Packed(object):
    pass


INPUTS = ("table", "h_status", "line_first", "t_off", "t_class", "T", "plain")
OUTPUTS = ("lo", "hi", "reason")


def pack(pages, front=True):
    """host arrays of one call; front: a page of two lines in front, which is part of the call and of pk.pages"""
    if front:
        pages = [page([[0, 0, 3], [0, 4, 2]], 6)] + list(pages)
    pk = Packed()
    pk.pages = pages
    cat = lambda xs, dt, shape=(-1,): (np.concatenate(xs) if xs else np.zeros(0)).astype(dt).reshape(shape)       # noqa: E731
    pk.table = np.ascontiguousarray(cat([pg["rows"] for pg in pages], np.int32, (-1, FIELDS)))
    pk.T = cat([pg["T"] for pg in pages], np.int32)
    pk.t_class = cat([pg["classes"] for pg in pages], np.int32)
    pk.h_status = np.asarray([pg["status"] for pg in pages], np.int32)
    pk.plain = np.asarray([pg["plain"] for pg in pages], np.uint8)
    pk.line_first = np.concatenate([[0], np.cumsum([len(pg["rows"]) for pg in pages])]).astype(np.int64)
    pk.t_off = np.concatenate([[0], np.cumsum([len(pg["classes"]) for pg in pages])]).astype(np.int64)
    pk.npages, pk.nlines, pk.t_len = len(pages), int(pk.line_first[-1]), int(pk.t_off[-1])
    for name in ("table", "T", "t_class"):                # never a pointer to nothing
        if getattr(pk, name).size == 0:
            setattr(pk, name, np.zeros(FIELDS if name == "table" else 1, np.int32))
    pk.lo = np.full(max(pk.nlines, 1), POISON32, np.int32)
    pk.hi = np.full(max(pk.nlines, 1), POISON32, np.int32)
    pk.reason = np.full(max(pk.npages, 1), POISON32, np.int32)
    return pk


def call(lib, pk, ptr, m, stream=None, **over):
    """ta_page_windows on pk's arrays at margin m, `ptr(array name)` giving each [device] pointer; over: arguments to replace"""
    a = dict(npages=pk.npages, nlines=pk.nlines, t_len=pk.t_len, margin=m)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    return lib.ta_page_windows(a["table"], a["h_status"], a["line_first"], a["t_off"], a["t_class"], a["T"], a["plain"],
                               a["npages"], a["nlines"], a["t_len"], a["margin"], a["lo"], a["hi"], a["reason"], stream)


def check(pk, wanted):
    """every output against the expected answers; lo / hi of a page with a reason must still be poison"""
    for p, (reason, win) in enumerate(wanted):
        a, b = int(pk.line_first[p]), int(pk.line_first[p + 1])
        assert int(pk.reason[p]) == reason, (p, int(pk.reason[p]), reason)
        if reason == 0:
            assert np.array_equal(pk.lo[a:b], win[0]) and np.array_equal(pk.hi[a:b], win[1]), (p, pk.lo[a:b], win[0], pk.hi[a:b], win[1])
        else:
            assert win is None and (pk.lo[a:b] == POISON32).all() and (pk.hi[a:b] == POISON32).all(), p
    assert (pk.lo[pk.nlines:] == POISON32).all() and (pk.hi[pk.nlines:] == POISON32).all()
