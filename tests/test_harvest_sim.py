"""The harvest kernels without a GPU: tests/native/sim_harvest.cpp compiles csrc/ta_harvest.hip ITSELF for the host (a
wave = 64 coroutines that meet at every ballot / barrier; tests/native/hipshim) and every integer it writes must equal
the plain-Python checker tests/harvest_ref.py -- the pages, refusals and packing that tests/test_harvest_gpu.py drives
through the real kernels, with the alignments of the aligner's CPU restatement, and random column sequences on top."""
import numpy as np
import pytest

import harvest_cases as C
import harvest_ref as R
import simlib
from text_alignment_amd import _abi

POISON = 0xEE


@pytest.fixture(scope="module")
def sim():
    deps = [simlib.HIPSHIM, simlib.CSRC + "ta_harvest.hip", simlib.HEADER]
    return _abi.bind(simlib.load("harvest", deps, include=["hipshim"]),
                     ["ta_harvest_workspace_bytes", "ta_harvest_lines", "ta_harvest_pack"])


def _aligned16(nbytes):
    raw = np.full(nbytes + 16, POISON, dtype=np.uint8)
    shift = (-raw.ctypes.data) % 16
    return raw[shift:shift + nbytes]


def _run(lib, pages, ops_list, asm, num=C.NUM, den=C.DEN, t_base=3, o_base=5, ops_len=None, o_line=None):
    """the host twin of harvest.harvest_alignment: the arrays laid out as an NWBatch lays them (alignment columns
    right-aligned in regions of n + m bytes, poison in front), offsets that do not start at 0, every output and the
    workspace poisoned"""
    nprob = len(pages)
    n = np.asarray([len(pg["t"]) for pg in pages], dtype=np.int64)
    m = np.asarray([len(pg["o"]) for pg in pages], dtype=np.int64)
    t_off = np.concatenate([[t_base], t_base + np.cumsum(n)]).astype(np.int64)
    o_off = np.concatenate([[o_base], o_base + np.cumsum(m)]).astype(np.int64)
    ops_off = np.concatenate([[0], np.cumsum(n + m)]).astype(np.int64)
    ops = np.full(int(ops_off[-1]) + 16, POISON, dtype=np.uint8)
    lens = np.zeros(nprob + 1, dtype=np.int32)
    for p, o in enumerate(ops_list):
        end = int(ops_off[p + 1])
        ops[end - len(o):end] = o
        lens[p] = len(o)
    if ops_len:
        for p, v in ops_len.items():
            lens[p] = v
    pad = lambda base, a, fill: np.concatenate([np.full(base, fill, np.int32), a, np.full(4, fill, np.int32)])    # noqa: E731
    t_codes = pad(t_base, np.concatenate([pg["t"] for pg in pages]), 77)
    o_codes = pad(o_base, np.concatenate([pg["o"] for pg in pages]), 78)
    t_class = pad(t_base, asm["t_class"], 1)
    ol = pad(o_base, asm["o_line"] if o_line is None else o_line, -5)
    nlines = int(asm["line_first"][-1])
    T = np.concatenate([asm["T"], [0]]).astype(np.int32)
    ws_bytes = lib.ta_harvest_workspace_bytes(nlines, int(t_off[-1]), int(o_off[-1]))
    assert ws_bytes > 0
    ws = _aligned16(ws_bytes)
    table = np.full((nlines + 1, R.FIELDS), -7, dtype=np.int32)
    status = np.full(nprob + 1, -7, dtype=np.int32)
    lf = np.ascontiguousarray(asm["line_first"], dtype=np.int64)
    rc = lib.ta_harvest_lines(ops.ctypes.data, ops_off.ctypes.data, lens.ctypes.data, ops.size, t_codes.ctypes.data,
                              t_off.ctypes.data, o_codes.ctypes.data, o_off.ctypes.data, nprob, ol.ctypes.data,
                              lf.ctypes.data, t_class.ctypes.data, T.ctypes.data, nlines, num, den, t_off.ctypes.data,
                              o_off.ctypes.data, lf.ctypes.data, ws.ctypes.data, ws.size, table.ctypes.data,
                              status.ctypes.data, None)
    assert rc == 0
    assert (table[nlines] == -7).all() and status[nprob] == -7
    cap = max(int(t_off[-1]), 1)
    acc_line = np.full(nlines + 1, -7, dtype=np.int32)
    L = np.full(nlines + 1, -7, dtype=np.int32)
    lab_off = np.full(nlines + 1, -7, dtype=np.int64)
    labels = np.full(cap + 1, -7, dtype=np.int32)
    count = np.full(2, -7, dtype=np.int64)
    rc = lib.ta_harvest_pack(table.ctypes.data, ws.ctypes.data, ws.size, t_class.ctypes.data, int(t_off[-1]), nlines, cap,
                             acc_line.ctypes.data, L.ctypes.data, lab_off.ctypes.data, labels.ctypes.data,
                             count.ctypes.data, None)
    assert rc == 0
    k, nl = int(count[0]), int(count[1])
    assert (acc_line[max(k, 0):] == -7).all() and (labels[max(nl, 0):] == -7).all()
    return table[:nlines], status[:nprob], (acc_line[:k].tolist(), L[:k].tolist(), lab_off[:k].tolist(), labels[:nl].tolist())


def _oracle_ops(pages, params):
    from oracle import nw_oracle
    return [np.asarray(nw_oracle.align_ids(pg["t"], pg["o"], params), dtype=np.uint8) for pg in pages]


def _random_ops(rng, n, m):
    """any monotone path is a page the rule must handle: n transcript and m OCR characters in runs of pairs and gaps"""
    ops, i, j = [], 0, 0
    while i < n or j < m:
        kind = int(rng.integers(0, 3))
        run = int(rng.integers(1, 9)) if rng.random() < 0.9 else int(rng.integers(30, 150))
        for _ in range(run):
            if kind == 0 and i < n and j < m:
                ops.append(0); i += 1; j += 1
            elif kind == 1 and i < n:
                ops.append(1); i += 1
            elif kind == 2 and j < m:
                ops.append(2); j += 1
    return np.asarray(ops, dtype=np.uint8)


def test_host_build_equals_the_checker_on_the_gpu_tests_pages(sim):
    for pages, params in ((C.sized_pages(), C.STIFF), (C.random_pages(), C.DEFAULT)):
        ops = _oracle_ops(pages, params)
        if params is C.STIFF:
            cols = [len(o) for o in ops]
            assert cols[:len(C.SIZES)] == list(C.SIZES)
        asm = C.assemble(pages, ops)
        want_table, refused, want_pack = C.expected(asm)
        table, status, packed = _run(sim, pages, ops, asm)
        assert not any(refused) and (status == 0).all()
        assert np.array_equal(table, want_table)
        assert packed == tuple(want_pack)
    assert len(want_pack[0]) > 0 and (want_table[:, 0] != 0).any()


def test_host_build_on_the_worked_example(sim):
    """the issue's hand-checked page, behind another page so that its lines are 2 .. 5 of the batch"""
    from test_harvest import WORKED, _classes
    tra = "".join(s[0] for s in WORKED)
    ocr = "".join(s[1] for s in WORKED)
    text = tra.replace("#", "")
    ids = lambda s: np.frombuffer(s.encode("latin-1"), dtype=np.uint8).astype(np.int32)      # noqa: E731
    worked = {"t": ids(text), "o": ids(ocr.replace("#", "")), "lines": 4, "T": np.asarray([40, 40, 40, 19], np.int32),
              "o_line": np.asarray([s[2] for s in WORKED for ch in s[1] if ch != "#"], np.int32),
              "t_class": np.asarray(_classes(text), np.int32)}
    ops = np.asarray([1 if o == "#" else (2 if t == "#" else 0) for t, o in zip(tra, ocr)], dtype=np.uint8)
    first = C.random_pages(seed=2, count=1)[0]
    first["lines"], first["T"], first["o_line"] = 2, np.asarray([30, 30], np.int32), np.zeros(len(first["o"]), np.int32)
    pages, ops_list = [first, worked], [_oracle_ops([first], C.DEFAULT)[0], ops]
    asm = C.assemble(pages, ops_list)
    table, status, packed = _run(sim, pages, ops_list, asm)
    assert table[2:].tolist() == [[12, 3, 12, 11, 1, 0, 0, 2], [6, 16, 8, 6, 0, 2, 0, 3], [3, 0, 0, 0, 0, 0, 0, 0],
                                  [4, 27, 9, 8, 1, 0, 1, 3]]
    assert np.array_equal(table, C.expected(asm)[0]) and (status == 0).all()


def test_host_build_on_random_column_sequences(sim):
    rng = np.random.default_rng(23)
    pages, ops = [], []
    for k in range(50):
        n, m = int(rng.integers(0, 400)), int(rng.integers(0, 400))
        t = C._words(rng, n)
        o = C._words(rng, m)
        nl = int(rng.integers(1, 8))
        empty = tuple(l for l in range(1, nl) if rng.random() < 0.2)
        pages.append(C._page(rng, t, o, nl, empty=empty, drop=k % 5 == 0))
        ops.append(_random_ops(rng, n, m))
    asm = C.assemble(pages, ops)
    for num, den in ((4, 5), (1, 3), (1, 1)):
        want_table, _, want_pack = C.expected(asm, num, den)
        table, status, packed = _run(sim, pages, ops, asm, num, den)
        assert (status == 0).all() and np.array_equal(table, want_table)
        assert packed == tuple(want_pack)
    assert len({int(r) for r in want_table[:, 0]}) > 8              # many different reason sets were reached


def test_host_build_refuses_pages_through_their_data(sim):
    pages = C.random_pages(seed=9, count=7)
    ops = _oracle_ops(pages, C.DEFAULT)
    asm = C.assemble(pages, ops)
    lf = asm["line_first"]
    pick = [p for p, pg in enumerate(pages) if len(pg["o"]) >= 4 and pg["lines"] >= 2][:2]
    assert len(pick) == 2
    a, b = pick
    oa = int(sum(len(pg["o"]) for pg in pages[:a])), int(sum(len(pg["o"]) for pg in pages[:b]))
    # an unfinished traceback on page 0, a decreasing o_line on page a, a line outside the page on page b
    o_line = asm["o_line"].copy()
    o_line[oa[0]] = lf[a] + 1                                         # the page's second line, then its first
    o_line[oa[0] + 1:oa[0] + len(pages[a]["o"])] = lf[a]
    o_line[oa[1] + 2] = lf[b + 1]                                     # the first line of the NEXT page
    ref = [dict(pg) for pg in asm["ref"]]
    ref[0]["unfinished"] = True
    ref[a]["o_line"] = o_line[oa[0]:oa[0] + len(pages[a]["o"])].tolist()
    ref[b]["o_line"] = o_line[oa[1]:oa[1] + len(pages[b]["o"])].tolist()
    want_table, refused = R.harvest_batch(ref, asm["T"].tolist(), C.NUM, C.DEN)
    assert [p for p, r in enumerate(refused) if r] == sorted({0, a, b})
    table, status, packed = _run(sim, pages, ops, asm, ops_len={0: -1}, o_line=o_line)
    assert np.array_equal(table, want_table)
    assert status.tolist() == [1 if p == 0 else (3 if p in (a, b) else 0) for p in range(len(pages))]
    assert packed == tuple(R.pack(want_table, ref))
    for p in (0, a, b):
        assert (table[lf[p]:lf[p + 1]] == [R.PAGE, 0, 0, 0, 0, 0, 0, 0]).all()
    # columns that do not add up: a length one short, one beyond the region, a column code above 2
    longest = int(np.argmax([len(o) for o in ops]))
    for bad_len in (len(ops[longest]) - 1, len(pages[longest]["t"]) + len(pages[longest]["o"]) + 1):
        table, status, _ = _run(sim, pages, ops, asm, ops_len={longest: bad_len})
        assert status[longest] == 2 and (table[lf[longest]:lf[longest + 1], 0] == R.PAGE).all()
        assert sum(status != 0) == 1
    ops2 = [o.copy() for o in ops]
    ops2[longest][len(ops2[longest]) // 2] = 3
    table, status, _ = _run(sim, pages, ops2, asm)
    assert status[longest] == 2 and sum(status != 0) == 1


def test_host_side_refusals_come_before_any_launch(sim):
    one = np.zeros(4, dtype=np.int64)
    p = one.ctypes.data

    def call(nprob=1, nlines=0, num=4, den=5, t_off=(0, 0), o_off=(0, 0), lf=(0, 0), ws_bytes=4096, ws=None):
        t_off, o_off, lf = (np.asarray(a, dtype=np.int64) for a in (t_off, o_off, lf))
        buf = _aligned16(4096)
        return sim.ta_harvest_lines(p, p, p, 16, p, p, p, p, nprob, p, p, p, p, nlines, num, den, t_off.ctypes.data,
                                    o_off.ctypes.data, lf.ctypes.data, buf.ctypes.data if ws is None else ws, ws_bytes,
                                    p, p, None)
    assert call() == 0 and call(nprob=-1) == -1 and call(nlines=-1) == -1
    assert call(num=0) == -1 and call(den=0) == -1 and call(num=6, den=5) == -1 and call(num=1, den=10 ** 6 + 1) == -1
    assert call(t_off=(5, 3)) == -1 and call(o_off=(0, -1)) == -1 and call(lf=(0, 1)) == -1 and call(lf=(1, 0)) == -1
    assert call(nlines=2, lf=(0, 2), ws_bytes=8) == -1                  # a workspace too small
    assert call(ws=_aligned16(64).ctypes.data + 4) == -1                # ... or not aligned
    assert call(t_off=(0, (1 << 24) + 1)) == -4 and call(nlines=(1 << 24) + 1, lf=(0, (1 << 24) + 1)) == -4
    assert sim.ta_harvest_workspace_bytes(-1, 0, 0) == -1 and sim.ta_harvest_workspace_bytes((1 << 24) + 1, 0, 0) == -4
    assert sim.ta_harvest_pack(p, p, 64, p, 0, -1, 1, p, p, p, p, p, None) == -1
    assert sim.ta_harvest_pack(p, None, 64, p, 0, 0, 1, p, p, p, p, p, None) == -1
    assert sim.ta_harvest_pack(p, _aligned16(64).ctypes.data, 8, p, 0, 4, 1, p, p, p, p, p, None) == -1
