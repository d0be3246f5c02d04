"""The gated page aligner with omission without a GPU: tests/native/sim_forced_page_omit_gated.cpp compiles
csrc/ta_forced_page_omit_gated.hip ITSELF for the host and every integer ta_forced_align_pages_omit_gated writes must equal
the checker tests/forced_page_omit_ref.py -- on EVERY case of tests/forced_page_omit_cases.py, with the gate, the caps and
the refusals of DESIGN.md section 14.17 on top.  tests/test_forced_page_omit_gated_gpu.py drives the same through the real
kernel."""
import ctypes

import numpy as np
import pytest

import forced_cases as C0
import forced_page_cases as PC
import forced_page_omit_cases as OC
import forced_page_omit_gated_cases as G
import forced_page_omit_ref as R
import simlib

UNIT = OC.UNIT
DEPS = [simlib.CSRC + "ta_forced_page_omit_gated.hip", simlib.CSRC + "forced_page_omit.h", simlib.CSRC + "forced_page_common.h",
        simlib.NAT + "sim_forced_omit_shim.h"] + C0.SIM_DEPS
EMPTY_PAGE = ([], [], [], [])


@pytest.fixture(scope="module")
def sim():
    return G.bind(simlib.load("forced_page_omit_gated", DEPS, include=["hipshim"]))


def _run(lib, pk, omit, **over):
    return G.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, omit, **over)


def widest(pg):
    return max(int(h) - int(l) for l, h in zip(pg[2], pg[3]))


@pytest.mark.parametrize("case", OC.cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("caps", ["widest window", "the text"])
def test_host_build_of_the_gated_kernel_equals_the_checker(sim, case, caps):
    """caps equal to the pages' widest windows, and min(n, 1023) as the pipeline passes them"""
    name, no, omit, pages = case
    slots = [(pg, 0, widest(pg) if caps == "widest window" else None) for pg in pages]
    pk = G.pack(sim, slots, no)
    assert _run(sim, pk, omit) == 0
    want = OC.want(name, pages, omit)
    assert [w[0] for w in want] == [R.OK] * len(pages)
    G.check(pk, want)
    if name.startswith(OC.STRICT):
        G.check(pk, OC.strict_want(pages))


def mixed(rng):
    """gated pages between good ones -- one with lines and text, one with no lines and no text, one with lines and no text
    --, two K in one call, a page whose windows need a wider variant than its cap, a page with more characters than frames"""
    no = 6
    narrow, wide = OC._page(rng, (12, 11), 8, (0, 3), (4, 8), no), OC._wide(rng, 70)
    crowded = OC._page(rng, (2, 1), 9, (0, 2), (6, 9), no)
    lines_only = ([OC.probs(rng, 5, no)], [], [0], [0])
    slots = [(narrow, 0, None), (OC._page(rng, (9, 9), 6, (0, 2), (4, 6), no), 3, None), (wide, 0, None), (EMPTY_PAGE, 5, None),
             (crowded, 0, None), (lines_only, 4, None), (OC._wide(rng, 70), 0, 60), (narrow, 0, 200), (wide, 6, 0)]
    want = G.want(slots, 2 * UNIT)
    want[6] = (R.BOUNDS, None, None)                     # K = 4 windows against a cap of 60 characters: K = 2
    return no, slots, want


def test_gate_caps_and_variants_in_one_call(sim):
    omit = 2 * UNIT
    no, slots, want = mixed(np.random.default_rng(1417))
    assert [w[0] for w in want] == [R.OK, G.SKIPPED, R.OK, G.SKIPPED, R.OK, G.SKIPPED, R.BOUNDS, R.OK, G.SKIPPED]
    pk = G.pack(sim, slots, no)
    assert sorted({PC.variant(widest(s[0])) for s in (slots[0], slots[2])}) == [2, 4]
    assert _run(sim, pk, omit) == 0
    G.check(pk, want)
    # a gated page's numbers are not read: rubbish in its windows, timesteps, rows and pieces changes nothing
    pk = G.pack(sim, slots, no)
    a = int(pk.line_first[1])
    pk.lo[a], pk.hi[a], pk.T[a], pk.row_off[a], pk.ws_off[a] = 7, -3, -1, 10 ** 12, -8
    host_T = G.pack(sim, slots, no).T
    assert _run(sim, pk, omit, T_host=host_T) == 0
    pk.ws_off[a] = G.pack(sim, slots, no).ws_off[a]      # (check() looks at the piece where it really lies)
    G.check(pk, want)
    # the device's cap decides on the device: a cap there below the windows' variant refuses the page, whatever the host's
    pk = G.pack(sim, slots, no)
    host_cap = pk.cap.copy()
    pk.cap[2] = 10
    assert _run(sim, pk, omit, cap_host=host_cap) == 0
    w = list(want)
    w[2] = (R.BOUNDS, None, None)
    G.check(pk, w)
    for bad in (-1, 1024):
        pk = G.pack(sim, slots, no)
        pk.cap[0] = bad
        assert _run(sim, pk, omit, cap_host=host_cap) == 0
        w = list(want)
        w[0] = (R.BOUNDS, None, None)
        G.check(pk, w)


def test_workspace_bytes(sim):
    ungated = OC.bind(simlib.load("forced_page_omit", [simlib.NAT + "sim_forced_omit_shim.h", simlib.CSRC + "ta_forced_page_omit.hip",
                                                       simlib.CSRC + "forced_page_omit.h", simlib.CSRC + "forced_page_common.h"]
                                  + C0.SIM_DEPS, include=["hipshim"]))
    T = np.asarray([3, 8, 9, 1], np.int32)
    f = lambda nl, cap: sim.ta_forced_page_omit_gated_workspace_bytes(nl, T.ctypes.data, cap)     # noqa: E731
    rows = lambda t, K: (2 * t if K == 32 else -(-t // (16 // K))) + -(-t // (32 // K))             # noqa: E731
    for cap in list(range(0, 1024, 7)) + [63, 64, 127, 128, 255, 256, 511, 512, 1023]:
        K = PC.variant(cap)
        assert f(4, cap) == sum(256 * rows(int(t), K) for t in T) == sum(
            sim.ta_forced_page_omit_gated_workspace_bytes(1, T[k:].ctypes.data, cap) for k in range(4))
        assert f(4, cap) == ungated.ta_forced_page_omit_workspace_bytes(4, T.ctypes.data, K)
    last = 0
    for cap in range(0, 1024):
        assert f(4, cap) >= last                         # never decreases with the cap: move rows and bit rows each
        last = f(4, cap)
    assert f(4, 0) == 256 * ((1 + 1 + 2 + 1) + 4) and f(4, 1023) == 256 * 3 * 21
    assert f(4, -1) == -1 and f(4, 1024) == -1 and f(0, 5) == -1
    assert sim.ta_forced_page_omit_gated_workspace_bytes(1, np.asarray([5001], np.int32).ctypes.data, 5) == -1
    assert sim.ta_forced_page_omit_gated_workspace_bytes(1, None, 5) == -1
    for t in (1, 2, 7, 15, 16, 17, 33, 1432, 5000):     # per line and per term, over every variant
        mv = [2 * t if K == 32 else -(-t // (16 // K)) for K in (2, 4, 8, 16, 32)]
        bt = [-(-t // (32 // K)) for K in (2, 4, 8, 16, 32)]
        assert mv == sorted(mv) and bt == sorted(bt)


def test_host_side_refusals_touch_nothing(sim):
    rng = np.random.default_rng(1418)
    pages = [OC._page(rng, (12, 11), 8, (0, 3), (4, 8), 6), OC._page(rng, (10, 9, 11), 9, (0, 1, 6), (5, 6, 9), 6)]
    slots = G.slots(pages)
    pk = G.pack(sim, slots, 6)
    omit = 2 * UNIT
    EINVAL, ELIMIT = -1, -4

    def arr(name, k, v):
        a = getattr(pk, name).copy()
        a[k] = v
        return a
    many = 6711                                           # more than 2^25 frames: 6711 lines of 5000 on page 0
    T_many = np.full(many + 3, 5000, np.int32)
    lf_many = np.asarray([0, many, many + 3], np.int64)
    sim.sim_forced_page_omit_gated_last_error.restype = ctypes.c_char_p
    last_error = sim.sim_forced_page_omit_gated_last_error
    null = "null pointer argument"
    price = "omit_q outside 0 .. TA_FORCED_OMIT_MAX"
    refusals = [
        (EINVAL, price, dict(omit_q=-1)), (EINVAL, price, dict(omit_q=(1 << 26) + 1)),
        (EINVAL, null, dict(probs=None)), (EINVAL, null, dict(frames=None)), (EINVAL, null, dict(gate=None)),
        (EINVAL, null, dict(cap=None)), (EINVAL, null, dict(cap_host=None)), (EINVAL, null, dict(lo=None)),
        (EINVAL, null, dict(workspace=None)), (EINVAL, null, dict(T_host=None)),
        (EINVAL, "negative size", dict(npages=-1)), (EINVAL, "negative size", dict(rows=-1)),
        (EINVAL, "no outside 2 .. TA_TRAIN_MAX_CLASSES", dict(no=1)), (EINVAL, "no outside 2 .. TA_TRAIN_MAX_CLASSES", dict(no=129)),
        (EINVAL, "the lines' timesteps exceed rows", dict(rows=int(pk.T.sum()) - 1)),
        (EINVAL, "the pages' texts exceed nlabels", dict(nlabels=int(pk.lab_off[-1]) - 1)),
        (EINVAL, "workspace smaller than the pages' ta_forced_page_omit_gated_workspace_bytes", dict(workspace_bytes=256)),
        (EINVAL, "workspace not 16-byte aligned", dict(workspace=pk.ws.ctypes.data + 4)),
        (EINVAL, "line_first does not run from 0 to nlines", dict(nlines=pk.nlines + 1)),
        (EINVAL, "line_first decreases", dict(line_first_host=np.asarray([0, 6, pk.nlines], np.int64))),
        (EINVAL, "lab_off decreases", dict(lab_off_host=arr("lab_off", 1, int(pk.lab_off[2]) + 1))),
        (EINVAL, "a line without timesteps", dict(T_host=arr("T", 1, 0))),
        (ELIMIT, "a line has more than TA_TRAIN_MAX_T timesteps", dict(T_host=arr("T", 1, 5001))),
        (EINVAL, "a negative cap", dict(cap_host=arr("cap", 1, -1))),
        (ELIMIT, "a cap of more than TA_FORCED_MAX_TARGET characters", dict(cap_host=arr("cap", 1, 1024))),
        (ELIMIT, "a page's text has more than 2^20 characters",
         dict(lab_off_host=arr("lab_off", 2, int(pk.lab_off[1]) + (1 << 20) + 1), nlabels=1 << 40)),
        (ELIMIT, "a page has more than 2^25 frames",
         dict(T_host=T_many, line_first_host=lf_many, nlines=many + 3, rows=1 << 40, workspace_bytes=1 << 40)),
    ]
    for code, text, over in refusals:
        assert _run(sim, pk, omit, **over) == code, (text, over)
        assert last_error().decode() == text, over
        assert (pk.frames == G.POISON32).all() and (pk.score == G.POISON64).all() and (pk.status == G.POISON32).all(), text
        assert (pk.ws == G.POISON_BYTE).all(), text
    assert _run(sim, pk, omit, npages=0) == 0 and (pk.status == G.POISON32).all()
    # exactly 2^20 characters is not the host's to refuse (the device then refuses the page: its windows do not end at n)
    assert _run(sim, pk, omit, lab_off_host=arr("lab_off", 2, int(pk.lab_off[1]) + (1 << 20)), nlabels=1 << 40) == 0
    pk = G.pack(sim, slots, 6)
    # a page without lines or without text is NOT refused by the host: the gate decides
    empty = G.pack(sim, [(pages[0], 0, None), (EMPTY_PAGE, 1, None), (pages[1], 0, None)], 6)
    assert _run(sim, empty, omit) == 0
    G.check(empty, [R.answer(*pages[0], omit), (G.SKIPPED, None, None), R.answer(*pages[1], omit)])
    # ... and such a page that the gate lets through is the device's to refuse
    empty = G.pack(sim, [(pages[0], 0, None), (EMPTY_PAGE, 0, None), (pages[1], 0, None)], 6)
    assert _run(sim, empty, omit) == 0
    G.check(empty, [R.answer(*pages[0], omit), (R.BOUNDS, None, None), R.answer(*pages[1], omit)])
    assert _run(sim, pk, omit) == 0
    G.check(pk, [R.answer(*pg, omit) for pg in pages])
