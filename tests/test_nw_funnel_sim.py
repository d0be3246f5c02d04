"""The funnel fill's data flow on the CPU (tests/native/sim_nw_funnel.cpp): phase 1 runs only the groups
funnel_groups() names inside a forced outer band, from the sentinel state, with the sentinel tails in a strip's rows,
and gathers the certificate's words in the kernel's order -- the exit word must EQUAL a scan of every cell of the region
for neighbours outside it, which proves the kernel's list of edge cells complete.  The unchanged phase 2 runs on top in
all three traceback flows and must never restart from or re-fill with anything phase 1 did not write (the replay fails
with a negative code if it does).  Where the certificate passes the alignment equals the oracle's and the oracle's
path lies inside the region; where the path leaves the region it must not pass."""
import ctypes

import numpy as np
import pytest

import simlib
from oracle import nw_oracle
from tools.synth import synth_pair_ids

DEFAULT = [8, -4, -7, -7, -3, 0]
FLOWS = [32, 1064, 2064]        # nw_trace2_kernel (32-lane window), nw_trace2w_kernel, nw_trace2h_kernel (half-strips)


def load_sim():
    lib = simlib.load("nw_funnel", [simlib.NAT + "sim_nw.cpp", simlib.CSRC + "nw_cell.h", simlib.CSRC + "nw_band.h"])
    lib.sim_nw2_funnel.restype = ctypes.c_int
    lib.sim_nw2_funnel.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                   ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                                   ctypes.c_void_p, ctypes.c_void_p]
    return lib


def replay(lib, t, o, params, w, flow):
    """dict of the replay's outcome: ok, v0, u, exit, count, scan, exit0, funnel, ranges, ops"""
    t = np.ascontiguousarray(t, dtype=np.int32)
    o = np.ascontiguousarray(o, dtype=np.int32)
    p = np.asarray(params, dtype=np.int32)
    ops = np.zeros(len(t) + len(o) + 1, dtype=np.uint8)
    ln = ctypes.c_int(0)
    info = np.zeros(8, dtype=np.int32)
    nstrips = (len(t) + 255) // 256
    ranges = np.zeros(2 * nstrips, dtype=np.int32)
    rc = lib.sim_nw2_funnel(t.ctypes.data, len(t), o.ctypes.data, len(o), p.ctypes.data, w, flow, ops.ctypes.data,
                            ctypes.byref(ln), info.ctypes.data, ranges.ctypes.data)
    assert rc == 0, (rc, len(t), len(o), w, flow)
    return {"ok": bool(info[0]), "v0": int(info[1]), "u": int(info[2]), "exit": int(info[3]), "count": int(info[4]),
            "scan": int(info[5]), "exit0": int(info[6]), "funnel": bool(info[7]),
            "ranges": ranges.reshape(nstrips, 2), "ops": ops[:ln.value]}


@pytest.fixture(scope="module")
def sim():
    return load_sim()


def _inside(ops, ranges, m):
    """does the alignment stay on cells of the region (or the boundary)?"""
    ngroups = (m + 63 + 3) // 4
    i = j = 0
    for op in ops.tolist():
        i += op != 2
        j += op != 1
        if i == 0 or j == 0:
            continue
        gl, gh = ranges[(i - 1) // 256]
        l = ((i - 1) % 256) // 4
        jlo = 1 if gl == 0 else 4 * gl - l + 3
        jhi = m if gh == ngroups else min(m, 4 * gh - l)
        if not jlo <= j <= jhi:
            return False
    return True


def _path_score(t, o, ops, s):
    sc, i, j, prev = 0, 0, 0, None
    for op in ops.tolist():
        if op == 0:
            sc += s[0] if t[i] == o[j] else s[1]; i += 1; j += 1
        elif op == 1:
            sc += s[4] + (s[2] if prev != 1 else 0); i += 1
        else:
            sc += s[5] + (s[3] if prev != 2 else 0); j += 1
        prev = op
    return sc


_ORACLE = {}


def _oracle(t, o, params):
    key = (np.asarray(t).tobytes(), np.asarray(o).tobytes(), tuple(params))
    if key not in _ORACLE:
        _ORACLE[key] = nw_oracle.align_ids(t, o, params)
    return _ORACLE[key]


def _check(lib, t, o, params, w, flow, must_certify=None):
    n, m = len(t), len(o)
    want = _oracle(t, o, params)
    r = replay(lib, t, o, params, w, flow)
    assert r["exit"] == r["scan"], (n, m, w, "the kernel's edge list against the scan of all cells", r["exit"], r["scan"])
    assert r["count"] == (n + 255) // 256 and r["exit"] >= r["exit0"]
    inside = _inside(want, r["ranges"], m)
    if r["ok"]:
        assert inside, (n, m, w, "certified although the oracle's path leaves the region")
        assert r["ops"].tolist() == want.tolist(), (n, m, w, flow)
    if not inside:
        assert not r["ok"]
    if must_certify is not None:
        assert r["ok"] == must_certify, (n, m, w, r)
    return r


@pytest.mark.parametrize("flow", FLOWS)
def test_funnel_replay_certified(sim, flow):
    for (n, m, seed), w in [((1100, 1100, 11), 600), ((1300, 900, 12), 600), ((900, 1300, 13), 600),
                            ((1025, 1040, 14), 500)]:
        t, o = synth_pair_ids(n, m, seed)
        r = _check(sim, t, o, DEFAULT, w, flow, must_certify=True)
        assert r["funnel"]
        # v0 is the smallest of the last cell's three values, all exact where certified: the oracle's path is worth
        # one of them, and they lie within a gap open + extend and a substitution of each other
        assert 0 <= _path_score(t, o, _oracle(t, o, DEFAULT), DEFAULT) - r["v0"] <= 40


@pytest.mark.parametrize("flow", FLOWS)
def test_funnel_replay_uncertified(sim, flow):
    rng = np.random.default_rng(5)
    # unrelated strings score low
    _check(sim, rng.integers(0, 27, 1100), rng.integers(0, 27, 1100), DEFAULT, 600, flow, must_certify=False)
    # a path that leaves the region: t = X k + C, o = C + Y k
    C = rng.integers(0, 20, 900)
    for k in (186, 326, 420):
        t = np.concatenate([np.full(k, 25), C]); o = np.concatenate([C, np.full(k, 26)])
        _check(sim, t, o, DEFAULT, 600, flow)


@pytest.mark.parametrize("flow", [2064])
def test_funnel_replay_other_systems_and_edges(sim, flow):
    """sizes around strip, half-strip and checkpoint-interval borders, other scoring systems with non-positive gap
    opens, outer widths that do and do not clip the funnel: the funnel's own ranges run in every one"""
    for n, m, seed in [(1025, 1030, 1), (1153, 1100, 2), (1281, 1281, 3), (1280, 1217, 5), (1101, 1024, 6)]:
        t, o = synth_pair_ids(n, m, seed)
        for params in (DEFAULT, [10, -5, -7, -7, -7, -7], [5, -10, -2, -7, 0, -5], [11, -4, -2, -2, 0, 0]):
            for w in (200, 700):
                assert _check(sim, t, o, params, w, flow)["funnel"]


# the funnel is declined -- a <= 0; gap steps so good that the left width's denominator a - 2 cvi - 2 chi is <= 0 -- and
# the outer band's ranges run under the exit certificate, from skewed step 4 gl + 2 of a strip that starts past group 0
DECLINED = [[-1, -4, -7, -7, -3, 0], [4, -4, 0, 0, 1, 1], [0, -8, -1, -1, -1, -1]]


@pytest.mark.parametrize("flow", FLOWS)
def test_funnel_replay_declined(sim, flow):
    """the band's own ranges under the funnel's certificate: the edge list still equals the scan of all cells, phase 2
    reads nothing phase 1 did not write, and what certifies is the oracle's.  Widths that cut the table on both sides
    (300), on neither side of the first strips (700), and shapes n != m both ways."""
    certified_cut = 0
    for n, m, seed in [(1100, 1100, 11), (1300, 900, 12), (900, 1300, 13), (1025, 1040, 14)]:
        t, o = synth_pair_ids(n, m, seed)
        for params in DECLINED:
            for w in (300, 700):
                r = _check(sim, t, o, params, w, flow)
                assert not r["funnel"]
                if w == 300:
                    assert r["ranges"][0][1] < (m + 63 + 3) // 4 and (m < n or r["ranges"][-1][0] > 0)
                certified_cut += r["ok"] and r["ranges"][-1][0] > 0
    assert certified_cut > 0                  # (phase 2 ran on a declined region that is cut on both sides, too)
