"""The LCS-bounded funnel on the CPU (tests/native/sim_nw_funnel_lcs.cpp): nw_lcs_suffix_kernel's data flow replayed
lane by lane -- every value it stores equals a plain dynamic-programming LCS table -- and phase 1 under the narrower
ranges with the three edge gatherings taking funnel_suf_lcs.  The exit word must EQUAL a scan of every cell of the region
and the boundary for neighbours outside it.  Where the certificate passes, the oracle's path lies inside the region; where
the path leaves the region it must not pass.  The same source builds, with its own main, as the stand-alone program
that runs under -fsanitize=address,undefined."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import simlib
from test_nw_funnel_sim import DEFAULT, _inside, _oracle
from tools.synth import synth_pair_ids

OTHER = [10, -5, -7, -7, -2, -2]


def load_sim():
    lib = simlib.load("nw_funnel_lcs", [simlib.NAT + "sim_nw.cpp", simlib.CSRC + "nw_cell.h", simlib.CSRC + "nw_band.h"])
    lib.sim_nw2_funnel_lcs.restype = ctypes.c_int
    lib.sim_nw2_funnel_lcs.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def lcs_words(n):
    nstrips = (n + 255) // 256
    return ((n + 1 + 63) & ~63) + 192 * nstrips


def replay(lib, t, o, params, w, alphabet=27):
    """dict of the replay's outcome: ok, v0, u, exit, count, scan, exit_lcs, flag, table_ok, static_scan, table, ranges"""
    t = np.ascontiguousarray(t, dtype=np.int32)
    o = np.ascontiguousarray(o, dtype=np.int32)
    p = np.asarray(params, dtype=np.int32)
    info = np.zeros(10, dtype=np.int32)
    nstrips = (len(t) + 255) // 256
    ranges = np.zeros(2 * nstrips, dtype=np.int32)
    table = np.zeros(lcs_words(len(t)), dtype=np.int32)
    rc = lib.sim_nw2_funnel_lcs(t.ctypes.data, len(t), o.ctypes.data, len(o), p.ctypes.data, w, alphabet,
                                info.ctypes.data, table.ctypes.data, ranges.ctypes.data)
    assert rc == 0, (rc, len(t), len(o), w)
    return {"ok": bool(info[0]), "v0": int(info[1]), "u": int(info[2]), "exit": int(info[3]), "count": int(info[4]),
            "scan": int(info[5]), "exit_lcs": int(info[6]), "flag": int(info[7]), "table_ok": bool(info[8]),
            "static_scan": int(info[9]), "table": table, "ranges": ranges.reshape(nstrips, 2)}


@pytest.fixture(scope="module")
def sim():
    return load_sim()


def _check(sim, t, o, params, w):
    n, m = len(t), len(o)
    r = replay(sim, t, o, params, w)
    assert r["flag"] == 2, (n, m, w)
    assert r["table_ok"], (n, m, "a stored count differs from the plain LCS table")
    assert r["exit"] == r["scan"], (n, m, w, "the kernels' edge list against the scan of all cells", r["exit"], r["scan"])
    assert r["scan"] <= r["static_scan"] and r["count"] == (n + 255) // 256
    inside = _inside(_oracle(t, o, params), r["ranges"], m)
    if r["ok"]:
        assert inside, (n, m, w, "certified although the oracle's path leaves the region")
    if not inside:
        assert not r["ok"]
    return r


@pytest.mark.parametrize("n,m,seed", [(1024, 1100, 41), (1280, 1024, 42), (1537, 2049, 43), (1100, 1100, 11), (2049, 1999, 44)])
@pytest.mark.parametrize("params", [DEFAULT, OTHER])
def test_exit_word_equals_the_scan_and_the_table_the_plain_lcs(sim, n, m, seed, params):
    t, o = synth_pair_ids(n, m, seed)
    r = _check(sim, t, o, params, 600)
    # related pairs certify under the narrower ranges (2049 rows: the OUTER band of 600 is too narrow for its bound U)
    assert r["ok"] == (r["v0"] > r["u"]) and (r["ok"] or n > 2000), r
    assert any(gh < r["ranges"][-1][1] for gl, gh in r["ranges"])


def test_unrelated_pair_does_not_certify(sim):
    rng = np.random.default_rng(5)
    t, o = rng.integers(0, 27, size=1100).astype(np.int32), rng.integers(0, 27, size=1100).astype(np.int32)
    r = _check(sim, t, o, DEFAULT, 600)
    assert not r["ok"]


def test_ids_outside_the_alphabet_never_match(sim):
    """an id the hint does not cover matches nothing in the kernel's profile; the table must not count it either"""
    t, o = synth_pair_ids(1100, 1100, 11)
    t, o = t.copy(), o.copy()
    t[::7] = 40
    o[::5] = 40
    r = replay(sim, t, o, DEFAULT, 600, alphabet=27)
    assert r["flag"] == 2 and r["table_ok"] and r["exit"] == r["scan"]


def test_declined_shapes(sim):
    """more columns than the kernel keeps words for, mismatch >= match, too large an alphabet: the static funnel's"""
    t, o = synth_pair_ids(1100, 1100, 11)
    assert replay(sim, t, o, [4, 4, -7, -7, -3, 0], 600)["flag"] != 2
    assert replay(sim, t, o, DEFAULT, 600, alphabet=65)["flag"] != 2
    t, o = synth_pair_ids(1100, 4100, 12)
    assert replay(sim, t, o, DEFAULT, 600)["flag"] != 2


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the replay with its own main, compiled with -fsanitize=address,undefined: no report, every check holds"""
    exe = str(tmp_path / "sim_nw_funnel_lcs_asan")
    src = os.path.join(simlib.REPO, simlib.NAT, "sim_nw_funnel_lcs.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DSIM_MAIN", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "BAD" not in out.stdout and out.stderr == "", (out.stdout, out.stderr)
