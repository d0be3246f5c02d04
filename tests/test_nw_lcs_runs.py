"""The run schedule of nw_lcs_suffix_kernel's right-edge stores (csrc/nw_band.h: lcs_next_run) on the CPU, through
tests/native/sim_nw_lcs_runs.cpp: expanded, the runs are the events of the schedule's definition (the next_event walker
of tests/native/sim_nw_funnel_lcs.cpp) in the same order with the same step, lane, bit, strip and l, and inside a run
the steps are exactly 4 apart.  The same source builds, with its own main, as the stand-alone program that runs under
-fsanitize=address,undefined."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import simlib

N_MAX = 1100


@pytest.fixture(scope="module")
def sim():
    lib = simlib.load("nw_lcs_runs", [simlib.CSRC + "nw_cell.h", simlib.CSRC + "nw_band.h"])
    lib.sim_lcs_runs_sweep.restype = ctypes.c_int
    lib.sim_lcs_runs_sweep.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p]
    lib.sim_lcs_runs_expand.restype = ctypes.c_int
    lib.sim_lcs_runs_expand.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    return lib


def _ms():
    """m at 64 k - 1, 64 k and 64 k + 1 up to N_MAX, a few small ones and the largest"""
    ms = [2, 3, 5, 31, N_MAX]
    for k in range(1, N_MAX // 64 + 1):
        ms += [64 * k - 1, 64 * k, 64 * k + 1]
    return np.array([m for m in ms if m <= N_MAX], dtype=np.int32)


@pytest.mark.parametrize("seed", [1, 2])
def test_runs_expand_to_the_definitions_events(sim, seed):
    """every n in 2 .. 1100 (all residues mod 4 and mod 256; n > m and m > n both occur) against every listed m, each
    under six kinds of non-decreasing gh per strip: all 0, all >= ngroups, random, a ramp, multiples of 16, around m / 4"""
    ms = _ms()
    fail = np.zeros(6, dtype=np.int32)
    rc = sim.sim_lcs_runs_sweep(2, N_MAX, ms.ctypes.data, len(ms), seed, fail.ctypes.data)
    assert rc == (N_MAX - 1) * len(ms) * 6, (rc, fail.tolist())


def _events(n, m, gh):
    """the definition once more, in Python: (step, lane, bit, strip, l) per store, strips from the last, lanes from 63"""
    ngroups = (m + 63 + 3) // 4
    out = []
    for s in range((n + 255) // 256 - 1, -1, -1):
        if gh[s] >= ngroups:
            continue
        for l in range(63, -1, -1):
            r, cnt = n - 256 * s - 4 * l, m - 4 * gh[s] + l
            if r >= 1 and cnt >= 0:
                out.append((r - 1 + cnt // 64, cnt // 64, cnt % 64, s, l))
    return out


@pytest.mark.parametrize("n,m,gh", [
    (1024, 1024, [48, 112, 176, 256]),          # every strip has an edge; word crossings inside strips
    (1027, 1087, [16, 16, 80, 160, 288]),       # a last strip of three rows: lanes 1 .. 63 have no row
    (1025, 1025, [64, 128, 192, 257, 257]),     # 4 gh > m: the low lanes have cnt < 0, and the last strip's one row no store
    (700, 1100, [0, 0, 0]),                     # gh = 0: cnt = m + l, the topmost words
    (1100, 300, [91, 91, 91, 91, 91]),          # no right edge anywhere
    (2, 2, [0]),
])
def test_against_the_definition_in_python(sim, n, m, gh):
    gh_a = np.array(gh, dtype=np.int32)
    assert len(gh) == (n + 255) // 256
    out = np.zeros(5 * 64 * len(gh), dtype=np.int32)
    cnt = sim.sim_lcs_runs_expand(n, m, gh_a.ctypes.data, out.ctypes.data, 64 * len(gh))
    want = _events(n, m, gh)
    assert cnt == len(want)
    assert [tuple(r) for r in out[:5 * cnt].reshape(cnt, 5).tolist()] == want
    steps = [e[0] for e in want]
    assert all(a < b for a, b in zip(steps, steps[1:]))


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the sweep with its own main, compiled with -fsanitize=address,undefined: no report, every case holds"""
    exe = str(tmp_path / "sim_nw_lcs_runs_asan")
    src = os.path.join(simlib.REPO, simlib.NAT, "sim_nw_lcs_runs.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DSIM_MAIN", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "BAD" not in out.stdout and out.stderr == "", (out.stdout, out.stderr)
