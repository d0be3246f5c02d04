"""The two-level match masks of nw_lcs_suffix_kernel (csrc/nw_band.h: lcs_mask_rows, lcs_mask_offsets) on the CPU,
through tests/native/sim_nw_lcs_masks.cpp: built as the kernel builds them, A[c >> 3] & B[c & 7] is the directly built
mask of every code of the alphabet and 0 for the pad and for codes outside it, on either string; the rows and the strips'
ranges stay within the 10 240 B at which LDS allows 16 one-wave workgroups per CU; and the bit-parallel recurrence on these
masks gives the plain LCS table.  The same source builds, with its own main, as the stand-alone program that runs under
-fsanitize=address,undefined."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import simlib

ALPHABETS = [1, 7, 8, 9, 16, 17, 27, 63, 64]
MS = [1, 63, 64, 65, 4095, 4096]
NS = [2, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def sim():
    lib = simlib.load("nw_lcs_masks", [simlib.CSRC + "nw_cell.h", simlib.CSRC + "nw_band.h"])
    lib.sim_lcs_masks_case.restype = ctypes.c_int
    lib.sim_lcs_masks_case.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p]
    lib.sim_lcs_mask_build.restype = ctypes.c_int
    lib.sim_lcs_mask_build.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.sim_lcs_mask_offsets.restype = ctypes.c_uint
    lib.sim_lcs_mask_pad.restype = ctypes.c_uint
    lib.sim_lcs_mask_lds_bytes.restype = ctypes.c_longlong
    return lib


@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_masks_and_recurrence(sim, alphabet):
    """per m: M of every code against the direct mask, 0 for the pad and for -1, alphabet, alphabet + 1, 255 (the strings
    carry those codes too); then the recurrence against the plain LCS table, every cell, at each n"""
    ns = np.array(NS, dtype=np.int32)
    for m in MS:
        fail = np.zeros(3, dtype=np.int32)
        rc = sim.sim_lcs_masks_case(alphabet, m, ns.ctypes.data, len(ns), 3, fail.ctypes.data)
        assert rc == 1 + len(NS), (rc, alphabet, m, fail.tolist())


def test_layout_in_python(sim):
    """the header's layout restated: A's rows, the pad row, B's eight; a code's offsets in the two halves of a word; the
    rows as numpy builds them from a string that also carries codes outside the alphabet"""
    rng = np.random.default_rng(17)
    for alphabet in ALPHABETS:
        nhi = (alphabet + 7) // 8
        assert sim.sim_lcs_mask_rows(alphabet) == nhi + 1 + 8
        pad = sim.sim_lcs_mask_pad(alphabet)
        assert pad == ((nhi * 512) << 16) | ((nhi + 1) * 512)
        for c in range(alphabet):
            assert sim.sim_lcs_mask_offsets(c, alphabet) == (((c >> 3) * 512) << 16) | ((nhi + 1 + (c & 7)) * 512)
        for c in (-1, alphabet, alphabet + 1, 255):
            assert sim.sim_lcs_mask_offsets(c, alphabet) == pad
        m = 1000
        o = rng.integers(0, alphabet, size=m).astype(np.int32)
        o[3::13] = np.resize([-1, alphabet, alphabet + 1, 255], len(o[3::13]))
        o[7] = alphabet - 1
        rows = np.zeros((nhi + 9) * 64, dtype=np.uint64)
        assert sim.sim_lcs_mask_build(o.ctypes.data, m, alphabet, rows.ctypes.data) == rows.size
        rows = rows.reshape(nhi + 9, 64)
        orev = np.full(4096, -1, dtype=np.int64)
        orev[:m] = o[::-1]
        inside = (orev >= 0) & (orev < alphabet)

        def words(sel):
            return np.packbits(sel.reshape(64, 64), axis=1, bitorder="little").view(np.uint64).reshape(64)

        for h in range(nhi):
            assert (rows[h] == words(inside & (orev >> 3 == h))).all(), (alphabet, h)
        assert not rows[nhi].any()
        for lo in range(8):
            assert (rows[nhi + 1 + lo] == words(inside & (orev & 7 == lo))).all(), (alphabet, lo)
        for c in range(alphabet):
            assert ((rows[c >> 3] & rows[nhi + 1 + (c & 7)]) == words(orev == c)).all(), (alphabet, c)


def test_sixteen_workgroups_per_cu_at_every_alphabet(sim):
    """rows x 512 B and 8 B per strip of the tallest problem the band takes: at most 160 KiB / 16"""
    max_a, max_n = sim.sim_lcs_max_alphabet(), sim.sim_lcs_max_n()
    assert max_a == 64
    for alphabet in range(1, max_a + 1):
        got = sim.sim_lcs_mask_lds_bytes(alphabet, max_n)
        assert got == 512 * sim.sim_lcs_mask_rows(alphabet) + 8 * ((max_n + 255) // 256)
        assert got <= 10240, (alphabet, got)
    assert sim.sim_lcs_mask_lds_bytes(27, 4096) == 13 * 512 + 128


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the sweep with its own main, compiled with -fsanitize=address,undefined: no report, every case holds"""
    exe = str(tmp_path / "sim_nw_lcs_masks_asan")
    src = os.path.join(simlib.REPO, simlib.NAT, "sim_nw_lcs_masks.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DSIM_MAIN", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "BAD" not in out.stdout and out.stderr == "", (out.stdout, out.stderr)
