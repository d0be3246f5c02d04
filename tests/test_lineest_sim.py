"""The line normaliser's kernels without a GPU: tests/native/sim_lineest.cpp compiles csrc/ta_lineest.hip ITSELF for the
host (a workgroup = 256 lanes that meet at every barrier; tests/native/hipshim_wg) and the result must agree with the checker
oracle/lineest_ref.py as tests/test_lineest_gpu.py asks of the real kernels: per-column arg-max, centre line, band
half-height and output width exactly, the rows to 2e-6 -- on the strips of tests/lineest_cases.py, which pick the kernels'
branches.  This is what runs the four spelled-out tap loops, the row kernel's second tile and its LDS array filled to the
last element, and the dewarp's bounds; the same source as a program under AddressSanitizer + UBSan must end clean on all
of them."""
import os
import subprocess

import numpy as np
import pytest

import lineest_cases as C
import simlib
from conftest import REPO
from text_alignment_amd import _abi

_NAT = os.path.join(REPO, "tests", "native")
_SRC = os.path.join(_NAT, "sim_lineest.cpp")
_EXE = os.path.join(_NAT, "build", "sim_lineest_san")
_DEPS = [_SRC, os.path.join(_NAT, "hipshim_wg", "hip", "hip_runtime.h"),
         os.path.join(REPO, "text_alignment_amd", "csrc", "ta_lineest.hip"),
         os.path.join(REPO, "text_alignment_amd", "csrc", "corr1d.h"),
         os.path.join(REPO, "text_alignment_amd", "csrc", "ta_common.h"),
         os.path.join(REPO, "include", "text_alignment_amd.h")]
_CXX = ["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(_NAT, "hipshim_wg")]


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in _DEPS)


@pytest.fixture(scope="module")
def sim():
    lib = simlib.load("lineest", _DEPS[1:], flags=["-ffp-contract=off"], include=["hipshim_wg"])
    return _abi.bind(lib, ["ta_linenorm_measure", "ta_linenorm_resample"])


class Packed(object):
    pass


def pack(strips):
    """host arrays of one measuring call, laid out as lineest_gpu.measure_strips_begin lays them out on the device: the
    strips' pixels back to back, one set of the package's own gaussian weights per distinct height"""
    from text_alignment_amd import lineest_gpu
    pk = Packed()
    n = pk.n = len(strips)
    pk.hh = np.asarray([s.shape[0] for s in strips], np.int32)
    pk.ww = np.asarray([s.shape[1] for s in strips], np.int32)
    sizes = pk.hh.astype(np.int64) * pk.ww
    pk.pix_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    pk.col_off = np.concatenate([[0], np.cumsum(pk.ww)]).astype(np.int64)
    pk.pix = np.concatenate([np.ascontiguousarray(s).reshape(-1) for s in strips])
    parts, where, pos = [], {}, 0
    pk.gw_off, pk.gr = np.zeros((n, 3), np.int64), np.zeros((n, 3), np.int32)
    for k in range(n):
        h = int(pk.hh[k])
        if h not in where:
            where[h] = []
            for wts, rad in lineest_gpu._line_kernels(h):
                parts.append(np.ascontiguousarray(wts, dtype=np.float64))
                where[h].append((pos + rad, rad))
                pos += len(wts)
        for q, (o, rad) in enumerate(where[h]):
            pk.gw_off[k, q], pk.gr[k, q] = o, rad
    pk.gw = np.concatenate(parts)
    pk.ws_off = 3 * pk.pix_off
    return pk


def _p(a):
    return a.ctypes.data


def normalise(lib, strips, planes=None):
    """both passes on host arrays, every output poisoned first: [(arg, center, r, wout, rows)] per strip; planes: a list
    that takes every strip's (smoothed, box-filtered) planes as the measuring pass leaves them in its workspace"""
    pk = pack(strips)
    n, ncol = pk.n, int(pk.col_off[-1])
    ws = np.full(3 * pk.pix.size, np.nan)
    arg, center = np.full(ncol, -77, np.int32), np.full(ncol, -77, np.int32)
    minmax, r, wout = np.full(2 * n, -77, np.int32), np.full(n, -77, np.int32), np.full(n, -77, np.int32)
    assert lib.ta_linenorm_measure(_p(pk.pix), _p(pk.pix_off), _p(pk.hh), _p(pk.ww), n, _p(pk.gw), _p(pk.gw_off),
                                   _p(pk.gr), _p(ws), _p(pk.ws_off), _p(arg), _p(center), _p(pk.col_off), _p(minmax),
                                   _p(r), _p(wout), None) == 0
    if planes is not None:                                # plane 2: both gaussians; plane 1: both box filters of it
        for k, s in enumerate(strips):
            pl = ws[pk.ws_off[k]:pk.ws_off[k] + 3 * s.size].reshape((3,) + s.shape)
            planes.append((pl[2], pl[1]))
    if (wout < 1).any():                                  # (the package refuses such a batch: measure_strips_end)
        return [(arg[a:b], center[a:b], r[k], wout[k], None) for k, (a, b) in enumerate(zip(pk.col_off, pk.col_off[1:]))]
    T = wout.astype(np.int64) + 2 * C.PAD
    row_off = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    tmp_off = np.concatenate([[0], np.cumsum(wout.astype(np.int64) * C.TARGET_HEIGHT)]).astype(np.int64)
    tmp = np.full(int(tmp_off[-1]), np.nan, np.float32)
    omax = np.full(n, 0x7fc00000, np.uint32)
    x = np.full((int(row_off[-1]), C.TARGET_HEIGHT), np.nan, np.float32)
    assert lib.ta_linenorm_resample(_p(pk.pix), _p(pk.pix_off), _p(pk.hh), _p(pk.ww), n, _p(center), _p(pk.col_off),
                                    _p(minmax), _p(r), _p(wout), _p(tmp), _p(tmp_off), _p(omax), _p(x), _p(row_off),
                                    None) == 0
    return [(arg[pk.col_off[k]:pk.col_off[k + 1]], center[pk.col_off[k]:pk.col_off[k + 1]], r[k], wout[k],
             x[row_off[k]:row_off[k + 1]]) for k in range(n)]


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """The sanitized program, STARTED on every accepted strip: four runs side by side, the strips dealt out by the row
    gaussian's cost (under the sanitizers the lot takes 15 s on one core), going on while the library below does the
    same work; the last test of this file waits for them.  [(strips, their packing, output file, process)]"""
    if _stale(_EXE):
        os.makedirs(os.path.dirname(_EXE), exist_ok=True)
        # (the runtimes linked in: the program is then on its own whatever else the environment loads into a process)
        subprocess.check_call(_CXX + ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                      "-static-libasan", "-static-libubsan", "-DSIM_LINEEST_MAIN", "-o", _EXE, _SRC])
    tmp = tmp_path_factory.mktemp("sim_lineest")
    cases = sorted(C.accepted(), key=lambda c: -c[1].size * min(4 * c[1].shape[0], c[1].shape[1]))
    groups, load = [[] for _ in range(4)], [0] * 4
    for name, s in cases:
        g = load.index(min(load))
        groups[g].append((name, s))
        load[g] += s.size * min(4 * s.shape[0], s.shape[1])
    runs = []
    for g, group in enumerate(groups):
        pk = pack([s for _, s in group])
        fin, fout = str(tmp / ("in%d.bin" % g)), str(tmp / ("out%d.bin" % g))
        with open(fin, "wb") as f:
            for a in (np.asarray([pk.n, pk.pix.size, pk.gw.size], np.int64), pk.hh, pk.ww, pk.gw_off, pk.gr, pk.gw, pk.pix):
                f.write(np.ascontiguousarray(a).tobytes())
        runs.append((group, pk, fout, subprocess.Popen([_EXE, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                                       text=True)))
    yield runs
    for _, _, _, proc in runs:
        if proc.poll() is None:
            proc.kill()
            proc.communicate()


@pytest.fixture(scope="module")
def results(sim, sanitized):
    """all accepted strips in ONE call (mixed heights, repeated heights sharing their weights, odd pixel offsets)"""
    cases = C.accepted()
    planes = []
    out = dict(zip([name for name, _ in cases], normalise(sim, [s for _, s in cases], planes)))
    out["planes"] = dict(zip([name for name, _ in cases], planes))
    return out


@pytest.mark.parametrize("name", [name for name, _ in C.accepted()])
def test_host_build_of_the_kernels_equals_the_checker(results, name):
    C.check_strip(name, *results[name])


def test_smoothed_planes_equal_scipy_bit_for_bit(results):
    """The integers above move only when a sum crosses a threshold; a tap pair lost at the far end of a column changes
    rows 0 and h - 1 of the smoothed strip and, on these strips, no arg-max.  The claim the kernels make is stronger --
    scipy's float64 sums, operation by operation -- and here it is held to: both gaussians' result and the box filters'
    of it, every element, every strip."""
    for name, _ in C.accepted():
        want_g, want_u = C.want_planes(name)
        g, u = results["planes"][name]
        assert g.tobytes() == want_g.tobytes(), (name, "gaussians", float(np.abs(g - want_g).max()))
        assert u.tobytes() == want_u.tobytes(), (name, "box filters", float(np.abs(u - want_u).max()))


def test_zero_width_strips_measure_as_width_zero(sim):
    """what the package refuses in measure_strips_end, as the checker does, is exactly this: the measuring pass itself
    writes an output width of 0, between two good strips that keep their answers"""
    good = ["scatter 8x4", "scatter 17x63"]
    for name, s in C.refused():
        got = normalise(sim, [C.by_name(good[0]), s, C.by_name(good[1])])
        assert got[1][3] == 0, name
        for k, g in ((0, good[0]), (2, good[1])):
            wt = C.want(g)
            assert np.array_equal(got[k][0], wt.arg) and np.array_equal(got[k][1], wt.center)
            assert (got[k][2], got[k][3]) == (wt.r, wt.wout)


def test_sanitized_program_ends_clean_and_agrees(results, sanitized):
    """the same source with its own main, built with AddressSanitizer and UBSan, on every accepted strip: every buffer
    is a heap block of the exact size and the LDS arrays are guarded statics, so a halo index, an LDS index or a dewarp
    row out of bounds ends the program; its integers equal the library's, its rows too (both are built without
    contraction)"""
    said = [proc.communicate()[0] for _, _, _, proc in sanitized]
    for (group, pk, fout, proc), out in zip(sanitized, said):
        names = [name for name, _ in group]
        assert proc.returncode == 0, (names, out[-4000:])
        assert "Sanitizer" not in out and "runtime error" not in out, (names, out[-4000:])
        n, ncol = pk.n, int(pk.col_off[-1])
        with open(fout, "rb") as f:
            r, wout = np.frombuffer(f.read(4 * n), np.int32), np.frombuffer(f.read(4 * n), np.int32)
            arg, center = np.frombuffer(f.read(4 * ncol), np.int32), np.frombuffer(f.read(4 * ncol), np.int32)
            x = np.frombuffer(f.read(), np.float32)
        have = [results[name] for name in names]
        assert np.array_equal(r, [h[2] for h in have]) and np.array_equal(wout, [h[3] for h in have]), names
        assert np.array_equal(arg, np.concatenate([h[0] for h in have])), names
        assert np.array_equal(center, np.concatenate([h[1] for h in have])), names
        assert x.tobytes() == np.concatenate([h[4] for h in have]).tobytes(), names
