"""The line distortion's kernels without a GPU: tests/native/sim_distort.cpp compiles csrc/ta_distort.hip ITSELF for the
host (a workgroup = 256 lanes that meet at every barrier, a grid in x, y and z; tests/native/hipshim_wg) and the result
must agree with the checker tests/distort_ref.py as tests/test_distort_edges_gpu.py asks of the real kernels
(distort_cases.check_case: fields to 1e-9 x distort, their peak, every pixel outside the excluded set) -- on the cases of
tests/distort_cases.py, which pick the kernels' branches: every column tile from 64 columns down to one, the LDS arrays
filled to their last element, the row pass's second and third tile, the column kernel's second sweep, radius 0 and 2048,
a seed and counters with high words, strips whose maximum is not 255.  That each case sits on the branch it names is
checked here against the source's own constants.  The same source as a program under AddressSanitizer + UBSan must end
clean on all of them and give the library's bytes."""
import concurrent.futures
import ctypes
import os
import subprocess

import numpy as np
import pytest

import distort_cases as C
import distort_ref as R
import simlib
from conftest import REPO
from text_alignment_amd import _abi

_NAT = os.path.join(REPO, "tests", "native")
_SRC = os.path.join(_NAT, "sim_distort.cpp")
_EXE = os.path.join(_NAT, "build", "sim_distort_san")
_DEPS = [_SRC, os.path.join(_NAT, "hipshim_wg", "hip", "hip_runtime.h"),
         os.path.join(REPO, "text_alignment_amd", "csrc", "ta_distort.hip"),
         os.path.join(REPO, "text_alignment_amd", "csrc", "corr1d.h"),
         os.path.join(REPO, "text_alignment_amd", "csrc", "ta_common.h"),
         os.path.join(REPO, "include", "text_alignment_amd.h")]
_CXX = ["g++", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(_NAT, "hipshim_wg")]

# On the host an idle workgroup is not free: the row grid is max_h workgroups per line and field, and each of them takes
# its 256 lanes through the nine barriers of the reduction.  So within a (sigma, distort) group the tall strips travel
# apart from the short ones.  MIXED is the batch in which one line sets the grid's row count (305 rows; the other line's
# workgroups idle beyond row 2) and the other its tile count (2305 columns: 37 column tiles, two row tiles; the tall
# line has one of each).
MIXED = ("305x20 ", "2x2305 ")
TOGETHER = [MIXED, ("112x40 ", "113x40 ", "304x20 ")]
TALL = 64                       # rows: a taller strip not named above travels alone
ALONE = ("2x4100 ",)            # 8200 busy workgroups of the column kernel: the longest call by itself


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in _DEPS)


def batches():
    """[[name]]: the calls this file makes, each of one (sigma, distort)"""
    out = []
    for _, names in C.groups():
        left = list(names)
        for prefixes in TOGETHER:
            picked = [n for n in left if n.startswith(prefixes)]
            if len(picked) == len(prefixes):
                out.append(picked)
                left = [n for n in left if n not in picked]
        alone = [n for n in left if C.case(n).strip.shape[0] > TALL or n.startswith(ALONE)]
        out += [[n] for n in alone]
        short = [n for n in left if n not in alone]
        if short:
            out.append(short)
    return out


class Packed(object):
    pass


def pack(names):
    """host arrays of one call, laid out as augment.distort_strips lays them out on the device"""
    from text_alignment_amd import lineest_gpu
    cs = [C.case(n) for n in names]
    assert len({(c.sigma, c.distort) for c in cs}) == 1
    pk = Packed()
    pk.n, pk.sigma, pk.distort = len(cs), cs[0].sigma, cs[0].distort
    pk.hh = np.asarray([c.strip.shape[0] for c in cs], np.int32)
    pk.ww = np.asarray([c.strip.shape[1] for c in cs], np.int32)
    sizes = pk.hh.astype(np.int64) * pk.ww
    pk.pix_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pk.pix = np.concatenate([c.strip.reshape(-1) for c in cs])
    pk.counters = np.asarray([c.counter for c in cs], np.uint64)
    pk.gw, pk.rad = lineest_gpu._gauss_weights(pk.sigma)
    pk.gw = np.ascontiguousarray(pk.gw, dtype=np.float64)
    assert pk.gw.size == 2 * pk.rad + 1 and pk.rad == C.radius(pk.sigma)
    return pk


def _p(a):
    return a.ctypes.data


def distort(lib, names):
    """one call on host arrays, every output and the workspace poisoned first: {name: (out, fields)}"""
    pk = pack(names)
    total = int(pk.pix_off[-1])
    ws_bytes = lib.ta_line_distort_workspace_bytes(pk.n, total)
    assert ws_bytes == 24 * pk.n + 32 * total
    ws = np.full(ws_bytes, 0xFF, np.uint8)                  # doubles of it are NaNs, max |F| bits above every double
    out = np.full(total, 0xA5, np.uint8)
    fields = np.full(2 * total, np.nan)
    rc = lib.ta_line_distort(_p(pk.pix), _p(pk.pix_off), _p(pk.hh), _p(pk.ww), _p(pk.counters), pk.n, _p(pk.hh), _p(pk.ww),
                             pk.distort, pk.sigma, C.SEED, _p(pk.gw), _p(ws), ws_bytes, _p(out), _p(fields), None)
    assert rc == 0, (names, lib.sim_distort_last_error())
    res = {}
    for k, name in enumerate(names):
        a, b, shape = int(pk.pix_off[k]), int(pk.pix_off[k + 1]), C.case(name).strip.shape
        res[name] = (out[a:b].reshape(shape), fields[2 * a:2 * b].reshape((2,) + shape))
    return res


@pytest.fixture(scope="module")
def sim():
    lib = simlib.load("distort", _DEPS[1:], flags=["-ffp-contract=off"], include=["hipshim_wg"])
    lib.sim_distort_constants.restype, lib.sim_distort_constants.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]
    lib.sim_distort_col_tile.restype, lib.sim_distort_col_tile.argtypes = ctypes.c_int, [ctypes.c_int32, ctypes.c_int32]
    lib.sim_distort_last_error.restype = ctypes.c_char_p
    return _abi.bind(lib, ["ta_line_distort", "ta_line_distort_workspace_bytes"])


@pytest.fixture(scope="module")
def constants(sim):
    buf = np.zeros(len(C.Constants._fields) - 1, np.int32)
    assert sim.sim_distort_constants(_p(buf), buf.size) == buf.size
    return C.Constants(*([int(v) for v in buf] + [sim.sim_distort_col_tile]))


def _cost(K, names):
    """of a batch on the host, roughly, in lane switches: the row grid's workgroups (idle ones too) through their
    barriers, the busy column tiles through theirs, and the taps at a few hundred to the switch"""
    cs = [C.case(n) for n in names]
    rad = C.radius(cs[0].sigma)
    rows = max(c.strip.shape[0] for c in cs) * len(cs) * 2 * K.threads * 11
    cols = sum(C.col_tiles(K, c.strip.shape[0], c.strip.shape[1], rad) for c in cs) * 2 * K.threads * 4
    return rows + cols + sum(c.strip.size for c in cs) * 4 * (2 * rad + 1) // 300


@pytest.fixture(scope="module")
def sanitized(constants, tmp_path_factory):
    """The sanitized program, STARTED on every batch: four at a time, the costly ones first (the column kernel's sweep
    is 8200 workgroups of 256 contexts and takes 10 s under the sanitizers, as long as three of the others), going on
    while the library below does the same work; the last test of this file waits for them.
    [(names, packing, output file, future of (exit code, what it printed))]"""
    if _stale(_EXE):
        os.makedirs(os.path.dirname(_EXE), exist_ok=True)
        # (the runtimes linked in: the program is then on its own whatever else the environment loads into a process)
        subprocess.check_call(_CXX + ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                      "-static-libasan", "-static-libubsan", "-DSIM_DISTORT_MAIN", "-o", _EXE, _SRC])
    tmp = tmp_path_factory.mktemp("sim_distort")
    live, stop = [], []

    def run(fin, fout):
        if stop:
            return None, ""
        proc = subprocess.Popen([_EXE, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        live.append(proc)
        said = proc.communicate()[0]
        return proc.returncode, said
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=4)
    runs = []
    for g, names in enumerate(sorted(batches(), key=lambda b: -_cost(constants, b))):
        pk = pack(names)
        fin, fout = str(tmp / ("in%d.bin" % g)), str(tmp / ("out%d.bin" % g))
        with open(fin, "wb") as f:
            for a in (np.asarray([pk.n, pk.pix.size, pk.rad], np.int64), np.asarray([pk.distort, pk.sigma], np.float64),
                      np.asarray([C.SEED], np.uint64), pk.hh, pk.ww, pk.counters, pk.gw, pk.pix):
                f.write(np.ascontiguousarray(a).tobytes())
        runs.append((names, pk, fout, pool.submit(run, fin, fout)))
    yield runs
    stop.append(True)
    for proc in live:
        if proc.poll() is None:
            proc.kill()
    pool.shutdown(wait=True)


@pytest.fixture(scope="module")
def results(sim, sanitized):
    """every case through the host library, in the calls of batches()"""
    out = {}
    for names in batches():
        out.update(distort(sim, names))
    return out


def test_every_case_sits_on_the_branch_it_names(constants):
    """the sentences of distort_cases as predicates over the SOURCE's constants and its choice of the column tile: a
    changed tile size, fit test, threshold or LDS size fails here instead of silently moving a case off its edge"""
    K = constants
    assert K.max_h + 2 * K.max_radius <= K.col_cells and K.threads * K.row_max_no + 2 * K.max_radius <= K.row_cells
    said = C.claims(K)
    assert len(said) >= 24
    for name, why, holds in said:
        assert holds, (name, why, K)
    # between them: every column tile there is, every count of outputs per lane, one to three row tiles
    have = {C.col_tile(K, c.strip.shape[0], C.radius(c.sigma)) for c in map(C.case, [n for n, _, _, _ in C.cases()])}
    tile, want = K.col_tile, set()
    while tile >= 1:
        want.add(tile)
        tile >>= 1
    assert have == want
    widths = [s.shape[1] for _, s, _, _ in C.cases()]
    assert {C.row_no(K, w) for w in widths} == {5, 7, K.row_max_no} and {C.row_tiles(K, w) for w in widths} >= {1, 2, 3}


def test_batches_hold_every_case_once_and_the_mixed_one():
    flat = [n for b in batches() for n in b]
    assert sorted(flat) == sorted(n for n, _, _, _ in C.cases())
    mixed = [b for b in batches() if len(b) == 2 and all(n.startswith(MIXED) for n in b)]
    assert len(mixed) == 1
    (h0, w0), (h1, w1) = (C.case(n).strip.shape for n in mixed[0])
    assert (h0, w0, h1, w1) == (305, 20, 2, 2305)           # one line's rows and the other's tiles make the grids


def test_seed_and_counters_have_high_words():
    assert C.SEED >> 32 and C.FIRST >> 32 and C.SEED & 0xFFFFFFFF and C.FIRST & 0xFFFFFFFF
    # and the checker reads them: another high word is another field
    a = R.noise(2, 3, C.SEED, C.FIRST)
    assert np.abs(a - R.noise(2, 3, C.SEED & 0xFFFFFFFF, C.FIRST)).max() > 0.1
    assert np.abs(a - R.noise(2, 3, C.SEED, C.FIRST & 0xFFFFFFFF)).max() > 0.1


def test_excluded_pixels_are_few():
    """the pixels no comparison rests on -- the checker's v within 1e-6 of a half-integer, its sample within 1e-6 of the
    rectangle's border -- are at most 0.1 % of all cases' pixels: a condition on the case set, from the checker alone"""
    excluded, total = C.excluded_share()
    print("excluded: %d of %d pixels" % (excluded, total))
    assert total > 100000 and excluded <= C.EXCLUDED_SHARE * total
    # cval is seen: strips whose maximum is not 255 have pixels that sample outside, and not all of them are excluded
    for name, s, _, _ in C.cases():
        if s.max() != 255 and s.min() != s.max():
            wt = C.want(name)
            assert int(((wt.out == s.max()) & ~wt.excluded).sum()) > 0, name


def test_the_field_bound_sees_a_lost_tap_pair():
    """on the checker alone: at every sigma of the list with a radius >= 1, a gaussian that loses its outermost tap pair
    -- along either axis -- moves some field value of some case by more than 100 x the bound check_case holds the
    kernels to, so the bound cannot hide the error it is there to catch"""
    by_sigma = {}
    for name, s, sigma, _ in C.cases():
        if C.radius(sigma) >= 1:
            by_sigma.setdefault(sigma, []).append((s.size, name))
    assert len(by_sigma) >= 7
    for sigma, members in sorted(by_sigma.items()):
        for axis in (0, 1):
            names = [n for _, n in sorted(members) if C.case(n).strip.shape[axis] > 1][:3]      # the smallest will do
            effect = max(C.lost_tap_effect(n, axis) for n in names)
            print("sigma %g, axis %d: a lost tap pair moves D by %.3g x distort" % (sigma, axis, effect))
            assert effect > 100 * C.FIELD_BOUND, (sigma, axis, effect)


@pytest.mark.parametrize("name", [name for name, _, _, _ in C.cases()])
def test_host_build_of_the_kernels_equals_the_checker(results, name):
    C.check_case(name, *results[name])


def test_largest_field_error_of_the_host_build(results):
    worst = max(float(np.abs(results[n][1] - C.want(n).d).max()) / d for n, _, _, d in C.cases())
    print("host build: max |D - D_ref| over all cases = %.3g x distort" % worst)
    assert worst <= C.FIELD_BOUND


def test_a_line_alone_equals_its_batch(sim, results):
    """with its own counter, either line of the mixed batch and a line of the short sigma-10 batch give the bytes they
    gave among their neighbours (tests/test_distort_edges_gpu.py asks it of every case)"""
    for prefix in ("305x20 grey, sigma 10, distort 3", "2x2305 grey, sigma 10, distort 3", "16x70 grey, sigma 10, distort 3"):
        name, = [n for n, _, _, _ in C.cases() if n.startswith(prefix)]
        out, fields = distort(sim, [name])[name]
        assert out.tobytes() == results[name][0].tobytes() and fields.tobytes() == results[name][1].tobytes(), name


def test_sanitized_program_ends_clean_and_agrees(results, sanitized):
    """the same source with its own main, built with AddressSanitizer and UBSan, on every batch: every buffer is a heap
    block of the exact size -- the weights 2 radius + 1 doubles, the workspace what ta_line_distort_workspace_bytes says
    -- and the LDS arrays are guarded statics, so a halo index, an LDS index or a sample out of bounds ends the program;
    its pixels and fields are the library's bytes (both are built without contraction)"""
    for names, pk, fout, future in sanitized:
        code, said = future.result()
        assert code == 0, (names, said[-4000:])
        assert "Sanitizer" not in said and "runtime error" not in said, (names, said[-4000:])
        # (all it may say is ASan's standing remark about programs that switch contexts)
        assert [ln for ln in said.splitlines() if ln and "makecontext/swapcontext" not in ln] == [], (names, said[-4000:])
        with open(fout, "rb") as f:
            out = np.frombuffer(f.read(pk.pix.size), np.uint8)
            fields = np.frombuffer(f.read(), np.float64)
        assert fields.size == 2 * pk.pix.size, names
        assert out.tobytes() == np.concatenate([results[n][0].reshape(-1) for n in names]).tobytes(), names
        assert fields.tobytes() == np.concatenate([results[n][1].reshape(-1) for n in names]).tobytes(), names
