"""The held-out scoring kernel without a GPU: tests/native/sim_errs.cpp compiles csrc/ta_errs.hip ITSELF for the host
(a wave = 64 coroutines that meet at every ballot / DPP move / barrier; tests/native/hipshim) and the result must equal
the plain-Python checker tests/errs_ref.py in every six-tuple and every cell of conf -- the same batch, kinds and
refusals as tests/test_errs_gpu.py drives through the real kernel."""
import numpy as np
import pytest

import errs_ref as R
import simlib
from text_alignment_amd import _abi

NO = 12


@pytest.fixture(scope="module")
def sim():
    deps = [simlib.HIPSHIM, simlib.CSRC + "ta_errs.hip", simlib.HEADER]
    return _abi.bind(simlib.load("errs", deps, include=["hipshim"]), ["ta_errs_workspace_bytes", "ta_edit_distance"])


def _score(lib, lines, kind, T=None, conf=None, dec_off_shift=None):
    """the host twin of errs.score_decoded: dec_c with gaps (filled with a code no line may read), a status word
    behind dec_n, the workspace sized from the bound (T + 1) // 2 and poisoned"""
    codes, targets = [a for a, _ in lines], [g for _, g in lines]
    n = len(lines)
    off, flat = [], []
    for k, a in enumerate(codes):
        flat.extend([99] * (3 + k % 5))
        off.append(len(flat))
        flat.extend(a)
    flat.extend([99] * 4)
    T = [max(2 * len(a) - 1, 0) for a in codes] if T is None else T
    dec_c = np.asarray(flat, dtype=np.int32)
    dec_off = np.asarray(off, dtype=np.int64)
    if dec_off_shift:
        for k, d in dec_off_shift.items():
            dec_off[k] += d
    dec_n = np.asarray([len(a) for a in codes] + [0x5a5a], dtype=np.int32)
    nb = np.asarray([(t + 1) // 2 for t in T], dtype=np.int32)
    m = np.asarray([len(g) for g in targets], dtype=np.int32)
    ws = np.asarray([lib.ta_errs_workspace_bytes(int(a), int(b)) for a, b in zip(nb, m)], dtype=np.int64)
    assert (ws >= 0).all()
    ws_off = np.zeros(n, dtype=np.int64)
    ws_off[1:] = np.cumsum(ws)[:-1]
    tgt_off = np.zeros(n, dtype=np.int64)
    tgt_off[1:] = np.cumsum(m.astype(np.int64))[:-1]
    tgt = np.asarray([c for g in targets for c in g] or [1], dtype=np.int32)
    work = np.full(max(int(ws.sum()), 16), 0xEE, dtype=np.uint8)
    per = np.full((n, 6), -7, dtype=np.int32)
    conf = np.zeros((NO + 1, NO + 1), dtype=np.int64) if conf is None else conf
    rc = lib.ta_edit_distance(dec_c.ctypes.data, dec_off.ctypes.data, dec_n.ctypes.data, dec_c.size, tgt.ctypes.data,
                              tgt_off.ctypes.data, m.ctypes.data, int(m.sum()), nb.ctypes.data, ws_off.ctypes.data, n,
                              NO + 1, R.KINDS.index(kind), nb.ctypes.data, m.ctypes.data, work.ctypes.data, work.size,
                              per.ctypes.data, conf.ctypes.data, None)
    assert rc == 0
    return per, conf


@pytest.fixture(scope="module")
def lines():
    from test_errs_gpu import _lines
    return _lines()


def test_host_build_of_the_kernel_equals_the_checker(sim, lines):
    from test_errs_gpu import SHAPES
    for kind in R.KINDS:
        per, conf = _score(sim, lines, kind)
        want_per, want_conf = R.score([a for a, _ in lines], [g for _, g in lines], NO + 1, kind)
        assert np.array_equal(per, want_per), kind
        assert np.array_equal(conf, want_conf), kind
        if kind == "exact":
            assert [tuple(r) for r in per[:, 1:3].tolist()] == SHAPES
    # two calls into one matrix
    conf = np.zeros((NO + 1, NO + 1), dtype=np.int64)
    p1, _ = _score(sim, lines[:6], "nospace", conf=conf)
    p2, _ = _score(sim, lines[6:], "nospace", conf=conf)
    assert np.array_equal(np.concatenate([p1, p2]), want_per) and np.array_equal(conf, want_conf)


def test_host_build_on_random_small_pairs(sim):
    """many short pairs over a three-letter alphabet (ties everywhere) with spaces and class 0 mixed in"""
    rng = np.random.default_rng(31)
    lines = []
    for _ in range(60):
        n, m = int(rng.integers(0, 140)), int(rng.integers(0, 140))
        a = rng.choice([0, 1, 2, 3, 4], p=[0.1, 0.15, 0.25, 0.25, 0.25], size=n).tolist()
        g = rng.choice([1, 2, 3, 4, NO], p=[0.15, 0.27, 0.27, 0.27, 0.04], size=m).tolist()
        lines.append((a, g))
    for kind in R.KINDS:
        per, conf = _score(sim, lines, kind)
        want_per, want_conf = R.score([a for a, _ in lines], [g for _, g in lines], NO + 1, kind)
        assert np.array_equal(per, want_per) and np.array_equal(conf, want_conf)


def test_host_build_refuses_what_the_kernel_must_refuse(sim, lines):
    pick = [lines[7], lines[6], lines[3]]
    T = [max(2 * len(a) - 1, 0) for a, _ in pick]
    T[1] -= 2                                            # the bound is now 64, the line decoded 65
    per, conf = _score(sim, pick, "exact", T=T)
    assert per[1].tolist() == [-1, 0, 0, 0, 0, 0]
    assert per[0].tolist() == list(R.score_line(*pick[0], NO + 1)[0]) and per[2].tolist() == [0, 1, 1, 0, 0, 0]
    assert np.array_equal(conf, R.score_line(*pick[0], NO + 1)[1] + R.score_line(*pick[2], NO + 1)[1])
    per, _ = _score(sim, pick, "exact", dec_off_shift={2: -1})          # reads the gap's code 99: no class
    assert per[2].tolist() == [-1, 0, 0, 0, 0, 0] and per[1, 0] == 65
    per, _ = _score(sim, pick, "exact", dec_off_shift={0: -(10 ** 6)})  # an offset before the array: nothing is read
    assert per[0].tolist() == [-1, 0, 0, 0, 0, 0] and per[1, 0] == 65
    per, _ = _score(sim, pick, "exact", dec_off_shift={1: 10 ** 6})     # ... and one behind it
    assert per[1].tolist() == [-1, 0, 0, 0, 0, 0] and per[2].tolist() == [0, 1, 1, 0, 0, 0]
    bad_target = [(lines[3][0], [0]), (lines[3][0], [NO + 1]), lines[3]]
    per, conf = _score(sim, bad_target, "exact")
    assert per[:, 0].tolist() == [-1, -1, 0] and conf.sum() == 1
