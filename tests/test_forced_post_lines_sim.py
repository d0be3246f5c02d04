"""ta_forced_posterior_lines without a GPU: the host build of csrc/ta_forced_post.hip
(tests/native/sim_forced_post_lines.cpp, -ffp-contract=off as the library's build) run through the entry whose line list
lies "on the device" -- the lines of tests/forced_conf_cases.py in the layout of tests/forced_post_lines_cases.py -- and
every word held against tests/forced_post_ref.py at the aligner's own peaks BIT FOR BIT (the float64 outputs through
their int64 view)."""
import numpy as np
import pytest

import forced_cases as C0
import forced_conf_cases as CC
import forced_post_lines_cases as C
import forced_post_ref as R
import forced_ref as R0
import simlib
from text_alignment_amd import _abi


@pytest.fixture(scope="module")
def sim():
    deps = [simlib.NAT + "sim_forced_conf_shim.h", simlib.CSRC + "ta_forced_post.hip"] + C0.SIM_DEPS
    return C.bind(simlib.load("forced_post_lines", deps, flags=["-ffp-contract=off"], include=["hipshim"]))


def _run(lib, pk, **over):
    return C.call(lib, pk, lambda name: getattr(pk, name).ctypes.data, **over)


def _got(pk):
    return lambda name: getattr(pk, name)


@pytest.mark.parametrize("case", CC.cases(), ids=lambda c: c[0])
def test_the_indexed_entry_equals_the_checker_at_the_aligners_peaks(sim, case):
    """acc_line a permutation with holes, caps equal to and above L, slots behind count whose arrays are poison; every K
    at both edges, T = S, L = 1 and T = 3, the backward fill's chunk lengths -- the cases' own names say which"""
    name, no, lines = case
    pk = C.pack(sim, lines, no, frames=C0.want(name, lines)[0], seed=len(name))
    assert _run(sim, pk) == 0
    C.check_case(pk, name, lines, _got(pk))


def test_the_cases_hold_what_the_kernel_can_get_wrong():
    lines = [ln for _, _, ls in CC.cases() for ln in ls]
    TL = {(len(P), len(cs)) for P, cs in lines}
    for K, lmax, lnext in C0.EDGES:                      # every K at both edges, at T = S
        assert {(2 * L + 1, L) for L in (lmax, lnext) if L is not None} <= TL
    assert (3, 1) in TL and {7, 8, 9, 15, 16, 17, 23, 24} <= {T for T, _ in TL}
    assert {1, 63, 64, 127, 128, 255, 256, 511, 512, 1023} <= {L for T, L in TL if T == 2 * L + 1}


def _three(rng):
    return [(C0.probs(rng, 30, 6), C0.text(rng, 7, 6)), (C0.probs(rng, 21, 6), C0.text(rng, 5, 6)),
            (C0.probs(rng, 140, 6), C0.text(rng, 66, 6))]


def test_a_slot_the_aligner_refused_is_skipped_and_one_refused_here_leaves_its_neighbours_alone(sim):
    rng = np.random.default_rng(21)
    lines = _three(rng)
    frames = R0.align_batch(lines)[0]
    wanted = C.answer(lines, frames)

    def check(pk, status, ran=False):
        assert ran or _run(sim, pk) == 0
        assert pk.status[:3].tolist() == [R0.OK, status, R0.OK] and (pk.status[3:] == C.POISON32).all()
        C.check_slots(pk, _got(pk), wanted, (0, 2), 3)
        assert (C.outside_pieces(pk, pk.ws, (0, 2)) == C.POISON_BYTE).all()       # the middle slot's piece among them
    # the aligner's status is not OK -- every one it can leave, and what is none of its codes: SKIPPED, and the slot's
    # frames -- poison here -- and labels are never read
    for st in (R0.BOUNDS, R0.LABEL, 3, R.QUERY, C.SKIPPED, -1, C.POISON32):
        poisoned = frames.copy()
        poisoned[7:12] = C.POISON32
        pk = C.pack(sim, lines, 6, frames=poisoned, align_status={1: st}, labels_edit={1: (2, 999)})
        check(pk, C.SKIPPED)
    # the device's L = 5 over a cap of 4; a cap above L that the device's L still exceeds; L = 0
    check(C.pack(sim, lines, 6, frames=frames, cap_edit={1: 4}), R0.BOUNDS)
    check(C.pack(sim, lines, 6, frames=frames, cap_edit={1: 8}, L_dev={1: 9}), R0.BOUNDS)
    check(C.pack(sim, lines, 6, frames=frames, L_dev={1: 0}), R0.BOUNDS)
    check(C.pack(sim, lines, 6, frames=frames, labels_edit={1: (2, 6)}), R0.LABEL)
    check(C.pack(sim, lines, 6, frames=frames, labels_edit={1: (0, 0)}), R0.LABEL)
    # acc_line outside the chunk's lines, offsets outside their arrays: nothing is read through them
    for name, k, v in (("acc_line", 1, -1), ("acc_line", 1, 6), ("acc_line", 1, 1 << 30), ("lab_off", 1, -1),
                       ("lab_off", 1, 10 ** 9), ("lab_off", 1, 1 << 62)):
        pk = C.pack(sim, lines, 6, frames=frames)
        assert pk.nlines_all == 6
        was = getattr(pk, name)[k]
        getattr(pk, name)[k] = v
        assert _run(sim, pk) == 0
        getattr(pk, name)[k] = was                       # gather looks the lines' rows up where they were
        check(pk, R0.BOUNDS, ran=True)
    for v in (-3, 10 ** 9):
        pk = C.pack(sim, lines, 6, frames=frames)
        pk.row_off_all[pk.slot_line[1]] = v
        check(pk, R0.BOUNDS)
    # a peak edited to decrease, and one outside the line's frames: QUERY
    for i, v in ((3, int(frames[7 + 2, 2]) - 1), (4, 21), (0, -1)):
        edited = frames.copy()
        edited[7 + i, 2] = v
        check(C.pack(sim, lines, 6, frames=edited), R.QUERY)
    # t_first and t_last are not the query: whatever they hold, the answer is the same
    edited = frames.copy()
    edited[:, :2] = C.POISON32
    pk = C.pack(sim, lines, 6, frames=edited)
    assert _run(sim, pk) == 0 and pk.status[:3].tolist() == [0, 0, 0]
    C.check_slots(pk, _got(pk), wanted, (0, 1, 2), 3)


def test_count_limits_the_slots_and_a_negative_count_touches_nothing(sim):
    rng = np.random.default_rng(22)
    lines = _three(rng)
    frames = R0.align_batch(lines)[0]
    wanted = C.answer(lines, frames)
    pk = C.pack(sim, lines, 6, frames=frames, count=2)   # three slots given, two filled
    assert _run(sim, pk) == 0
    assert pk.status[:2].tolist() == [R0.OK, R0.OK] and (pk.status[2:] == C.POISON32).all()
    C.check_slots(pk, _got(pk), wanted, (0, 1), 3)
    assert (C.outside_pieces(pk, pk.ws, (0, 1)) == C.POISON_BYTE).all()
    for count in (0, -1, -(1 << 40)):
        pk = C.pack(sim, lines, 6, frames=frames, count=count)
        assert _run(sim, pk) == 0 and C.untouched(pk), count
    pk = C.pack(sim, lines, 6, frames=frames, count=1 << 40)   # more than the slots the call covers: the covered ones run
    pk.acc_line[3:], pk.L[3:], pk.lab_off[3:], pk.align_status[3:] = -1, 1, 0, 0
    assert _run(sim, pk) == 0 and pk.status.tolist() == [R0.OK] * 3 + [R0.BOUNDS] * 2


def test_host_side_refusals_touch_nothing(sim):
    rng = np.random.default_rng(23)
    lines = _three(rng)[:2]
    frames = R0.align_batch(lines)[0]
    pk = C.pack(sim, lines, 6, frames=frames)
    for what, code, over in C.refusals(pk):
        if over == "misalign":
            over = dict(workspace=pk.ws.ctypes.data + 4)
        assert _run(sim, pk, **over) == code, what
        assert C.untouched(pk), what
    assert _run(sim, pk, nslots=0) == 0 and C.untouched(pk)
    assert _run(sim, pk, nlines_all=0, nslots=0) == 0 and C.untouched(pk)
    # no line can receive a text: nothing to launch, and no workspace is asked for
    assert _run(sim, pk, Lcap_host=np.zeros(pk.nlines_all, np.int32), workspace_bytes=0) == 0 and C.untouched(pk)
    assert _run(sim, pk) == 0 and pk.status[:2].tolist() == [0, 0]
    C.check_slots(pk, _got(pk), C.answer(lines, frames), (0, 1), 2)


def test_workspace_bytes(sim):
    f = sim.ta_forced_posterior_lines_workspace_bytes
    # a forward row of 64 K doubles and 64 K exponents for every label the chunk can hold, K the widest cap's
    assert f(1000, 1) == 1536 * 1000 and f(1000, 63) == 1536 * 1000 and f(1000, 64) == 3072 * 1000
    assert f(7, 127) == 3072 * 7 and f(7, 128) == 6144 * 7 and f(7, 255) == 6144 * 7 and f(7, 256) == 12288 * 7
    assert f(7, 511) == 12288 * 7 and f(7, 512) == 24576 * 7 and f(1 << 40, 1023) == 24576 << 40
    assert f(0, 5) == 0 and f(123, 0) == 0 and f(0, 0) == 0
    for cap, lmax in ((-1, 5), (5, -1), (5, 1024), (1 << 62, 1), (-1, 0)):
        assert f(cap, lmax) == -1
    # never below the single-line call's piece for any text within the cap
    one = _abi.bind(sim, ["ta_forced_posterior_workspace_bytes"]).ta_forced_posterior_workspace_bytes
    for L in (1, 63, 64, 300, 1023):
        assert f(L, L) == one(2 * L + 1, L)
        assert all(f(L, L) >= one(2 * l + 1, l) for l in range(1, L + 1, 7))
