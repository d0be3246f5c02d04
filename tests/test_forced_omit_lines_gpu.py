"""ta_forced_align_omit_lines (csrc/ta_forced_omit.hip, the slot variants) on the GPU against the checker
tests/forced_omit_ref.py: every case of tests/forced_omit_cases.py in the layout of tests/forced_omit_lines_cases.py
through the library with real device pointers -- what tests/test_forced_omit_lines_sim.py runs in the host build.  Every
output is an integer and is compared for equality; everything is poisoned first."""
import numpy as np
import pytest

import forced_cases as C0
import forced_omit_cases as OC
import forced_omit_lines_cases as LC
import forced_omit_ref as R
import forced_ref as R0

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
UNIT = OC.UNIT
NAMES = LC.INPUTS + LC.OUTPUTS + ("ws",)


class _Device(object):
    """a packed case's arrays on the device; back() copies the outputs and the workspace into the packed case"""

    def __init__(self, pk):
        self.pk = pk
        self.t = {name: torch.from_numpy(getattr(pk, name)).cuda() for name in NAMES}

    def ptr(self, name):
        return self.t[name].data_ptr()

    def call(self, lib, omit, **over):
        return LC.call(lib, self.pk, self.ptr, omit, torch.cuda.current_stream().cuda_stream, **over)

    def back(self):
        for name in LC.OUTPUTS + ("ws",):
            getattr(self.pk, name)[...] = self.t[name].cpu().numpy()
        return self.pk


@pytest.fixture(scope="module")
def lib():
    from text_alignment_amd import _native
    return _native.lib


def _run(lib, pk, omit, **over):
    d = _Device(pk)
    rc = d.call(lib, omit, **over)
    d.back()
    return rc


@pytest.mark.parametrize("case", OC.cases(), ids=lambda c: c[0])
def test_kernel_equals_the_checker(lib, case):
    name, no, omit, lines = case
    pk = LC.pack(lib, lines, no, seed=len(name))
    assert _run(lib, pk, omit) == 0
    frames, score = OC.want(name, lines, omit)
    n = len(lines)
    assert pk.status[:n].tolist() == [R0.OK] * n
    assert (pk.status[n:] == LC.POISON32).all() and (pk.score[n:] == LC.POISON64).all()
    assert np.array_equal(C0.gather(pk, pk.frames), frames)
    assert np.array_equal(pk.score[:n], score)
    if name == OC.STRICT:
        strict_frames, strict_score = R0.align_batch(lines)
        assert np.array_equal(frames, strict_frames) and np.array_equal(score, strict_score)


def _three(rng):
    return [(C0.probs(rng, 30, 6), C0.text(rng, 7, 6)), (C0.probs(rng, 21, 6), C0.text(rng, 5, 6)),
            (C0.probs(rng, 140, 6), C0.text(rng, 66, 6))]


def test_a_slot_refused_through_its_data_leaves_its_neighbours_alone(lib):
    rng = np.random.default_rng(15)
    omit = 2 * UNIT
    lines = _three(rng)
    frames, score = R.align_batch(lines, omit)
    keep = np.r_[0:7, 12:78]

    def check(pk, status):
        assert pk.status[:3].tolist() == [R0.OK, status, R0.OK]
        got = C0.gather(pk, pk.frames)
        assert np.array_equal(got[keep], frames[keep]) and (got[7:12] == LC.POISON32).all()
        assert pk.score[1] == LC.POISON64 and np.array_equal(pk.score[[0, 2]], score[[0, 2]])
    for edit, status in ((dict(cap_edit={1: 4}), R0.BOUNDS), (dict(cap_edit={1: 8}, L_dev={1: 9}), R0.BOUNDS),
                         (dict(L_dev={1: 0}), R0.BOUNDS), (dict(labels_edit={1: (2, 6)}), R0.LABEL)):
        pk = LC.pack(lib, lines, 6, **edit)
        assert _run(lib, pk, omit) == 0
        check(pk, status)
    for name, k, v in (("acc_line", 1, -1), ("acc_line", 1, 6), ("lab_off", 1, -1), ("lab_off", 1, 10 ** 9)):
        pk = LC.pack(lib, lines, 6)
        was = getattr(pk, name)[k]
        getattr(pk, name)[k] = v
        assert _run(lib, pk, omit) == 0
        getattr(pk, name)[k] = was                       # gather looks the lines' rows up where they were
        check(pk, R0.BOUNDS)
    for name, v in (("row_off_all", 10 ** 9), ("ws_off_all", 8), ("ws_off_all", 10 ** 12)):
        pk = LC.pack(lib, lines, 6)
        a = int(pk.ws_off_all[pk.slot_line[1]])
        getattr(pk, name)[pk.slot_line[1]] = v
        assert _run(lib, pk, omit) == 0
        check(pk, R0.BOUNDS)
        assert (pk.ws[a:a + 256] == LC.POISON_BYTE).all()  # the piece the refused slot would have had stays poison


def test_count_limits_the_slots_and_a_negative_count_touches_nothing(lib):
    rng = np.random.default_rng(16)
    omit = 2 * UNIT
    lines = _three(rng)
    frames, score = R.align_batch(lines, omit)
    pk = LC.pack(lib, lines, 6, count=2)
    assert _run(lib, pk, omit) == 0
    assert pk.status[:2].tolist() == [R0.OK, R0.OK] and (pk.status[2:] == LC.POISON32).all()
    got = C0.gather(pk, pk.frames)
    assert np.array_equal(got[:12], frames[:12]) and (got[12:] == LC.POISON32).all()
    assert np.array_equal(pk.score[:2], score[:2]) and (pk.score[2:] == LC.POISON64).all()
    for count in (0, -1, -(1 << 40)):
        pk = LC.pack(lib, lines, 6, count=count)
        assert _run(lib, pk, omit) == 0 and LC.untouched(pk)


def test_host_side_refusals_touch_nothing_and_the_good_call_then_runs(lib):
    from text_alignment_amd import _native
    rng = np.random.default_rng(17)
    omit = 2 * UNIT
    lines = _three(rng)[:2]
    pk = LC.pack(lib, lines, 6)
    d = _Device(pk)
    for what, code, over in LC.refusals(pk):
        if over == "misalign":
            over = dict(workspace=d.ptr("ws") + 4)
        assert d.call(lib, omit, **over) == code, what
    with pytest.raises(_native.NativeArgumentError):
        _native.check(d.call(lib, -5), "ta_forced_align_omit_lines")
    assert d.call(lib, omit, nslots=0) == 0 and d.call(lib, omit, Lcap_host=np.zeros(pk.nlines_all, np.int32)) == 0
    torch.cuda.synchronize()
    assert LC.untouched(d.back())
    assert d.call(lib, omit) == 0
    d.back()
    assert pk.status[:2].tolist() == [0, 0]
    assert np.array_equal(C0.gather(pk, pk.frames), R.align_batch(lines, omit)[0])
