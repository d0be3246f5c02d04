"""The two kernels of the pipeline's refinement on the GPU against their checkers: ta_forced_align_lines (csrc/ta_forced.hip,
the cases of tests/forced_cases.py in the layout of tests/forced_lines_cases.py, checker tests/forced_ref.py) and
ta_refine_columns (csrc/ta_refine.hip, the cases of tests/refine_cases.py, checker tests/refine_ref.py) through the
library with real device pointers -- what tests/test_forced_lines_sim.py and tests/test_refine_sim.py run in the host
build.  Every output is an integer and is compared for equality; everything is poisoned first."""
import numpy as np
import pytest

import forced_cases as C
import forced_lines_cases as LC
import forced_ref as R
import refine_cases as RC
import refine_ref as RR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class _Device(object):
    """a packed case's arrays on the device; back() copies the outputs into the packed case"""

    def __init__(self, pk, names, outputs):
        self.pk, self.outputs = pk, outputs
        self.t = {name: torch.from_numpy(getattr(pk, name)).cuda() for name in names}

    def ptr(self, name):
        return self.t[name].data_ptr()

    def back(self):
        for name in self.outputs:
            getattr(self.pk, name)[...] = self.t[name].cpu().numpy()
        return self.pk


@pytest.fixture(scope="module")
def lib():
    from text_alignment_amd import _native
    return _native.lib


def _lines(lib, pk, **over):
    d = _Device(pk, LC.INPUTS + LC.OUTPUTS + ("ws",), LC.OUTPUTS + ("ws",))
    rc = LC.call(lib, pk, d.ptr, torch.cuda.current_stream().cuda_stream, **over)
    d.back()
    return rc


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_forced_align_lines_equals_the_checker(lib, case):
    name, no, lines = case
    pk = LC.pack(lib, lines, no, seed=len(name))
    assert _lines(lib, pk) == 0
    frames, score = C.want(name, lines)
    n = len(lines)
    assert pk.status[:n].tolist() == [R.OK] * n
    assert (pk.status[n:] == LC.POISON32).all() and (pk.score[n:] == LC.POISON64).all()
    assert np.array_equal(C.gather(pk, pk.frames), frames)
    assert np.array_equal(pk.score[:n], score)


def test_forced_align_lines_refusals_and_counts(lib):
    rng = np.random.default_rng(15)
    lines = [(C.probs(rng, 30, 6), C.text(rng, 7, 6)), (C.probs(rng, 21, 6), C.text(rng, 5, 6)),
             (C.probs(rng, 140, 6), C.text(rng, 66, 6))]
    frames, score = R.align_batch(lines)
    keep = np.r_[0:7, 12:78]
    for edit, status in ((dict(cap_edit={1: 4}), R.BOUNDS), (dict(cap_edit={1: 8}, L_dev={1: 9}), R.BOUNDS),
                         (dict(labels_edit={1: (2, 6)}), R.LABEL)):
        pk = LC.pack(lib, lines, 6, **edit)
        assert _lines(lib, pk) == 0
        assert pk.status[:3].tolist() == [R.OK, status, R.OK]
        got = C.gather(pk, pk.frames)
        assert np.array_equal(got[keep], frames[keep]) and (got[7:12] == LC.POISON32).all()
        assert pk.score[1] == LC.POISON64 and np.array_equal(pk.score[[0, 2]], score[[0, 2]])
    pk = LC.pack(lib, lines, 6)
    pk.acc_line[1] = 6                                   # one past the chunk's lines
    assert _lines(lib, pk) == 0 and pk.status[:3].tolist() == [R.OK, R.BOUNDS, R.OK]
    pk = LC.pack(lib, lines, 6, count=2)
    assert _lines(lib, pk) == 0
    assert pk.status[:2].tolist() == [R.OK, R.OK] and (pk.status[2:] == LC.POISON32).all()
    assert (C.gather(pk, pk.frames)[12:] == LC.POISON32).all()
    for count in (0, -1):
        pk = LC.pack(lib, lines, 6, count=count)
        assert _lines(lib, pk) == 0 and LC.untouched(pk)
    pk = LC.pack(lib, lines[:2], 6)
    for what, code, over in LC.refusals(pk):
        if over != "misalign":
            d = _Device(pk, LC.INPUTS + LC.OUTPUTS + ("ws",), ())
            assert LC.call(lib, pk, d.ptr, torch.cuda.current_stream().cuda_stream, **over) == code, what


def _columns(lib, pk, **over):
    d = _Device(pk, RC.INPUTS + RC.OUTPUTS, RC.OUTPUTS)
    rc = RC.call(lib, pk, d.ptr, torch.cuda.current_stream().cuda_stream, **over)
    d.back()
    return rc


@pytest.mark.parametrize("case", RC.cases(), ids=lambda c: c[0])
def test_refine_columns_equals_the_checker(lib, case):
    name, chunk = case
    pk = RC.pack(chunk, seed=len(name))
    assert _columns(lib, pk) == 0
    RC.compare(pk)


def test_refine_columns_out_of_bounds_page_and_host_refusals(lib):
    name, chunk = [c for c in RC.cases() if c[0] == "three pages"][0]
    pk = RC.pack(chunk, seed=1)
    answer = RC.want(pk)
    pk.ops_len[2] = 10 ** 6
    assert _columns(lib, pk) == 0
    assert pk.status[:4].tolist() == [0, 0, RR.BOUNDS, 0] and pk.ops_new_len[2] == -1 and pk.idx_new_len[2] == -1
    for q in (0, 1, 3):
        r0, (st, ops, idx) = int(pk.ops_off[q]), answer[0][q]
        assert np.array_equal(pk.ops_new[r0:r0 + len(ops)], ops) and np.array_equal(pk.idx_new[r0:r0 + len(idx)], idx)
    assert (pk.ops_new[int(pk.ops_off[2]):int(pk.ops_off[3])] == RC.POISON8).all()
    pk = RC.pack(chunk, seed=1)
    assert _columns(lib, pk, box_base=-1) == -1 and _columns(lib, pk, box_base=2 ** 31 - 5) == -4
    assert _columns(lib, pk, plain=None) == -1
    assert (pk.status == RC.POISON32).all() and (pk.ops_new == RC.POISON8).all()
