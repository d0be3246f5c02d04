"""ta_refine_columns_omit (csrc/ta_refine.hip, the kOmit instantiation) on the GPU against its checker
tests/refine_omit_ref.py: the cases of tests/refine_omit_cases.py through the library with real device pointers -- what
tests/test_refine_omit_sim.py runs in the host build.  Every output is an integer and is compared for equality;
everything is poisoned first."""
import numpy as np
import pytest

import refine_cases as RC
import refine_omit_cases as C
import refine_omit_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def lib():
    from text_alignment_amd import _native
    return _native.lib


def _columns(lib, pk, call=C.call, names=C.INPUTS + C.OUTPUTS, outputs=C.OUTPUTS, **over):
    t = {name: torch.from_numpy(getattr(pk, name)).cuda() for name in names}
    rc = call(lib, pk, lambda name: t[name].data_ptr(), torch.cuda.current_stream().cuda_stream, **over)
    for name in outputs:
        getattr(pk, name)[...] = t[name].cpu().numpy()
    return rc


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_refine_columns_omit_equals_the_checker(lib, case):
    name, chunk = case
    pk = C.pack(chunk, seed=len(name))
    assert _columns(lib, pk) == 0
    C.compare(pk)


def test_with_every_character_present_it_is_ta_refine_columns(lib):
    for name, chunk in RC.cases():
        pk, strict = C.pack(chunk, seed=len(name)), RC.pack(chunk, seed=len(name))
        assert _columns(lib, pk) == 0
        assert _columns(lib, strict, call=RC.call, names=RC.INPUTS + RC.OUTPUTS, outputs=RC.OUTPUTS) == 0
        for out in RC.OUTPUTS:
            assert np.array_equal(getattr(pk, out), getattr(strict, out)), (name, out)


def test_out_of_bounds_page_and_host_refusals(lib):
    name, chunk = [c for c in C.cases() if c[0] == "refine_cases: three pages"][0]
    pk = C.pack(chunk, seed=1)
    answer = C.want(pk)
    lf0, lf1 = int(pk.line_first[2]), int(pk.line_first[3])
    pk.ops_len[2] = 10 ** 6
    assert _columns(lib, pk) == 0
    assert pk.status[:4].tolist() == [0, 0, R.BOUNDS, 0] and pk.ops_new_len[2] == -1 and pk.idx_new_len[2] == -1
    assert (pk.omitted[lf0:lf1] == C.POISON32).all()
    assert np.array_equal(np.delete(pk.omitted[:pk.nlines], np.r_[lf0:lf1]), np.delete(answer[3], np.r_[lf0:lf1]))
    for q in (0, 1, 3):
        r0, (st, ops, idx) = int(pk.ops_off[q]), answer[0][q]
        assert np.array_equal(pk.ops_new[r0:r0 + len(ops)], ops) and np.array_equal(pk.idx_new[r0:r0 + len(idx)], idx)
    assert (pk.ops_new[int(pk.ops_off[2]):int(pk.ops_off[3])] == C.POISON8).all()
    pk = C.pack(chunk, seed=1)
    assert _columns(lib, pk, box_base=-1) == -1 and _columns(lib, pk, box_base=2 ** 31 - 5) == -4
    assert _columns(lib, pk, frames=None) == -1 and _columns(lib, pk, omitted=None) == -1
    assert (pk.status == C.POISON32).all() and (pk.ops_new == C.POISON8).all() and (pk.omitted == C.POISON32).all()
