"""The training kernels without a GPU: tests/native/sim_train.cpp compiles csrc/ta_train.hip ITSELF for the host (a
workgroup = the launch's 512, 128 or 256 lanes that meet at every barrier; tests/native/hipshim_wg) and every case of
tests/train_cases.py goes through ta_ctc_align, ta_lstm_train_forward and ta_lstm_train_backward with host pointers, in
a caller's own layout with every output poisoned, under the bound the real kernels are held to (train_ref.bound64).
This is what runs the lattice's second to ninth pass over the states, the output layer's row tail, T = 1, 2 and 3
through the recurrences, the clamps, and the kernels' own refusals."""
import pytest

import simlib
import train_cases as C

_DEPS = [simlib.NAT + "hipshim_wg/hip/hip_runtime.h", simlib.CSRC + "ta_train.hip", simlib.CSRC + "ta_common.h",
         simlib.HEADER]


@pytest.fixture(scope="module")
def sim():
    return C.bind(simlib.load("train", _DEPS, flags=["-ffp-contract=off"], include=["hipshim_wg"]))


def _ptr(pk, **over):
    """host pointers of a packing; over: arrays that stand in for the device's copy of an input"""
    return lambda name: C._p(over[name] if name in over else getattr(pk, name))


@pytest.mark.parametrize("name", [c[0] for c in C.lattice_cases()])
def test_host_build_of_the_lattice_equals_the_checker(sim, name):
    _, P, cs = C.lattice_case(name)
    pk = C.pack_ctc(sim, [(P, cs)], P.shape[1])
    assert C.call_ctc(sim, pk, _ptr(pk)) == 0
    C.check_ctc(pk, pk, [C.lattice_want(name)], what=name)


def test_lattice_lines_out_of_order_and_the_refusals_between_them(sim):
    no, lines = C.three_lattice_lines()
    wants = C.three_lattice_wants()
    pk = C.pack_ctc(sim, lines, no)
    assert list(pk.row_off) != sorted(pk.row_off) and list(pk.ws_off) != sorted(pk.ws_off)
    assert C.call_ctc(sim, pk, _ptr(pk)) == 0
    C.check_ctc(pk, pk, wants, what="three lines")
    for what, name, k, v in C.ctc_edits(pk):
        pk = C.pack_ctc(sim, lines, no)
        spoiled = getattr(pk, name).copy()
        spoiled[k] = v
        assert C.call_ctc(sim, pk, _ptr(pk, **{name: spoiled})) == 0, what
        C.check_ctc(pk, pk, wants, refused=(1,), what=what)


@pytest.mark.parametrize("name", [c[0] for c in C.net_cases()])
def test_host_build_of_the_recurrences_equals_the_checker(sim, name):
    _, model, lines, _ = C.net_case(name)
    wants = C.net_want(name)
    pk = C.pack_net(model, lines, wants)
    assert C.call_forward(sim, pk, _ptr(pk)) == 0 and C.call_backward(sim, pk, _ptr(pk)) == 0
    C.check_net(pk, pk, wants, what=name)
    if name == "57 rows":
        assert (pk.dpeep[0] == 0).all()                    # T = 1: no step has a predecessor


def test_recurrences_refuse_a_line_between_good_neighbours(sim):
    _, model, lines, _ = C.net_case("55 rows")
    wants = C.net_want("55 rows")
    for what, name, k, v in C.net_edits(C.pack_net(model, lines, wants)):
        pk = C.pack_net(model, lines, wants)
        spoiled = getattr(pk, name).copy()
        spoiled[k] = v
        ptr = _ptr(pk, **{name: spoiled})
        assert C.call_forward(sim, pk, ptr) == 0 and C.call_backward(sim, pk, ptr) == 0, what
        C.check_net(pk, pk, wants, refused=(1,), what=what)

