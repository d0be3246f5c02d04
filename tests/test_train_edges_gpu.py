"""The training kernels (csrc/ta_train.hip) on the GPU at their edges, against the float64 checker tests/train_ref.py
under the bound taken from the checker alone (train_ref.bound64: 64 x max(noise64, 4 ulp of the array's largest
reference magnitude), noise64 being the float64 checker's distance from its own long-double run).  The cases are those of
tests/train_cases.py, which tests/test_train_cases.py shows able to fail and tests/test_train_sim.py runs on the host
build: lattices of up to nine passes over the states, S == T, empty texts, T = 1; batches whose output layer has a row
tail and whose lines are 1, 2 and 3 steps long; 2, 3, 127 and 128 classes; a model past every clamp; and the C ABI with
a caller's own layout, every output poisoned, and a line the device alone refuses between two good ones.

Slowest test here on an MI355X: 1.3 s (a T = S = 2049 lattice; its long-double checker run is nearly all of it).  Worst
quotient error / max(noise64, 4 ulp) recorded in profiles/train_agreement.json: 17.3 of the 64 allowed (the summed squared
deltas of a 128-class line)."""
import numpy as np
import pytest

import train_cases as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from text_alignment_amd import _native
    return C.bind(_native.lib)


@pytest.mark.parametrize("name", [c[0] for c in C.lattice_cases()])
def test_lattice_equals_the_checker(name):
    w = C.lattice_want(name)
    got = C.device_lattice(name)
    print(name, {k: "%.3g" % (64 * q) for k, q in w.miss(got).items()}, "x max(noise64, 4 ulp); noise64", w.noise)
    w.check(got, name)
    assert np.abs(got["aligned"].sum(axis=1) - 1.0).max() <= w.bound["aligned"]


@pytest.mark.parametrize("name", [c[0] for c in C.net_cases()])
def test_align_and_gradients_equal_the_checker(name):
    wants = C.net_want(name)
    got = C.device_net(name)
    assert len(got) == len(wants)
    for b, (w, g) in enumerate(zip(wants, got)):
        print(name, b, "worst %.3g x max(noise64, 4 ulp)" % (64 * max(w.miss(g).values())))
        w.check(g, "%s line %d" % (name, b))
        assert np.abs(g["aligned"].sum(axis=1) - 1.0).max() <= w.bound["aligned"]
    if name == "57 rows":                                  # its first line has one timestep: no step has a predecessor
        assert got[0]["probs"].shape[0] == 1
        assert all((got[0][d + k] == 0).all() for d in ("fwd ", "rev ") for k in ("WIP", "WFP", "WOP"))


def test_ctc_abi_with_a_callers_layout_and_lines_refused_on_the_device(lib):
    """three lines stored out of order with gaps in rows, labels and workspace; then the middle line spoiled in the
    device's copy of one input alone (the host's T and L stay right, so the call itself is accepted): its err is NaN, its
    rows and its workspace piece keep their poison, both neighbours equal the checker.  Every spoiled line is refused by
    the kernel's own bounds check before it reads or writes anything of the line."""
    no, lines = C.three_lattice_lines()
    wants = C.three_lattice_wants()
    pk = C.pack_ctc(lib, lines, no)
    d = C.Device(pk, C.CTC_INPUTS, C.CTC_OUTPUTS)
    assert C.call_ctc(lib, pk, d.ptr, d.stream()) == 0
    C.check_ctc(d.back(), pk, wants, what="three lines")
    for what, name, k, v in C.ctc_edits(pk):
        pk = C.pack_ctc(lib, lines, no)
        spoiled = getattr(pk, name).copy()
        spoiled[k] = v
        d = C.Device(pk, C.CTC_INPUTS, C.CTC_OUTPUTS, **{name: spoiled})
        assert C.call_ctc(lib, pk, d.ptr, d.stream()) == 0, what
        C.check_ctc(d.back(), pk, wants, refused=(1,), what=what)


@pytest.mark.parametrize("name", [c[0] for c in C.net_cases()])
def test_lstm_abi_with_a_callers_layout(lib, name):
    """forward and backward on lines stored out of order with gap rows: states, hout, probs, gate errors and the
    peepholes' gradients against the checker, the gap rows still poison"""
    _, model, lines, _ = C.net_case(name)
    wants = C.net_want(name)
    pk = C.pack_net(model, lines, wants)
    d = C.Device(pk, C.NET_INPUTS, C.NET_OUTPUTS)
    assert C.call_forward(lib, pk, d.ptr, d.stream()) == 0 and C.call_backward(lib, pk, d.ptr, d.stream()) == 0
    C.check_net(d.back(), pk, wants, what=name)


def test_lstm_abi_refuses_a_line_on_the_device_between_good_neighbours(lib):
    _, model, lines, _ = C.net_case("55 rows")
    wants = C.net_want("55 rows")
    for what, name, k, v in C.net_edits(C.pack_net(model, lines, wants)):
        pk = C.pack_net(model, lines, wants)
        spoiled = getattr(pk, name).copy()
        spoiled[k] = v
        d = C.Device(pk, C.NET_INPUTS, C.NET_OUTPUTS, **{name: spoiled})
        assert C.call_forward(lib, pk, d.ptr, d.stream()) == 0 and C.call_backward(lib, pk, d.ptr, d.stream()) == 0, what
        C.check_net(d.back(), pk, wants, refused=(1,), what=what)
