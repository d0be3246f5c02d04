"""ta_posterior_pages on the GPU: the pages of tests/test_posterior_pages_sim.py through the library with real device
pointers against tests/refine_post_ref.py, and the device's division and ldexp against numpy's -- synthetic pairs fed
straight into the kernel, the expected values from forced.posterior_values on the host, everything compared through its
int64 view."""
import numpy as np
import pytest

import refine_post_cases as C
import refine_post_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class _Device(object):
    """a packed case's arrays on the device"""

    def __init__(self, pk):
        self.pk = pk
        self.t = {name: torch.from_numpy(getattr(pk, name)).cuda() for name in C.INPUTS + C.OUTPUTS}

    def ptr(self, name):
        return self.t[name].data_ptr()

    def call(self, lib, **over):
        return C.call(lib, self.pk, self.ptr, torch.cuda.current_stream().cuda_stream, **over)

    def host(self, name):
        return self.t[name].cpu().numpy()

    def back(self):
        for name in C.OUTPUTS:
            setattr(self.pk, name, self.host(name))


@pytest.fixture(scope="module")
def lib():
    from text_alignment_amd import _native
    return _native.lib


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_posterior_pages_equals_the_checker(lib, case):
    name, pages = case
    d = _Device(C.pack(pages, seed=len(name)))
    assert d.call(lib) == 0
    d.back()
    C.compare(d.pk)


def test_refusals_on_the_device_and_on_the_host(lib):
    name, pages = [c for c in C.cases() if c[0] == "three pages"][0]
    for count in (-1, 1):
        d = _Device(C.pack(pages, seed=3, count=count))
        assert d.call(lib) == 0
        d.back()
        C.compare(d.pk)
    for field, at, v, hit in (("t_off", 3, 1 << 40, (2, 3)), ("line_first", 2, -2, (1, 2)), ("syl_off", 4, -7, (3,))):
        pk = C.pack(pages, seed=1)
        answer, was = C.want(pk), getattr(pk, field)[at]
        getattr(pk, field)[at] = v
        d = _Device(pk)
        assert d.call(lib) == 0
        d.back()
        getattr(pk, field)[at] = was
        assert [int(pk.status[p]) for p in hit] == [R.BOUNDS] * len(hit), (field, at)
        C.compare(pk, answer, skip=hit)
    d = _Device(C.pack(pages))
    for over in (dict(own_m=None), dict(z_x=None), dict(status=None), dict(nsyl=-1), dict(nprob=-1)):
        assert d.call(lib, **over) == -1
    assert d.call(lib, nlines=(1 << 24) + 1) == -4 and d.call(lib, nprob=0) == 0
    torch.cuda.synchronize()
    assert (d.host("char_post").view(np.int64) == C.POISON64).all() and (d.host("status") == C.POISON32).all()
    assert d.call(lib) == 0
    d.back()
    C.compare(d.pk)


def test_the_devices_division_and_ldexp_are_numpys_bit_for_bit(lib):
    """synthetic pairs fed straight in (refine_post_cases.division_pages): own = z, a zero mass, quotients that round,
    exponent differences down through the subnormal range; expected values from forced.posterior_values on the host"""
    from text_alignment_amd import forced
    pages = C.division_pages()
    d = _Device(C.pack(pages, seed=5))
    assert d.call(lib) == 0
    d.back()
    C.check_division(d.pk, pages, forced.posterior_values)
