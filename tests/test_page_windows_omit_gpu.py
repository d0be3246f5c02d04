"""ta_page_windows_omit (csrc/ta_page_windows_omit.hip) on the GPU: the pages of tests/page_windows_cases.py and the limit
pages of tests/page_windows_omit_cases.py through the library with real device pointers against
forced.page_scope_eligibility(..., omit=True), every output poisoned first; and the two kernels of page scope with omission
back to back on one stream -- ta_page_windows_omit, then ta_forced_align_pages_omit_gated on the lo / hi / reason it left
on the device."""
import numpy as np
import pytest

import forced_page_cases as FC
import forced_page_omit_cases as OC
import forced_page_omit_gated_cases as G
import forced_page_omit_ref as R
import page_windows_cases as C
import page_windows_omit_cases as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class _Device(object):
    """a packed case's arrays on the device; back() copies the outputs into the packed case"""

    def __init__(self, pk, names, outputs):
        self.pk, self.outputs = pk, outputs
        self.t = {name: torch.from_numpy(np.ascontiguousarray(getattr(pk, name))).cuda() for name in names}

    def ptr(self, name):
        return self.t[name].data_ptr()

    def back(self):
        for name in self.outputs:
            getattr(self.pk, name)[...] = self.t[name].cpu().numpy()
        return self.pk


def _windows(pk):
    return _Device(pk, C.INPUTS + C.OUTPUTS, C.OUTPUTS)


@pytest.fixture(scope="module")
def lib():
    from text_alignment_amd import _native
    return _native.lib


def _call(lib, d, m, **over):
    return O.call(lib, d.pk, d.ptr, m, torch.cuda.current_stream().cuda_stream, **over)


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_kernel_equals_the_host_rule(lib, case):
    name, margin, pages = case
    d = _windows(C.pack(pages))
    assert _call(lib, d, margin) == 0
    C.check(d.back(), O.want(d.pk.pages, margin))


@pytest.mark.parametrize("case", O.limit_cases(), ids=lambda c: c[0])
def test_the_limits_of_the_lattice_with_omission(lib, case):
    name, margin, pages, reasons = case
    d = _windows(C.pack(pages))
    wanted = O.want(d.pk.pages, margin)
    assert [r for r, _ in wanted] == [0] + reasons
    assert _call(lib, d, margin) == 0
    C.check(d.back(), wanted)


def test_host_side_refusals_touch_nothing_and_the_good_call_then_runs(lib):
    from text_alignment_amd import _native
    d = _windows(C.pack([C.page(C.EXAMPLE, 37, T=[9, 9, 9, 9])]))
    for over in (dict(table=None), dict(plain=None), dict(reason=None), dict(lo=None), dict(npages=-1), dict(nlines=-1),
                 dict(t_len=-1), dict(margin=-1)):
        assert _call(lib, d, 16, **over) == -1, over
    with pytest.raises(_native.NativeArgumentError):
        _native.check(_call(lib, d, 16, margin=-2), "ta_page_windows_omit")
    assert _call(lib, d, 16, npages=0) == 0
    torch.cuda.synchronize()
    pk = d.back()
    assert (pk.lo == C.POISON32).all() and (pk.hi == C.POISON32).all() and (pk.reason == C.POISON32).all()
    assert _call(lib, d, 16) == 0
    C.check(d.back(), O.want(pk.pages, 16))
    assert pk.reason.tolist() == [0, 0]


def test_windows_and_gated_aligner_back_to_back_on_one_stream(lib):
    """harvest rows and probabilities for five pages; ta_page_windows_omit writes lo / hi / reason,
    ta_forced_align_pages_omit_gated reads them where they lie: frames, score and status equal the checker's on the windows
    the host rule makes, a page with a reason is passed over, and a page whose transcript has more characters than its
    lines have frames -- PAGE_FRAMES under the strict rule -- has windows and a path"""
    rng = np.random.default_rng(1419)
    no, margin, omit = 7, 2, 2 * OC.UNIT
    spec = [dict(Ts=(30, 34, 28), cores=[(0, 9), (9, 8), (17, 10)]),                 # eligible, K = 2
            dict(Ts=(30, 30), cores=[(0, 9), (9, 9)], plain=False),                  # NOT_PLAIN: passed over
            dict(Ts=(300, 40), cores=[(0, 130), (130, 9)]),                          # eligible, K = 8 (a window of 132)
            dict(Ts=(3, 3), cores=[(0, 9), (9, 9)]),                                 # more characters than frames: eligible
            dict(Ts=(25, 9, 31), cores=[(0, 8), None, (11, 9)])]                     # an EMPTY line in the middle
    w_pages, slots = [], []
    for s in spec:
        n = max(a + L for a, L in [c for c in s["cores"] if c])
        rows = [[0, c[0], c[1]] if c else [C.EMPTY, 0, 0] for c in s["cores"]]
        w_pages.append(C.page(rows, n, T=s["Ts"], plain=s.get("plain", True), classes=FC.text(rng, n, no)))
    wanted = O.want(w_pages, margin)
    assert [r for r, _ in wanted] == [0, 1, 0, 0, 0] and C.want(w_pages, margin)[3][0] == 6
    for s, pg, (reason, win) in zip(spec, w_pages, wanted):
        Ps = [FC.probs(rng, T, no) for T in s["Ts"]]
        lo, hi = win if win is not None else ([0] * len(Ps), [0] * len(Ps))
        slots.append(((Ps, pg["classes"], lo, hi), reason, None))
    want = G.want(slots, omit)
    assert [w[0] for w in want] == [R.OK, G.SKIPPED, R.OK, R.OK, R.OK]
    assert (want[3][2][:, 0] == R.OMITTED).sum() >= 12      # 18 characters on 6 frames
    wk = C.pack(w_pages, front=False)
    gk = G.pack(lib, slots, no)
    assert np.array_equal(wk.line_first, gk.line_first) and np.array_equal(wk.t_off + 2, gk.lab_off)
    gk.lo[:], gk.hi[:], gk.gate[:] = C.POISON32, C.POISON32, C.POISON32      # the aligner gets them from the window kernel
    w, g = _windows(wk), _Device(gk, G.INPUTS + G.OUTPUTS + ("ws",), G.OUTPUTS + ("ws", "lo", "hi", "gate"))
    stream = torch.cuda.current_stream().cuda_stream
    # ONE set of lo / hi / reason on the device: the window kernel's outputs are the aligner's inputs
    assert O.call(lib, wk, w.ptr, margin, stream, lo=g.ptr("lo"), hi=g.ptr("hi"), reason=g.ptr("gate")) == 0
    assert G.call(lib, gk, g.ptr, omit, stream) == 0
    g.back()
    for p, (reason, win) in enumerate(wanted):
        a, b = int(gk.line_first[p]), int(gk.line_first[p + 1])
        assert int(gk.gate[p]) == reason
        if reason == 0:
            assert np.array_equal(gk.lo[a:b], win[0]) and np.array_equal(gk.hi[a:b], win[1])
        else:
            assert (gk.lo[a:b] == C.POISON32).all() and (gk.hi[a:b] == C.POISON32).all()
    G.check(gk, want)
