"""ta_forced_align_pages_omit_gated (csrc/ta_forced_page_omit_gated.hip) on the GPU against the checker
tests/forced_page_omit_ref.py: every case of tests/forced_page_omit_cases.py through the library with real device pointers
and the pipeline's caps, and the gate, the caps and the refusals of tests/test_forced_page_omit_gated_sim.py.  Every output
is an integer and is compared for equality; everything is poisoned first.  (The window kernel in front of it on one stream:
tests/test_page_windows_omit_gpu.py.)"""
import numpy as np
import pytest

import forced_page_omit_cases as OC
import forced_page_omit_gated_cases as G
import forced_page_omit_ref as R
from test_forced_page_omit_gated_sim import EMPTY_PAGE, mixed, widest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
UNIT = OC.UNIT


class _Device(object):
    def __init__(self, pk):
        self.pk = pk
        self.t = {name: torch.from_numpy(np.ascontiguousarray(getattr(pk, name))).cuda() for name in G.INPUTS + G.OUTPUTS + ("ws",)}

    def ptr(self, name):
        return self.t[name].data_ptr()

    def call(self, lib, omit, **over):
        return G.call(lib, self.pk, self.ptr, omit, torch.cuda.current_stream().cuda_stream, **over)

    def back(self):
        for name in G.OUTPUTS + ("ws",):
            getattr(self.pk, name)[...] = self.t[name].cpu().numpy()
        return self.pk


@pytest.fixture(scope="module")
def lib():
    from text_alignment_amd import _native
    return _native.lib


@pytest.mark.parametrize("case", OC.cases(), ids=lambda c: c[0])
def test_gated_kernel_equals_the_checker(lib, case):
    """caps as the pipeline passes them, min(n, 1023): the workspace is sized for a wider variant than the windows need"""
    name, no, omit, pages = case
    d = _Device(G.pack(lib, G.slots(pages), no))
    assert d.call(lib, omit) == 0
    want = OC.want(name, pages, omit)
    G.check(d.back(), want)
    if name.startswith(OC.STRICT):
        G.check(d.pk, OC.strict_want(pages))


@pytest.mark.parametrize("case", [c for c in OC.cases() if c[0] in ("window shifts", "mixed K", "window 127", "window 128", "window 513")],
                         ids=lambda c: c[0])
def test_caps_equal_to_the_widest_windows(lib, case):
    name, no, omit, pages = case
    d = _Device(G.pack(lib, [(pg, 0, widest(pg)) for pg in pages], no))
    assert d.call(lib, omit) == 0
    G.check(d.back(), OC.want(name, pages, omit))


def test_gate_caps_and_variants_in_one_call(lib):
    omit = 2 * UNIT
    no, slots, want = mixed(np.random.default_rng(1417))
    d = _Device(G.pack(lib, slots, no))
    assert d.call(lib, omit) == 0
    G.check(d.back(), want)
    # a gated page's numbers are not read: rubbish in its windows, timesteps, rows and pieces changes nothing
    pk = G.pack(lib, slots, no)
    a = int(pk.line_first[1])
    good_T, good_ws = pk.T.copy(), int(pk.ws_off[a])
    pk.lo[a], pk.hi[a], pk.T[a], pk.row_off[a], pk.ws_off[a] = 7, -3, -1, 10 ** 12, -8
    d = _Device(pk)
    assert d.call(lib, omit, T_host=good_T) == 0
    d.back()
    pk.ws_off[a] = good_ws
    G.check(pk, want)
    # the device's cap decides on the device
    pk = G.pack(lib, slots, no)
    host_cap = pk.cap.copy()
    pk.cap[2] = 10
    d = _Device(pk)
    assert d.call(lib, omit, cap_host=host_cap) == 0
    w = list(want)
    w[2] = (R.BOUNDS, None, None)
    G.check(d.back(), w)


def test_host_side_refusals_touch_nothing_and_the_good_call_then_runs(lib):
    from text_alignment_amd import _native
    rng = np.random.default_rng(1418)
    omit = 2 * UNIT
    pages = [OC._page(rng, (12, 11), 8, (0, 3), (4, 8), 6), OC._page(rng, (10, 9, 11), 9, (0, 1, 6), (5, 6, 9), 6)]
    pk = G.pack(lib, G.slots(pages), 6)
    d = _Device(pk)
    EINVAL, ELIMIT = -1, -4

    def arr(name, k, v):
        a = getattr(pk, name).copy()
        a[k] = v
        return a
    for what, code, over in (
            ("omit -1", EINVAL, dict(omit_q=-1)), ("omit above the maximum", EINVAL, dict(omit_q=(1 << 26) + 1)),
            ("null gate", EINVAL, dict(gate=None)), ("null cap_host", EINVAL, dict(cap_host=None)),
            ("negative nlabels", EINVAL, dict(nlabels=-1)), ("no = 129", EINVAL, dict(no=129)),
            ("workspace too small", EINVAL, dict(workspace_bytes=256)),
            ("workspace misaligned", EINVAL, dict(workspace=d.ptr("ws") + 4)),
            ("line_first decreases", EINVAL, dict(line_first_host=np.asarray([0, 6, pk.nlines], np.int64))),
            ("a negative cap", EINVAL, dict(cap_host=arr("cap", 1, -1))), ("cap 1024", ELIMIT, dict(cap_host=arr("cap", 1, 1024))),
            ("T > 5000", ELIMIT, dict(T_host=arr("T", 1, 5001))),
            ("2^20 + 1 characters", ELIMIT, dict(lab_off_host=arr("lab_off", 2, int(pk.lab_off[1]) + (1 << 20) + 1), nlabels=1 << 40))):
        assert d.call(lib, omit, **over) == code, what
    with pytest.raises(_native.NativeArgumentError):
        _native.check(d.call(lib, omit, no=1), "ta_forced_align_pages_omit_gated")
    torch.cuda.synchronize()
    d.back()
    assert (pk.frames == G.POISON32).all() and (pk.score == G.POISON64).all() and (pk.status == G.POISON32).all()
    assert (pk.ws == G.POISON_BYTE).all()
    assert d.call(lib, omit) == 0
    G.check(d.back(), [R.answer(*pg, omit) for pg in pages])
    # a page without lines or text: passed over behind its gate, the device's to refuse without one
    for gate, status in ((1, G.SKIPPED), (0, R.BOUNDS)):
        d = _Device(G.pack(lib, [(pages[0], 0, None), (EMPTY_PAGE, gate, None), (pages[1], 0, None)], 6))
        assert d.call(lib, omit) == 0
        G.check(d.back(), [R.answer(*pages[0], omit), (status, None, None), R.answer(*pages[1], omit)])


def test_workspace_bytes(lib):
    T = np.asarray([3, 8, 9, 1], np.int32)
    f = lambda nl, cap: lib.ta_forced_page_omit_gated_workspace_bytes(nl, T.ctypes.data, cap)      # noqa: E731
    for cap in (0, 63, 64, 127, 128, 255, 256, 511, 512, 1023):
        assert f(4, cap) == lib.ta_forced_page_omit_workspace_bytes(4, T.ctypes.data, lib.ta_forced_page_variant(cap))
    assert f(4, -1) == -1 and f(4, 1024) == -1 and f(0, 5) == -1
