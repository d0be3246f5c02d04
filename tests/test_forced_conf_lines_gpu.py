"""ta_forced_confidence_lines and ta_confidence_pages on the GPU: the case tables of tests/test_forced_conf_lines_sim.py
and tests/test_refine_conf_sim.py through the library with real device pointers -- every output and the workspace
poisoned -- against the checkers tests/forced_conf_ref.py and tests/refine_conf_ref.py.  Every output is an integer and is
compared for equality."""
import numpy as np
import pytest

import forced_cases as C0
import forced_conf_cases as CC
import forced_conf_lines_cases as C
import forced_conf_ref as R
import forced_ref as R0
import refine_conf_cases as PC
import refine_conf_ref as PR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class _Device(object):
    """a packed case's arrays on the device"""

    def __init__(self, pk, mod):
        self.pk, self.mod = pk, mod
        names = mod.INPUTS + mod.OUTPUTS + (("ws",) if hasattr(pk, "ws") else ())
        self.t = {name: torch.from_numpy(getattr(pk, name)).cuda() for name in names}

    def ptr(self, name):
        return self.t[name].data_ptr()

    def call(self, lib, **over):
        return self.mod.call(lib, self.pk, self.ptr, torch.cuda.current_stream().cuda_stream, **over)

    def host(self, name):
        return self.t[name].cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    from text_alignment_amd import _native
    return _native.lib


# ---- ta_forced_confidence_lines ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CC.cases(), ids=lambda c: c[0])
def test_the_indexed_entry_equals_the_checker_at_the_aligners_peaks(lib, case):
    name, no, lines = case
    d = _Device(C.pack(lib, lines, no, frames=C0.want(name, lines)[0], seed=len(name)), C)
    assert d.call(lib) == 0
    C.check_case(d.pk, name, lines, d.host("confidence"), d.host("rival"), d.host("status"), d.host("ws"))


def _three(rng):
    return [(C0.probs(rng, 30, 6), C0.text(rng, 7, 6)), (C0.probs(rng, 21, 6), C0.text(rng, 5, 6)),
            (C0.probs(rng, 140, 6), C0.text(rng, 66, 6))]


def _answer(lines, frames):
    off = np.cumsum([0] + [len(cs) for _, cs in lines])
    return R.query_batch(lines, [frames[a:b, 2] for a, b in zip(off[:-1], off[1:])])


def test_a_slot_the_aligner_refused_is_skipped_and_one_refused_here_leaves_its_neighbours_alone(lib):
    rng = np.random.default_rng(21)
    lines = _three(rng)
    frames = R0.align_batch(lines)[0]
    conf, rival = _answer(lines, frames)
    keep = np.r_[0:7, 12:78]
    poisoned = frames.copy()
    poisoned[7:12] = C.POISON32
    decreasing, outside = frames.copy(), frames.copy()
    decreasing[7 + 3, 2] = frames[7 + 2, 2] - 1
    outside[7 + 4, 2] = 21
    packs = [(C.pack(lib, lines, 6, frames=poisoned, align_status={1: st}, labels_edit={1: (2, 999)}), C.SKIPPED)
             for st in (R0.BOUNDS, C.SKIPPED, -1)]
    packs += [(C.pack(lib, lines, 6, frames=frames, cap_edit={1: 4}), R0.BOUNDS),
              (C.pack(lib, lines, 6, frames=frames, L_dev={1: 0}), R0.BOUNDS),
              (C.pack(lib, lines, 6, frames=frames, labels_edit={1: (2, 6)}), R0.LABEL),
              (C.pack(lib, lines, 6, frames=decreasing), R.QUERY), (C.pack(lib, lines, 6, frames=outside), R.QUERY)]
    for name, v in (("acc_line", -1), ("acc_line", 6), ("lab_off", -1), ("lab_off", 1 << 62)):
        pk = C.pack(lib, lines, 6, frames=frames)
        pk.edit = (name, getattr(pk, name)[1])
        getattr(pk, name)[1] = v
        packs.append((pk, R0.BOUNDS))
    for pk, status in packs:
        d = _Device(pk, C)
        assert d.call(lib) == 0
        if hasattr(pk, "edit"):                          # gather looks the lines' rows up where they were
            getattr(pk, pk.edit[0])[1] = pk.edit[1]
        st = d.host("status")
        assert st[:3].tolist() == [R0.OK, status, R0.OK] and (st[3:] == C.POISON32).all()
        for name, want, poison in (("confidence", conf, C.POISON64), ("rival", rival, C.POISON32)):
            got = CC.gather(pk, d.host(name), poison)
            assert np.array_equal(got[keep], want[keep]) and (got[7:12] == poison).all()
        assert (C.outside_pieces(pk, d.host("ws"), (0, 2)) == C.POISON_BYTE).all()


def test_count_limits_the_slots_and_a_negative_count_touches_nothing(lib):
    rng = np.random.default_rng(22)
    lines = _three(rng)
    frames = R0.align_batch(lines)[0]
    conf, _ = _answer(lines, frames)
    d = _Device(C.pack(lib, lines, 6, frames=frames, count=2), C)
    assert d.call(lib) == 0
    st = d.host("status")
    assert st[:2].tolist() == [R0.OK, R0.OK] and (st[2:] == C.POISON32).all()
    got = CC.gather(d.pk, d.host("confidence"), C.POISON64)
    assert np.array_equal(got[:12], conf[:12]) and (got[12:] == C.POISON64).all()
    for count in (0, -1, -(1 << 40)):
        d = _Device(C.pack(lib, lines, 6, frames=frames, count=count), C)
        assert d.call(lib) == 0
        assert C.untouched(d.pk, ws=d.host("ws"), **{name: d.host(name) for name in C.OUTPUTS}), count


def test_host_side_refusals_touch_nothing_and_the_good_call_then_runs(lib):
    rng = np.random.default_rng(23)
    lines = _three(rng)[:2]
    frames = R0.align_batch(lines)[0]
    d = _Device(C.pack(lib, lines, 6, frames=frames), C)
    for what, code, over in C.refusals(d.pk):
        if over == "misalign":
            over = dict(workspace=d.ptr("ws") + 4)
        assert d.call(lib, **over) == code, what
    assert d.call(lib, nslots=0) == 0
    assert d.call(lib, Lcap_host=np.zeros(d.pk.nlines_all, np.int32)) == 0
    torch.cuda.synchronize()
    assert C.untouched(d.pk, ws=d.host("ws"), **{name: d.host(name) for name in C.OUTPUTS})
    assert d.call(lib) == 0
    assert d.host("status")[:2].tolist() == [0, 0]
    assert np.array_equal(CC.gather(d.pk, d.host("confidence"), C.POISON64), _answer(lines, frames)[0])


def test_behind_the_aligner_on_one_stream(lib):
    """ta_forced_align_lines, then this call on what it left on the device -- its status and its frames, no look at either
    from the host in between: the typical lines, one of them over its cap (the aligner refuses it, this call skips it)"""
    import forced_lines_cases as LC
    name, no, lines = [c for c in CC.cases() if c[0] == "typical"][0]
    apk = LC.pack(lib, lines, no, cap_edit={2: 50})
    a = {n: torch.from_numpy(getattr(apk, n)).cuda() for n in LC.INPUTS + LC.OUTPUTS + ("ws",)}
    stream = torch.cuda.current_stream().cuda_stream
    assert LC.call(lib, apk, lambda n: a[n].data_ptr(), stream) == 0
    pk = C.pack(lib, lines, no, frames=np.full((sum(len(cs) for _, cs in lines), 3), C.POISON32, np.int32), cap_edit={2: 50})
    d = _Device(pk, C)
    assert d.call(lib, align_status=a["status"].data_ptr(), frames=a["frames"].data_ptr()) == 0
    assert a["status"].cpu().numpy()[:4].tolist() == [R0.OK, R0.OK, R0.BOUNDS, R0.OK]
    assert d.host("status")[:4].tolist() == [R0.OK, R0.OK, C.SKIPPED, R0.OK]
    _, conf, rival = CC.want(name, lines)["peak"]
    off = np.cumsum([0] + [len(cs) for _, cs in lines])
    keep = np.r_[off[0]:off[2], off[3]:off[4]]
    got = CC.gather(pk, d.host("confidence"), C.POISON64)
    assert np.array_equal(got[keep], conf[keep]) and (got[off[2]:off[3]] == C.POISON64).all()
    assert np.array_equal(CC.gather(pk, d.host("rival"), C.POISON32)[keep], rival[keep])


# ---- ta_confidence_pages ----------------------------------------------------------------------------------------------------

def _back(d):
    for name in PC.OUTPUTS:
        setattr(d.pk, name, d.host(name))


@pytest.mark.parametrize("case", PC.cases(), ids=lambda c: c[0])
def test_confidence_pages_equals_the_checker(lib, case):
    name, pages = case
    d = _Device(PC.pack(pages, seed=len(name)), PC)
    assert d.call(lib) == 0
    _back(d)
    PC.compare(d.pk)


def test_confidence_pages_refusals_on_the_device_and_on_the_host(lib):
    name, pages = [c for c in PC.cases() if c[0] == "three pages"][0]
    for count in (-1, 1):
        d = _Device(PC.pack(pages, seed=3, count=count), PC)
        assert d.call(lib) == 0
        _back(d)
        PC.compare(d.pk)
    for field, at, v, hit in (("t_off", 3, 1 << 40, (2, 3)), ("line_first", 2, -2, (1, 2)), ("syl_off", 4, -7, (3,))):
        pk = PC.pack(pages, seed=1)
        answer, was = PC.want(pk), getattr(pk, field)[at]
        getattr(pk, field)[at] = v
        d = _Device(pk, PC)
        assert d.call(lib) == 0
        _back(d)
        getattr(pk, field)[at] = was
        assert [int(pk.status[p]) for p in hit] == [PR.BOUNDS] * len(hit), (field, at)
        PC.compare(pk, answer, skip=hit)
    d = _Device(PC.pack(pages), PC)
    for over in (dict(confidence=None), dict(status=None), dict(nsyl=-1), dict(nprob=-1)):
        assert d.call(lib, **over) == -1
    assert d.call(lib, nlines=(1 << 24) + 1) == -4 and d.call(lib, nprob=0) == 0
    torch.cuda.synchronize()
    assert (d.host("char_conf") == PC.POISON64).all() and (d.host("status") == PC.POISON32).all()
    assert d.call(lib) == 0
    _back(d)
    PC.compare(d.pk)
