"""ta_forced_posterior_lines on the GPU: the case table and the refusals of tests/test_forced_post_lines_sim.py through
the library with real device pointers -- every output and the workspace poisoned -- against the checker
tests/forced_post_ref.py, word for word (the float64 outputs through their int64 view)."""
import numpy as np
import pytest

import forced_cases as C0
import forced_conf_cases as CC
import forced_post_cases as PC
import forced_post_lines_cases as C
import forced_post_ref as R
import forced_ref as R0

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class _Device(object):
    """a packed case's arrays on the device"""

    def __init__(self, pk):
        self.pk = pk
        self.t = {name: torch.from_numpy(getattr(pk, name)).cuda() for name in C.INPUTS + C.OUTPUTS + ("ws",)}

    def ptr(self, name):
        return self.t[name].data_ptr()

    def call(self, lib, **over):
        return C.call(lib, self.pk, self.ptr, torch.cuda.current_stream().cuda_stream, **over)

    def host(self, name):
        return self.t[name].cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    from text_alignment_amd import _native
    return _native.lib


@pytest.mark.parametrize("case", CC.cases(), ids=lambda c: c[0])
def test_the_indexed_entry_equals_the_checker_at_the_aligners_peaks(lib, case):
    name, no, lines = case
    d = _Device(C.pack(lib, lines, no, frames=C0.want(name, lines)[0], seed=len(name)))
    assert d.call(lib) == 0
    C.check_case(d.pk, name, lines, d.host)


def _three(rng):
    return [(C0.probs(rng, 30, 6), C0.text(rng, 7, 6)), (C0.probs(rng, 21, 6), C0.text(rng, 5, 6)),
            (C0.probs(rng, 140, 6), C0.text(rng, 66, 6))]


def test_a_slot_the_aligner_refused_is_skipped_and_one_refused_here_leaves_its_neighbours_alone(lib):
    rng = np.random.default_rng(21)
    lines = _three(rng)
    frames = R0.align_batch(lines)[0]
    wanted = C.answer(lines, frames)
    poisoned = frames.copy()
    poisoned[7:12] = C.POISON32
    packs = [(C.pack(lib, lines, 6, frames=poisoned, align_status={1: st}, labels_edit={1: (2, 999)}), C.SKIPPED)
             for st in (R0.BOUNDS, R0.LABEL, 3, R.QUERY, C.SKIPPED, -1, C.POISON32)]
    packs += [(C.pack(lib, lines, 6, frames=frames, cap_edit={1: 4}), R0.BOUNDS),
              (C.pack(lib, lines, 6, frames=frames, cap_edit={1: 8}, L_dev={1: 9}), R0.BOUNDS),
              (C.pack(lib, lines, 6, frames=frames, L_dev={1: 0}), R0.BOUNDS),
              (C.pack(lib, lines, 6, frames=frames, labels_edit={1: (2, 6)}), R0.LABEL),
              (C.pack(lib, lines, 6, frames=frames, labels_edit={1: (0, 0)}), R0.LABEL)]
    for i, v in ((3, int(frames[7 + 2, 2]) - 1), (4, 21), (0, -1)):       # a decreasing peak, peaks outside the line
        edited = frames.copy()
        edited[7 + i, 2] = v
        packs.append((C.pack(lib, lines, 6, frames=edited), R.QUERY))
    for name, v in (("acc_line", -1), ("acc_line", 6), ("acc_line", 1 << 30), ("lab_off", -1), ("lab_off", 10 ** 9),
                    ("lab_off", 1 << 62), ("row_off_all", -3), ("row_off_all", 10 ** 9)):
        pk = C.pack(lib, lines, 6, frames=frames)
        at = int(pk.slot_line[1]) if name == "row_off_all" else 1
        pk.edit = (name, at, getattr(pk, name)[at])
        getattr(pk, name)[at] = v
        packs.append((pk, R0.BOUNDS))
    for pk, status in packs:
        d = _Device(pk)
        assert d.call(lib) == 0
        if hasattr(pk, "edit"):                          # gather looks the lines' rows up where they were
            getattr(pk, pk.edit[0])[pk.edit[1]] = pk.edit[2]
        st = d.host("status")
        assert st[:3].tolist() == [R0.OK, status, R0.OK] and (st[3:] == C.POISON32).all()
        C.check_slots(pk, d.host, wanted, (0, 2), 3)
        assert (C.outside_pieces(pk, d.host("ws"), (0, 2)) == C.POISON_BYTE).all()


def test_count_limits_the_slots_and_a_negative_count_touches_nothing(lib):
    rng = np.random.default_rng(22)
    lines = _three(rng)
    frames = R0.align_batch(lines)[0]
    wanted = C.answer(lines, frames)
    d = _Device(C.pack(lib, lines, 6, frames=frames, count=2))
    assert d.call(lib) == 0
    st = d.host("status")
    assert st[:2].tolist() == [R0.OK, R0.OK] and (st[2:] == C.POISON32).all()
    C.check_slots(d.pk, d.host, wanted, (0, 1), 3)
    assert (C.outside_pieces(d.pk, d.host("ws"), (0, 1)) == C.POISON_BYTE).all()
    for count in (0, -1, -(1 << 40)):
        d = _Device(C.pack(lib, lines, 6, frames=frames, count=count))
        assert d.call(lib) == 0
        assert C.untouched(d.pk, d.host), count
    pk = C.pack(lib, lines, 6, frames=frames, count=1 << 40)   # more than the slots the call covers: the covered ones run
    pk.acc_line[3:], pk.L[3:], pk.lab_off[3:], pk.align_status[3:] = -1, 1, 0, 0
    d = _Device(pk)
    assert d.call(lib) == 0 and d.host("status").tolist() == [R0.OK] * 3 + [R0.BOUNDS] * 2


def test_host_side_refusals_touch_nothing_and_the_good_call_then_runs(lib):
    rng = np.random.default_rng(23)
    lines = _three(rng)[:2]
    frames = R0.align_batch(lines)[0]
    d = _Device(C.pack(lib, lines, 6, frames=frames))
    for what, code, over in C.refusals(d.pk):
        if over == "misalign":
            over = dict(workspace=d.ptr("ws") + 4)
        assert d.call(lib, **over) == code, what
    assert d.call(lib, nslots=0) == 0
    assert d.call(lib, Lcap_host=np.zeros(d.pk.nlines_all, np.int32)) == 0
    torch.cuda.synchronize()
    assert C.untouched(d.pk, d.host)
    assert d.call(lib) == 0
    assert d.host("status")[:2].tolist() == [0, 0]
    C.check_slots(d.pk, d.host, C.answer(lines, frames), (0, 1), 2)


def test_workspace_bytes(lib):
    f = lib.ta_forced_posterior_lines_workspace_bytes
    assert f(1000, 1) == 1536 * 1000 and f(1000, 64) == 3072 * 1000 and f(7, 128) == 6144 * 7 and f(7, 256) == 12288 * 7
    assert f(7, 512) == 24576 * 7 and f(7, 1023) == 24576 * 7 and f(0, 5) == 0 and f(123, 0) == 0
    for cap, lmax in ((-1, 5), (5, -1), (5, 1024), (1 << 62, 1)):
        assert f(cap, lmax) == -1
    for L in (1, 63, 64, 300, 1023):
        assert f(L, L) == lib.ta_forced_posterior_workspace_bytes(2 * L + 1, L)


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
    d = _Device(pk)
    assert d.call(lib, align_status=a["status"].data_ptr(), frames=a["frames"].data_ptr()) == 0
    assert a["status"].cpu().numpy()[:4].tolist() == [R0.OK, R0.OK, R0.BOUNDS, R0.OK]
    assert d.host("status")[:4].tolist() == [R0.OK, R0.OK, C.SKIPPED, R0.OK]
    C.check_slots(pk, d.host, PC.want(name, lines)["peak"][1], (0, 1, 3), 4)
