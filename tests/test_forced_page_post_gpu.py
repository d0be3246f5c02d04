"""The page-scope posterior kernel (csrc/ta_forced_page_post.hip) on the GPU against the checker
tests/forced_page_post_ref.py: the cases of tests/forced_page_cases.py with the queries of
tests/forced_page_post_cases.py through the library with real device pointers -- the aligner and the posterior back to
back on one stream, the aligner's frames handed over where they lie --, the refusals, and the device-level Python call.
Every output word is compared bit for bit; everything is poisoned first."""
import numpy as np
import pytest

import forced_page_cases as PC
import forced_page_post_cases as C
import forced_page_post_ref as R
import forced_page_ref as PR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NAMES = tuple(dict.fromkeys(PC.INPUTS + PC.OUTPUTS + ("ws",) + C.INPUTS + C.OUTPUTS + ("pws",)))


class _Device(object):
    """a packed case's arrays on the device; back() copies the outputs into the packed case"""

    def __init__(self, pk):
        self.pk = pk
        self.t = {name: torch.from_numpy(getattr(pk, name)).cuda() for name in NAMES}

    def ptr(self, name):
        return self.t[name].data_ptr()

    def align(self, lib):
        return PC.call(lib, self.pk, self.ptr, torch.cuda.current_stream().cuda_stream)

    def call(self, lib, **over):
        return C.call(lib, self.pk, self.ptr, torch.cuda.current_stream().cuda_stream, **over)

    def back(self):
        for name in PC.OUTPUTS + C.OUTPUTS + ("ws", "pws"):
            getattr(self.pk, name)[...] = self.t[name].cpu().numpy()
        return self.pk


@pytest.fixture(scope="module")
def lib():
    from text_alignment_amd import _native
    return _native.lib


def _queries(want):
    return [(w["line"], w["frame"]) for w in want]


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_kernel_equals_the_checker(lib, case):
    """the seeded queries from the host, then the aligner and the posterior back to back on one stream with the frames
    handed over on the device: a page the aligner found no path for left its frames alone, so its queries are refused"""
    name, no, pages = case
    want = C.want(name, pages)
    d = _Device(C.pack(lib, pages, no, _queries(want["seeded"]), aligner=lib))
    assert d.call(lib) == 0
    C.check(d.back(), want["seeded"])
    d = _Device(C.pack(lib, pages, no, _queries(want["peak"]), aligner=lib))
    assert d.align(lib) == 0 and d.call(lib, query=d.ptr("frames")) == 0
    pk = d.back()
    PC.check(pk, PC.want(name, pages))
    C.check(pk, [w if w["status"] == PR.OK else C.refused(R.QUERY) for w in want["peak"]])


def _three(rng):
    return [PC._page(rng, (12, 11), 8, (0, 3), (4, 8), 6), PC._page(rng, (10, 9, 11), 9, (0, 1, 6), (5, 6, 9), 6),
            PC._wide(rng, 70)]


def _wants(rng, pages):
    return [C.answer(pg, *C.seeded_queries(rng, [len(P) for P in pg[0]], len(pg[1]), pg[2], pg[3])) for pg in pages]


def test_a_page_refused_or_without_a_path_leaves_its_neighbours_alone(lib):
    rng = np.random.default_rng(7)
    pages = _three(rng)
    want = _wants(rng, pages)
    ql, qt = np.asarray([0, 0, 0, 0, 0, 1, 2, 2, 2], np.int32), np.asarray([0, 2, 2, 5, 9, 4, 0, 3, 10], np.int32)
    want[1] = C.answer(pages[1], ql, qt)
    queries = _queries(want)
    a = int(C.pack(lib, pages, 6, queries).lab_off[1])
    edits = [(PR.LABEL, "labels", a + 2, 6), (PR.LABEL, "labels", a + 8, 0), (PR.BOUNDS, "lo", 2, 1), (PR.BOUNDS, "hi", 4, 8),
             (PR.BOUNDS, "lo", 3, 6), (PR.BOUNDS, "lo", 4, 0), (PR.BOUNDS, "hi", 3, 4), (PR.BOUNDS, "hi", 3, 1030),
             (PR.BOUNDS, "T", 3, 0), (PR.BOUNDS, "T", 3, 5001), (PR.BOUNDS, "row_off", 4, 10 ** 9), (PR.BOUNDS, "row_off", 2, -3),
             (PR.BOUNDS, "pws_off", 1, 8), (PR.BOUNDS, "pws_off", 1, 10 ** 12), (PR.BOUNDS, "pws_off", 1, -16)]
    for i, k, t in ((0, -1, 0), (8, 3, 0), (3, 0, -1), (4, 0, 10), (8, 2, 11), (0, 2, 0), (8, 1, 8), (5, 0, 9), (2, 0, 6), (3, 1, 0)):
        edits.append((R.QUERY, "query", a + i, [k, -7, -7, t]))
    for status, name, k, v in edits:
        pk = C.pack(lib, pages, 6, queries)
        host = {h: getattr(pk, h[:-5]).copy() for h in C.HOST}                # the host's copies stay right
        getattr(pk, name)[k] = v
        d = _Device(pk)
        assert d.call(lib, **host) == 0
        w = list(want)
        w[1] = C.refused(status)
        C.check(d.back(), w)
    # a page without a path between two good ones: five characters on three frames
    nopath = PC._page(rng, (2, 1), 5, (0, 2), (4, 5), 6)
    w = [want[0], C.answer(nopath, *C.seeded_queries(rng, [2, 1], 5, nopath[2], nopath[3])), want[2]]
    assert w[1]["status"] == PR.NOPATH
    d = _Device(C.pack(lib, [pages[0], nopath, pages[2]], 6, _queries(w)))
    assert d.call(lib) == 0
    C.check(d.back(), w)
    # the device's windows ask for a variant that the host's copies did not launch
    wide = PC._page(np.random.default_rng(8), (150, 12), 73, (0, 68), (70, 73), 6)
    w2 = _wants(rng, [pages[0], wide])
    pk = C.pack(lib, [pages[0], wide], 6, _queries(w2))
    narrow, early = pk.hi.copy(), pk.lo.copy()
    narrow[2], early[3] = 60, 58
    d = _Device(pk)
    assert d.call(lib, hi_host=narrow, lo_host=early) == 0
    C.check(d.back(), [w2[0], C.refused(PR.BOUNDS)])


def test_host_side_refusals_touch_nothing_and_the_good_call_then_runs(lib):
    from text_alignment_amd import _native
    rng = np.random.default_rng(9)
    pages = _three(rng)[:2]
    want = _wants(rng, pages)
    pk = C.pack(lib, pages, 6, _queries(want))
    d = _Device(pk)
    EINVAL, ELIMIT = -1, -4

    def arr(name, k, v):
        a = getattr(pk, name).copy()
        a[k] = v
        return a
    wide_hi, wide_lab = pk.hi.copy(), pk.lab_off.copy()
    wide_hi[:2] = 1024
    wide_lab[1:] += 1016
    nl = 3356                                             # more than 2^24 frames on one page
    big = dict(nlines=nl, npages=1, rows=1 << 40, T_host=np.full(nl, 5000, np.int32), lo_host=np.zeros(nl, np.int32),
               hi_host=np.full(nl, 8, np.int32), line_first_host=np.asarray([0, nl], np.int64),
               lab_off_host=np.asarray([int(pk.lab_off[0]), int(pk.lab_off[0]) + 8], np.int64))
    for what, code, over in (
            ("null probs", EINVAL, dict(probs=None)), ("null query", EINVAL, dict(query=None)),
            ("null status", EINVAL, dict(pstatus=None)), ("null z_m", EINVAL, dict(z_m=None)),
            ("negative nlabels", EINVAL, dict(nlabels=-1)),
            ("no = 129", EINVAL, dict(no=129)), ("workspace too small", EINVAL, dict(workspace_bytes=sum(pk.piece) - 1)),
            ("workspace misaligned", EINVAL, dict(workspace=d.ptr("pws") + 4)),
            ("non-monotone window", EINVAL, dict(lo_host=arr("lo", 4, 0))),
            ("lo_0 != 0", EINVAL, dict(lo_host=arr("lo", 0, 1))), ("hi_last != n", EINVAL, dict(hi_host=arr("hi", 1, 7))),
            ("width 1024", ELIMIT, dict(hi_host=wide_hi, lab_off_host=wide_lab, nlabels=10 ** 6)),
            ("T > 5000", ELIMIT, dict(T_host=arr("T", 1, 5001))), ("2^24 frames", ELIMIT, big)):
        assert d.call(lib, **over) == code, what
    with pytest.raises(_native.NativeArgumentError):
        _native.check(d.call(lib, no=1), "ta_forced_page_posterior")
    assert d.call(lib, npages=0) == 0
    torch.cuda.synchronize()
    assert C.untouched(d.back())
    assert d.call(lib) == 0
    C.check(d.back(), want)
    f = lib.ta_forced_page_posterior_workspace_bytes
    assert f(9, 2) == 13824 and f(1027, 32) == 24576 * 1027 and f(0, 2) == -1 and f(5, 3) == -1 and f((1 << 29) + 1, 2) == -1


def test_forced_page_posterior_python_call():
    """the device-level Python call: its own workspace layout, poisoned; pages of different variants; queries from the host
    and as the device tensor forced_page_alignment returned; the refusals"""
    from text_alignment_amd import forced
    rng = np.random.default_rng(10)
    pages = [PC._page(rng, (40, 33, 21), 30, (0, 8, 19), (14, 24, 30), 30), PC._wide(rng, 66, no=30),
             PC._page(rng, (2, 1), 5, (0, 2), (4, 5), 30)]
    aligned = [PR.align_page(*pg)[:3] for pg in pages]
    assert [w[0] for w in aligned] == [PR.OK, PR.OK, PR.NOPATH]
    Ps = [P for pg in pages for P in pg[0]]
    T = [len(P) for P in Ps]
    probs = torch.from_numpy(np.concatenate(Ps)).cuda()
    row_off = np.cumsum([0] + T[:-1])
    line_first = np.cumsum([0] + [len(pg[0]) for pg in pages])
    lab_off = np.cumsum([0] + [len(pg[1]) for pg in pages])
    lo, hi = np.concatenate([pg[2] for pg in pages]), np.concatenate([pg[3] for pg in pages])
    labels = np.concatenate([pg[1] for pg in pages])
    frames, _, st = forced.forced_page_alignment(probs, row_off, T, line_first, lo, hi, labels, lab_off)
    got = forced.forced_page_posterior(probs, row_off, T, line_first, lo, hi, labels, lab_off, frames)
    assert st.cpu().tolist() == [0, 0, forced.NOPATH]
    want = [R.query(*pg, w[2][:, 0], w[2][:, 3]) for pg, w in zip(pages[:2], aligned)]

    def same(got_, p):
        for name in R.PER_LABEL:
            assert C._same(np.asarray(got_[name])[lab_off[p]:lab_off[p + 1]], want[p][name]), (p, name)
        for name in R.PER_PAGE:
            assert C._same(np.asarray(got_[name])[p:p + 1], [want[p][name]]), (p, name)

    dev = {name: t.cpu().numpy() for name, t in got.items()}
    assert dev["own_m"].dtype == np.float64 and dev["own_x"].dtype == np.int32 and dev["rival_state"].dtype == np.int32
    for p in range(2):
        same(dev, p)
    assert dev["status"].tolist()[:2] == [0, 0]           # (page 2's frames are whatever the allocation held)
    query = np.full((len(labels), 4), -7, np.int32)
    for p in range(2):
        query[lab_off[p]:lab_off[p + 1]] = aligned[p][2]
    ql, qt = C.seeded_queries(rng, [2, 1], 5, pages[2][2], pages[2][3])
    query[lab_off[2]:, 0], query[lab_off[2]:, 3] = ql, qt
    got = forced.forced_page_posterior(probs, row_off, T, line_first, lo, hi, labels, lab_off, query, host=True, _fill=0xEE)
    assert got["status"].tolist() == [0, 0, forced.NOPATH]
    for p in range(2):
        same(got, p)
    for name in R.PER_LABEL:
        assert (got[name][lab_off[2]:].view(np.uint8) == 0xEE).all(), name
    assert (got["z_m"][2:].view(np.uint8) == 0xEE).all() and (got["z_x"][2:].view(np.uint8) == 0xEE).all()
    # the host's formulas: a posterior at the aligner's own peak is positive and at most one, the likelihood negative
    for p in range(2):
        post = forced.posterior_values(got["own_m"][lab_off[p]:lab_off[p + 1]], got["own_x"][lab_off[p]:lab_off[p + 1]],
                                       got["z_m"][p], got["z_x"][p])
        assert (post > 0).all() and (post <= 1 + 8 * sum(T) * 2.0 ** -53).all()
        assert forced.loglik_bits(got["z_m"][p], got["z_x"][p]) < 0
    query[3, 3] = 5000
    assert forced.forced_page_posterior(probs, row_off, T, line_first, lo, hi, labels, lab_off, query,
                                        host=True)["status"].tolist() == [forced.CONF_QUERY, 0, forced.NOPATH]
    bad_lo = lo.copy()
    bad_lo[1] = 15
    for over in (dict(lo=bad_lo), dict(T=[0] + T[1:]), dict(line_first=[0, 3, 3, 7]), dict(query=query[:-1]),
                 dict(query=torch.from_numpy(query).cuda().long())):
        a = dict(T=T, line_first=line_first, lo=lo, query=query)
        a.update(over)
        with pytest.raises(ValueError):
            forced.forced_page_posterior(probs, row_off, a["T"], a["line_first"], a["lo"], hi, labels, lab_off, a["query"])
