"""The chained span search on the GPU (ta_nw_span_chain): every (i0, i1, score) and every total the kernels give equals
the checker tests/span_chain_ref.py -- row counts around one strip and around more strips than waves, column counts
around the 64-step start-up, every scoring system, chains of 1, 2 and 5 pages in one call with an empty page inside,
the repeated passage, a planted noisy book, a floor that binds, the single search on a chain of one page, the same
bytes twice, refusals on the host that touch nothing and a chain refused on the device between two good ones."""
import numpy as np
import pytest

import span_cases as C
import span_chain_ref as CH
import span_ref as R
from test_span_chain import DEFAULT, repeated_passage

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NS = (0, 1, 255, 256, 257, 2049)                         # 2049 rows = 9 strips of 256 for 8 waves: a wave's second strip
MS = (0, 1, 63, 64, 65, 300)
_refs = {}


def _bound(ts, pages, systems):
    return (max(len(t) for t in ts) + max([len(o) for o in pages] + [0]) + 2) * (3 * int(np.abs(systems).max()) + 2)


def _ref(key, t, pages, system, floor):
    key = (key, tuple(system), floor)
    if key not in _refs:
        spans, total, _ = CH.chain_numpy(t, pages, system, floor)
        _refs[key] = (spans, total)
    return _refs[key]


def _run(ts, page_lists, params, floor=None, again=False):
    from text_alignment_amd import textSeqCompare as tsc
    batch = tsc.SpanChainBatch(ts, page_lists, params, floor=floor)
    assert batch.cells < 3e7
    runs = []
    for _ in range(2 if again else 1):
        batch.out.fill_(-77)                              # poison: every word of the result is the kernels'
        batch.total.fill_(-77)
        batch.ws.fill_(0x5a)
        batch.run()
        batch.fetch_begin()
        out, total = batch.results()
        assert out.shape == (sum(len(p) for p in page_lists), 3) and out.dtype == np.int32 and total.dtype == np.int64
        runs.append((out.tobytes(), total.tobytes()))
    if again:
        assert runs[0] == runs[1]
    first = batch.page_first
    return [([tuple(int(v) for v in row) for row in out[first[c]:first[c + 1]]], int(total[c]))
            for c in range(len(ts))], batch


def _chain(rng, n, ms, alphabet=4):
    t = rng.randint(0, alphabet, size=n).astype(np.int32)
    pages, at = [], 0
    for k, m in enumerate(ms):
        o = rng.randint(0, alphabet, size=m).astype(np.int32)
        if 0 < m and at + m < n and k % 3 != 2:            # planted in reading order, a few substitutions
            a = at + int(rng.randint(0, max(1, (n - at - m) // 2)))
            o = t[a:a + m].copy()
            o[rng.randint(0, m, size=m // 8)] = rng.randint(0, alphabet)
            at = a + m
        pages.append(o)
    return t, pages


@pytest.mark.parametrize("n", NS)
def test_rows_and_columns_at_the_edges(n):
    """one call per row count: three chains over transcripts of n rows whose pages take every column count"""
    rng = np.random.RandomState(300 + n)
    chains = [_chain(rng, n, ms) for ms in ((0, 1, 63), (64, 65, 300), (300, 0, 64, 1, 65))]
    system = C.SYSTEMS[NS.index(n) % len(C.SYSTEMS)]
    floor = _bound([c[0] for c in chains], [o for c in chains for o in c[1]], np.array(system))
    got, _ = _run([c[0] for c in chains], [c[1] for c in chains], system)
    assert got == [_ref(("edges", n, k), t, pages, system, floor) for k, (t, pages) in enumerate(chains)]


@pytest.mark.parametrize("sys_k", range(len(C.SYSTEMS)))
def test_every_scoring_system(sys_k):
    rng = np.random.RandomState(40)                       # the same chains for every system: the references are shared
    chains = [_chain(rng, n, ms, alphabet=2 + 23 * (k % 2)) for k, (n, ms) in
              enumerate([(257, (65, 63, 64)), (600, (300, 1, 100)), (2049, (64, 300))])]
    system = C.SYSTEMS[sys_k]
    floor = _bound([c[0] for c in chains], [o for c in chains for o in c[1]], np.array(system))
    got, _ = _run([c[0] for c in chains], [c[1] for c in chains], system)
    assert got == [_ref(("systems", k), t, pages, system, floor) for k, (t, pages) in enumerate(chains)]


def test_chains_of_one_two_and_five_pages_with_a_system_each():
    """the later steps launch fewer workgroups; a page with m = 0 sits in the middle of the longest chain; the chain of
    one page is listed between the others, so the ranking by page count is no identity"""
    rng = np.random.RandomState(41)
    chains = [_chain(rng, 700, (80, 120)), _chain(rng, 300, (90,)), _chain(rng, 1100, (100, 64, 0, 130, 65))]
    systems = [C.SYSTEMS[0], C.SYSTEMS[3], C.SYSTEMS[4]]
    floor = _bound([c[0] for c in chains], [o for c in chains for o in c[1]], np.array(systems))
    got, batch = _run([c[0] for c in chains], [c[1] for c in chains], systems, again=True)
    assert batch.pages.tolist() == [2, 1, 5]
    assert got == [_ref(("125", k), t, pages, s, floor) for k, ((t, pages), s) in enumerate(zip(chains, systems))]
    assert got[2][0][2][0] == got[2][0][2][1]              # the empty page: an empty span, in its place
    for spans, _ in got:
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def test_repeated_passage_goes_to_its_own_copy():
    from text_alignment_amd import textSeqCompare as tsc
    t, pages = repeated_passage()
    t, pages = t.astype(np.int32), [o.astype(np.int32) for o in pages]
    alone = tsc.SpanBatch([t] * 3, pages, DEFAULT)
    alone.run()
    assert [tuple(r[:2]) for r in alone.results().tolist()] == [(70, 130), (130, 190), (30, 70)]
    got, _ = _run([t], [pages], DEFAULT)
    assert [s[:2] for s in got[0][0]] == [(70, 130), (130, 190), (190, 230)]
    assert got[0] == _ref("repeat", t, pages, DEFAULT, _bound([t], pages, np.array(DEFAULT)))
    strings = ["".join(chr(97 + int(v)) for v in x) for x in [t] + pages]
    assert tsc.locate_chain(strings[0], strings[1:], DEFAULT) == got[0]
    assert tsc.locate_chains([(strings[0], strings[1:]), (strings[0], strings[3:])], [8, -12, -6, -2]) == \
        [got[0], ([(30, 70, 320)], 320)]


def test_a_planted_noisy_book():
    tr, _, _ = C.planted(31, 0, 2400, 0, 1.0)
    rng = np.random.RandomState(32)
    cuts = [(40, 400), (430, 800), (800, 1300), (1350, 1700), (1800, 2350)]
    ocr = [C.noisy(rng, tr[a:b], 0.8) for a, b in cuts]
    t, *pages = C.codes(tr, *ocr)
    for system in (DEFAULT, C.SYSTEMS[1]):
        got, _ = _run([t], [pages], system)
        assert got[0] == _ref("book", t, pages, system, _bound([t], pages, np.array(system)))
        for (i0, i1, _), (a, b) in zip(got[0][0], cuts):
            assert abs(i0 - a) <= 12 and abs(i1 - b) <= 12     # and they are where the text was taken from


def test_a_floor_that_binds():
    rng = np.random.RandomState(43)
    t, pages = repeated_passage()
    chains = [(t.astype(np.int32), [o.astype(np.int32) for o in pages]), _chain(rng, 513, (65, 0, 64, 100))]
    got, batch = _run([c[0] for c in chains], [c[1] for c in chains], DEFAULT, floor=5)
    assert batch.floor == 5
    for k, (t, pages) in enumerate(chains):
        spans, total, bound = CH.chain_numpy(t, pages, DEFAULT, 5)
        assert bound and got[k] == (spans, total), k


def test_a_chain_of_one_page_is_the_single_search():
    from text_alignment_amd import textSeqCompare as tsc
    rng = np.random.RandomState(44)
    ts, os_ = [], []
    for n, m in ((0, 5), (1, 1), (255, 64), (257, 0), (2049, 300), (600, 65)):
        t, pages = _chain(rng, n, (m,), alphabet=3)
        ts.append(t); os_.append(pages[0])
    systems = [C.SYSTEMS[k % len(C.SYSTEMS)] for k in range(len(ts))]
    single = tsc.SpanBatch(ts, os_, systems)
    single.run()
    want = [tuple(r) for r in single.results().tolist()]
    got, _ = _run(ts, [[o] for o in os_], systems)
    assert [g[0] for g in got] == [[w] for w in want] and [g[1] for g in got] == [w[2] for w in want]
    assert want == [R.span_numpy(t, o, s) for t, o, s in zip(ts, os_, systems)]


def test_host_refusals_touch_nothing():
    from text_alignment_amd import _native, textSeqCompare as tsc
    rng = np.random.RandomState(45)
    chains = [_chain(rng, 300, (60, 70)), _chain(rng, 200, (50,))]
    batch = tsc.SpanChainBatch([c[0] for c in chains], [c[1] for c in chains], C.SYSTEMS[0])
    batch.out.fill_(-77); batch.total.fill_(-77); batch.ws.fill_(0x5a)
    good = dict(nchains=batch.nchains, npages=batch.npages, pages=batch.pages, stride=0, floor=batch.floor,
                max_n=batch.max_n, max_m=batch.max_m, bound=batch.score_bound, max_param=batch.max_param,
                ws=batch.ws.data_ptr(), ws_bytes=batch.ws_bytes, total=batch.total.data_ptr())

    def call(**change):
        a = dict(good, **change)
        return _native.lib.ta_nw_span_chain(
            batch.t_codes.data_ptr(), batch.t_start.data_ptr(), batch.t_len.data_ptr(), batch.o_codes.data_ptr(),
            batch.o_off.data_ptr(), batch.d_page_first.data_ptr(), a["nchains"], a["npages"], a["pages"].ctypes.data,
            batch.params.data_ptr(), a["stride"], a["floor"], batch.out.data_ptr(), a["total"], a["max_n"], a["max_m"],
            a["bound"], a["max_param"], a["ws"], a["ws_bytes"], torch.cuda.current_stream().cuda_stream)
    einval, erange = _native.TA_EINVAL, _native.TA_ERANGE
    assert call(nchains=-1) == einval and call(stride=5) == einval and call(floor=0) == einval
    assert call(max_m=_native.lib.ta_nw_span_max_m() + 1) == einval and call(max_n=1 << 28) == einval
    assert call(bound=(1 << 23) - batch.floor) == erange and call(max_param=(1 << 19) + 1) == erange
    assert call(bound=(1 << 23) - batch.floor - 1, floor=batch.floor + 1) == erange
    assert call(ws_bytes=batch.ws_bytes - 1) == einval and call(ws=0) == einval and call(total=0) == einval
    assert call(pages=np.array([2, 2], dtype=np.int32)) == einval       # host counts that do not add up to npages
    assert call(pages=np.array([4, -1], dtype=np.int32)) == einval
    torch.cuda.synchronize()
    assert (batch.out.cpu().numpy() == -77).all() and (batch.total.cpu().numpy() == -77).all()
    assert (batch.ws.cpu().numpy() == 0x5a).all()
    assert _native.lib.ta_nw_span_chain_workspace_bytes(-1, 1, 1) < 0
    assert _native.lib.ta_nw_span_chain_workspace_bytes(1, 1, 1 << 28) < 0
    assert call() == _native.TA_OK                         # and the same arguments unchanged are taken
    out, total = batch.results()
    floor = _bound([c[0] for c in chains], [o for c in chains for o in c[1]], np.array(C.SYSTEMS[0]))
    for k, (t, pages) in enumerate(chains):
        spans, tot, _ = CH.chain_numpy(t, pages, C.SYSTEMS[0], floor)
        assert [tuple(r) for r in out[batch.page_first[k]:batch.page_first[k + 1]].tolist()] == spans and total[k] == tot
    for bad in ([lambda x, y: 1, -1, -1, -1, -1], [8.5, -1, -9, -9, -4, -4]):
        with pytest.raises(ValueError):
            tsc.locate_chain("abc", ["ab"], bad)
        with pytest.raises(ValueError):
            tsc.locate_chains([("abc", ["ab"])], [bad])
    with pytest.raises(OverflowError):                     # score_bound fits 2^23, score_bound + floor does not
        tsc.SpanChainBatch([np.zeros(5000, np.int32)], [[np.zeros(2000, np.int32)]], [200, -200, -200, -200, -200, -200])
    tsc.SpanBatch([np.zeros(5000, np.int32)], [np.zeros(2000, np.int32)], [200, -200, -200, -200, -200, -200])
    with pytest.raises(OverflowError):
        tsc.SpanChainBatch([chains[0][0]], [[np.zeros(_native.lib.ta_nw_span_max_m() + 1, np.int32)]], C.SYSTEMS[0])


def test_a_chain_refused_on_the_device_sits_between_two_good_ones():
    from text_alignment_amd import textSeqCompare as tsc
    rng = np.random.RandomState(46)
    chains = [_chain(rng, 300, (60, 70)), _chain(rng, 280, (50, 0, 64)), _chain(rng, 513, (65,))]
    systems = np.array([C.SYSTEMS[0], C.SYSTEMS[1], C.SYSTEMS[3]], dtype=np.int32)
    batch = tsc.SpanChainBatch([c[0] for c in chains], [c[1] for c in chains], systems)
    broken = systems.copy()
    broken[1, 0] = (1 << 21) + 1                          # beyond the carrier, behind the host's back
    batch.params.copy_(torch.from_numpy(broken).to(batch.params.device).reshape(batch.params.shape))
    batch.out.fill_(-77); batch.total.fill_(-77)
    batch.run()
    with pytest.raises(OverflowError):
        batch.results()
    out, total = batch.out.cpu().numpy(), batch.total.cpu().numpy()
    floor = batch.floor
    for k in (0, 2):
        spans, tot, _ = CH.chain_numpy(chains[k][0], chains[k][1], systems[k], floor)
        assert [tuple(r) for r in out[batch.page_first[k]:batch.page_first[k + 1]].tolist()] == spans and total[k] == tot
    assert out[2:5].tolist() == [[-1, -1, np.iinfo(np.int32).min]] * 3 and total[1] == np.iinfo(np.int64).min
