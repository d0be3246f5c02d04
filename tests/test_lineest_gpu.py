"""Device line normaliser (csrc/ta_lineest.hip) against the checker oracle/lineest_ref.py (scipy.ndimage
in float64; ocropy itself is absent, so the checker is a parity-unpinned
restatement): identical per-column arg-max, centre line and band height, resampled input rows equal to float32
rounding -- on the word-like strips this file began with and on the strips of tests/lineest_cases.py, which pick the
kernels' branches and the content that strains them (tests/test_lineest_sim.py runs the same list through a host build
of the kernels)."""
import numpy as np
import pytest

import lineest_cases as C

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_strip = C.strip


def test_device_normaliser_matches_host():
    assert torch.cuda.is_available()
    from oracle import lineest_ref as lineest
    from text_alignment_amd import lineest_gpu
    strips = C.word_strips()
    x, T, dbg = lineest_gpu.normalize_strips(strips, want_debug=True)
    x = x.cpu().numpy()
    row = 0
    for k, s in enumerate(strips):
        norm = lineest.CenterNormalizer()
        want = lineest.prepare_raw_strip(s, norm)
        assert np.array_equal(dbg["center"][k], norm.center), k
        assert int(dbg["r"][k]) == norm.r, k
        assert T[k] == want.shape[0], (k, T[k], want.shape)
        got = x[row:row + T[k]]
        row += int(T[k])
        assert got.shape == want.shape
        assert float(np.abs(got - want.astype(np.float32)).max()) <= 2e-6, k
    assert row == x.shape[0]


def _per_strip(x, T, dbg):
    """[(arg, center, r, wout, rows)] of one normalize_strips(..., want_debug=True) call"""
    x = x.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(T)])
    assert off[-1] == x.shape[0]
    return [(dbg["arg"][k], dbg["center"][k], int(dbg["r"][k]), int(T[k]) - 2 * C.PAD, x[off[k]:off[k + 1]])
            for k in range(len(T))]


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:4] == b[2:4] and
            a[4].tobytes() == b[4].tobytes())


@pytest.fixture(scope="module")
def batch():
    """every accepted strip in ONE call: mixed heights, repeated heights sharing one set of weights, odd pixel offsets"""
    from text_alignment_amd import lineest_gpu
    cases = C.accepted()
    got = _per_strip(*lineest_gpu.normalize_strips([s for _, s in cases], want_debug=True))
    return dict(zip([name for name, _ in cases], got))


@pytest.mark.parametrize("name", [name for name, _ in C.accepted()])
def test_every_kernel_path_matches_the_checker(batch, name):
    """arg, center, r and the output width equal to the checker's, the rows within 2e-6"""
    C.check_strip(name, *batch[name])


def test_a_strip_does_not_depend_on_its_place_in_the_batch(batch):
    """the same list reversed, and every single-column and single-row strip in a batch of its own: bit for bit"""
    from text_alignment_amd import lineest_gpu
    cases = C.accepted()[::-1]
    got = _per_strip(*lineest_gpu.normalize_strips([s for _, s in cases], want_debug=True))
    for (name, _), g in zip(cases, got):
        assert _same(g, batch[name]), name
    alone = [name for name, s in cases if min(s.shape) == 1]
    assert sorted(alone) == ["one pixel 40x1", "one pixel 8x1", "scatter 1x50"]
    for name in alone:
        (g,) = _per_strip(*lineest_gpu.normalize_strips([C.by_name(name)], want_debug=True))
        assert _same(g, batch[name]), name


def _longest_first(Tl):
    """LineRecognizer.prepare's layout: first row of every line, the lines sorted by length, longest first"""
    order = np.argsort(-Tl, kind="stable")
    start = np.empty(len(Tl), dtype=np.int64)
    start[order] = np.cumsum(Tl[order]) - Tl[order]
    return start


def _last_first(Tl):
    return (np.cumsum(Tl[::-1]) - Tl[::-1])[::-1]


def test_resampling_a_run_of_a_measured_batch_and_in_a_layout_of_the_callers(batch):
    from text_alignment_amd import lineest_gpu
    names = ["scatter 30x2305", "one pixel 8x1", "scatter 161x642", "scatter 1x50", "word strip 3 (33x300)",
             "bands at both edges", "scatter 98x70", "values 100..180"]
    strips = [C.by_name(name) for name in names]
    n = len(strips)
    ms = lineest_gpu.measure_strips(strips)
    x, T = lineest_gpu.resample_strips(ms, 0, n)
    x = x.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(T)])
    assert off[-1] == x.shape[0]
    for k, name in enumerate(names):
        assert x[off[k]:off[k + 1]].tobytes() == batch[name][4].tobytes(), name
    for a, b in ((3, 6), (n - 1, n), (0, 1)):                # strips from `a` on: the per-strip arrays start there
        xs, Ts = lineest_gpu.resample_strips(ms, a, b)
        assert np.array_equal(Ts, T[a:b])
        assert xs.cpu().numpy().tobytes() == x[off[a]:off[b]].tobytes(), (a, b)
    for a, b, layout in ((0, n, _longest_first), (0, n, _last_first), (2, 7, _longest_first), (2, 7, _last_first)):
        xl, Tl = lineest_gpu.resample_strips(ms, a, b, layout=layout)
        assert np.array_equal(Tl, T[a:b]) and xl.shape[0] == int(Tl.sum())
        xl = xl.cpu().numpy()
        start = layout(Tl)
        covered = np.zeros(xl.shape[0], dtype=np.int64)
        for k in range(b - a):
            covered[start[k]:start[k] + Tl[k]] += 1
            assert xl[start[k]:start[k] + Tl[k]].tobytes() == x[off[a + k]:off[a + k + 1]].tobytes(), (a, b, k)
        assert (covered == 1).all()
    # the measuring pass in two halves, with host work in between
    half = lineest_gpu.measure_strips_begin(strips)
    assert half.wo is None and half.T is None
    want = [C.want(name).wout for name in names]
    assert lineest_gpu.measure_strips_end(half) is half and half.wo.tolist() == want == ms.wo.tolist()
    assert np.array_equal(half.T, ms.T)
    for field in ("arg", "center", "r", "wout", "minmax"):
        assert torch.equal(getattr(half, field), getattr(ms, field)), field
    xh, _ = lineest_gpu.resample_strips(half)
    assert xh.cpu().numpy().tobytes() == x.tobytes()


def test_device_normaliser_rejects_what_the_checker_rejects(batch):
    from oracle import lineest_ref as lineest
    from text_alignment_amd import lineest_gpu, ocr
    with pytest.raises(ValueError):
        lineest_gpu.normalize_strips([np.full((30, 100), 255, np.uint8)])
    with pytest.raises(TypeError):
        lineest_gpu.normalize_strips([np.zeros((30, 100), np.float32)])
    x, T, _ = lineest_gpu.normalize_strips([])
    assert x.shape == (0, 48) and len(T) == 0
    # a strip whose output width int(48 / (2 r) * w) is 0: the checker fails on the empty line, the device path refuses
    # it in words that tell it from a constant strip
    good = ["scatter 17x63", "bilevel", "scatter 30x1281"]
    rec = ocr.LineRecognizer(ocr.LineModel.random(11, no=40))
    for name, s in C.refused():
        with pytest.raises(ValueError):
            lineest.prepare_raw_strip(s)
        on_dev = torch.from_numpy(s).cuda()
        for bad in (s, on_dev):
            for strips in ([bad], [C.by_name(good[0]), bad, C.by_name(good[1]), C.by_name(good[2])]):
                with pytest.raises(ValueError, match="width 0") as err:
                    lineest_gpu.normalize_strips(strips)
                assert "constant" not in str(err.value)
                ms = lineest_gpu.measure_strips_begin(strips)
                for _ in range(2):                           # refused, and still refused when asked again
                    with pytest.raises(ValueError, match="width 0"):
                        lineest_gpu.measure_strips_end(ms)
                    assert ms.wo is None and ms.T is None
                with pytest.raises(ValueError, match="width 0"):
                    rec.prepare(strips)
                st = rec.prepare(strips, defer=True)
                with pytest.raises(ValueError, match="width 0"):
                    rec.complete(st)
        # the good strips of such a batch, without the refused one
        got = _per_strip(*lineest_gpu.normalize_strips([C.by_name(g) for g in good], want_debug=True))
        for g, have in zip(good, got):
            C.check_strip(g, *have)
            assert _same(have, batch[g]), g
    with pytest.raises(ValueError, match="empty or constant"):
        lineest_gpu.normalize_strips([C.by_name(good[0]), np.full((60, 1), 7, np.uint8)])


def test_strips_already_on_the_device_are_normalised_where_they_are():
    """The device preprocessing leaves its strips on the GPU (Strip.device_pixels): the normaliser takes
    them there, alone or mixed with host strips, bit for bit as from host arrays; a constant one is
    refused (after the measuring pass, which finds its minimum and maximum anyway); `.pixels` downloads."""
    from text_alignment_amd import lineest_gpu, page as page_mod
    rng = np.random.default_rng(21)
    strips = [_strip(rng, h, w) for h, w in [(44, 600), (50, 420), (61, 800), (38, 256)]]
    on_dev = [torch.from_numpy(s).cuda() for s in strips]
    x0, T0, _ = lineest_gpu.normalize_strips(strips)
    for mix in (on_dev, [on_dev[0], strips[1], on_dev[2], strips[3]]):
        x1, T1, _ = lineest_gpu.normalize_strips(mix)
        assert np.array_equal(T0, T1) and torch.equal(x0, x1)
    with pytest.raises(ValueError, match="empty or constant"):
        lineest_gpu.normalize_strips([on_dev[0], torch.full((30, 100), 255, dtype=torch.uint8, device="cuda")])
    with pytest.raises(TypeError):
        lineest_gpu.normalize_strips([on_dev[0].t()])                       # not contiguous
    st = page_mod.Strip(3, 4, 44, device_pixels=on_dev[0])
    assert st.width == 600 and page_mod.prepared_line(st)[0] is on_dev[0]
    assert np.array_equal(st.pixels, strips[0])
    # DeviceStrips: pieces of packed buffers, as the page preprocessing leaves them -- neighbours in one buffer (taken
    # as ONE slice), a gap between two, a second buffer, a tensor and a host strip in between
    sizes = [s.size for s in strips]
    buf_a = torch.cat([on_dev[0].reshape(-1), on_dev[1].reshape(-1), torch.zeros(100, dtype=torch.uint8, device="cuda"),
                       on_dev[2].reshape(-1)])
    buf_b = torch.cat([torch.zeros(7, dtype=torch.uint8, device="cuda"), on_dev[3].reshape(-1)])
    ds = [page_mod.DeviceStrip(buf_a, 0, 44, 600), page_mod.DeviceStrip(buf_a, sizes[0], 50, 420),
          page_mod.DeviceStrip(buf_a, sizes[0] + sizes[1] + 100, 61, 800), page_mod.DeviceStrip(buf_b, 7, 38, 256)]
    for mix in (ds, [ds[0], ds[1]] + [on_dev[2], strips[3]], [strips[0], ds[1], ds[2], ds[3]]):
        x1, T1, _ = lineest_gpu.normalize_strips(mix)
        assert np.array_equal(T0, T1) and torch.equal(x0, x1)
    x1, T1, _ = lineest_gpu.normalize_strips(ds[:2])                        # one slice, no copy
    xa, Ta, _ = lineest_gpu.normalize_strips(strips[:2])
    assert np.array_equal(Ta, T1) and torch.equal(xa, x1)
    st = page_mod.Strip(3, 4, 50, device_pixels=ds[1])
    assert st.width == 420 and page_mod.prepared_line(st)[0] is ds[1] and np.array_equal(st.pixels, strips[1])
    with pytest.raises(ValueError, match="outside its buffer"):
        lineest_gpu.normalize_strips([page_mod.DeviceStrip(buf_b, 8, 38, 256)])
    with pytest.raises(TypeError):
        lineest_gpu.normalize_strips([page_mod.DeviceStrip(buf_a.view(2, -1), 0, 44, 600)])


def test_recogniser_takes_raw_strips():
    """LineRecognizer.prepare: raw uint8 strips (device normaliser) mixed with host-prepared lines
    give the rows the checker's normaliser gives, and the same decoded characters."""
    from oracle import lineest_ref as lineest
    from text_alignment_amd import ocr
    rng = np.random.default_rng(9)
    strips = [_strip(rng, h, w) for h, w in [(44, 600), (50, 420), (61, 800), (38, 256), (44, 333)]]
    host = [lineest.prepare_raw_strip(s).astype(np.float32) for s in strips]
    model = ocr.LineModel.random(11, no=40)
    for wts in (model.fwd, model.rev):                         # contractive recurrence: see test_ocr_gpu._tame
        for name in ("WGI", "WGF", "WGO", "WCI"):
            wts[name][:, 49:] *= 0.25
        for name in ("WIP", "WFP", "WOP"):
            wts[name] *= 0.25
    rec = ocr.LineRecognizer(model)
    mixed = [strips[0], host[1], strips[2], strips[3], host[4]]
    st_m, st_h = rec.prepare(mixed), rec.prepare(host)
    assert np.array_equal(st_m["T_host"], st_h["T_host"])
    assert float((st_m["x"] - st_h["x"]).abs().max()) <= 2e-6
    assert rec.recognise(mixed) == rec.recognise(host)
    assert list(rec.last_T) == [h.shape[0] for h in host]
