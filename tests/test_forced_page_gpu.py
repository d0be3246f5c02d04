"""The page-scope forced-alignment kernel (csrc/ta_forced_page.hip) on the GPU against the checker
tests/forced_page_ref.py: the cases of tests/forced_page_cases.py through the library with real device pointers, the
device-level Python call, and forced.align_page_lines end to end.  Every output is an integer and is compared for
equality; everything is poisoned first."""
import numpy as np
import pytest

import forced_page_cases as C
import forced_page_ref as R
import forced_ref as FR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class _Device(object):
    """a packed case's arrays on the device; back() copies the outputs into the packed case"""

    def __init__(self, pk):
        self.pk = pk
        self.t = {name: torch.from_numpy(getattr(pk, name)).cuda() for name in C.INPUTS + C.OUTPUTS + ("ws",)}

    def ptr(self, name):
        return self.t[name].data_ptr()

    def call(self, lib, **over):
        return C.call(lib, self.pk, self.ptr, torch.cuda.current_stream().cuda_stream, **over)

    def back(self):
        for name in C.OUTPUTS + ("ws",):
            getattr(self.pk, name)[...] = self.t[name].cpu().numpy()
        return self.pk


@pytest.fixture(scope="module")
def lib():
    from text_alignment_amd import _native
    return _native.lib


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_kernel_equals_the_checker(lib, case):
    name, no, pages = case
    d = _Device(C.pack(lib, pages, no))
    assert d.call(lib) == 0
    C.check(d.back(), C.want(name, pages))


def test_a_page_refused_through_its_data_leaves_its_neighbours_alone(lib):
    rng = np.random.default_rng(7)
    pages = [C._page(rng, (12, 11), 8, (0, 3), (4, 8), 6), C._page(rng, (10, 9, 11), 9, (0, 1, 6), (5, 6, 9), 6),
             C._wide(rng, 70)]
    want = [R.align_page(*pg)[:3] for pg in pages]
    a = int(C.pack(lib, pages, 6).lab_off[1])
    edits = [(R.LABEL, "labels", a + 2, 6), (R.LABEL, "labels", a + 8, 0), (R.BOUNDS, "lo", 2, 1), (R.BOUNDS, "hi", 4, 8),
             (R.BOUNDS, "lo", 3, 6), (R.BOUNDS, "lo", 4, 0), (R.BOUNDS, "hi", 3, 4), (R.BOUNDS, "hi", 3, 1030),
             (R.BOUNDS, "T", 3, 0), (R.BOUNDS, "T", 3, 5001), (R.BOUNDS, "row_off", 4, 10 ** 9), (R.BOUNDS, "row_off", 2, -3),
             (R.BOUNDS, "ws_off", 2, 8), (R.BOUNDS, "ws_off", 3, 10 ** 12), (R.BOUNDS, "ws_off", 4, -16)]
    for status, name, k, v in edits:
        pk = C.pack(lib, pages, 6)
        host = {h: getattr(pk, h[:-5]).copy() for h in C.HOST}                # the host's copies stay right
        getattr(pk, name)[k] = v
        d = _Device(pk)
        assert d.call(lib, **host) == 0
        w = list(want)
        w[1] = (status, None, None)
        C.check(d.back(), w)
    # the device's windows ask for a variant that the host's copies did not launch
    wide = C._page(np.random.default_rng(8), (150, 12), 73, (0, 68), (70, 73), 6)
    pk = C.pack(lib, [pages[0], wide], 6)
    narrow, early = pk.hi.copy(), pk.lo.copy()
    narrow[2], early[3] = 60, 58
    d = _Device(pk)
    assert d.call(lib, hi_host=narrow, lo_host=early) == 0
    assert d.back().status.tolist() == [R.OK, R.BOUNDS]


def test_host_side_refusals_touch_nothing_and_the_good_call_then_runs(lib):
    from text_alignment_amd import _native
    rng = np.random.default_rng(9)
    pages = [C._page(rng, (12, 11), 8, (0, 3), (4, 8), 6), C._page(rng, (10, 9, 11), 9, (0, 1, 6), (5, 6, 9), 6)]
    pk = C.pack(lib, pages, 6)
    d = _Device(pk)
    EINVAL, ELIMIT = -1, -4

    def arr(name, k, v):
        a = getattr(pk, name).copy()
        a[k] = v
        return a
    wide_hi, wide_lab = pk.hi.copy(), pk.lab_off.copy()
    wide_hi[:2] = 1024
    wide_lab[1:] += 1016
    for what, code, over in (
            ("null probs", EINVAL, dict(probs=None)), ("null status", EINVAL, dict(status=None)),
            ("negative nlabels", EINVAL, dict(nlabels=-1)), ("no = 129", EINVAL, dict(no=129)),
            ("workspace too small", EINVAL, dict(workspace_bytes=256)),
            ("workspace misaligned", EINVAL, dict(workspace=d.ptr("ws") + 4)),
            ("non-monotone window", EINVAL, dict(lo_host=arr("lo", 4, 0))),
            ("lo_0 != 0", EINVAL, dict(lo_host=arr("lo", 0, 1))), ("hi_last != n", EINVAL, dict(hi_host=arr("hi", 1, 7))),
            ("width 1024", ELIMIT, dict(hi_host=wide_hi, lab_off_host=wide_lab, nlabels=10 ** 6)),
            ("T > 5000", ELIMIT, dict(T_host=arr("T", 1, 5001)))):
        assert d.call(lib, **over) == code, what
    with pytest.raises(_native.NativeArgumentError):
        _native.check(d.call(lib, no=1), "ta_forced_align_pages")
    torch.cuda.synchronize()
    d.back()
    assert (pk.frames == C.POISON32).all() and (pk.score == C.POISON64).all() and (pk.status == C.POISON32).all()
    assert (pk.ws == C.POISON_BYTE).all()
    assert d.call(lib) == 0
    C.check(d.back(), [R.align_page(*pg)[:3] for pg in pages])


def test_forced_page_alignment_python_call():
    """the device-level Python call: its own workspace layout, poisoned; pages of different variants; the refusals"""
    from text_alignment_amd import forced
    rng = np.random.default_rng(10)
    pages = [C._page(rng, (40, 33, 21), 30, (0, 8, 19), (14, 24, 30), 30), C._wide(rng, 66, no=30),
             C._page(rng, (2, 1), 5, (0, 2), (4, 5), 30)]
    want = [R.align_page(*pg)[:3] for pg in pages]
    assert [w[0] for w in want] == [R.OK, R.OK, R.NOPATH]
    Ps = [P for pg in pages for P in pg[0]]
    T = [len(P) for P in Ps]
    probs = torch.from_numpy(np.concatenate(Ps)).cuda()
    row_off = np.cumsum([0] + T[:-1])
    line_first = np.cumsum([0] + [len(pg[0]) for pg in pages])
    lab_off = np.cumsum([0] + [len(pg[1]) for pg in pages])
    lo, hi = np.concatenate([pg[2] for pg in pages]), np.concatenate([pg[3] for pg in pages])
    labels = np.concatenate([pg[1] for pg in pages])
    got = forced.forced_page_alignment(probs, row_off, T, line_first, lo, hi, labels, lab_off, host=True, _fill=0xEE)
    assert got["status"].tolist() == [0, 0, forced.NOPATH]
    for p in range(2):
        assert np.array_equal(got["frames"][lab_off[p]:lab_off[p + 1]], want[p][2]) and got["score"][p] == want[p][1]
    assert (got["frames"][lab_off[2]:].view(np.uint8) == 0xEE).all() and (got["score"][2:].view(np.uint8) == 0xEE).all()
    f2, s2, st2 = forced.forced_page_alignment(probs, row_off, T, line_first, lo, hi, labels, lab_off)
    assert np.array_equal(f2.cpu().numpy()[:lab_off[2]], got["frames"][:lab_off[2]]) and st2.cpu().tolist() == [0, 0, 3]
    bad_lo, bad_hi = lo.copy(), hi.copy()
    bad_lo[1], bad_hi[2] = 15, 29
    for over in (dict(lo=bad_lo), dict(hi=bad_hi), dict(T=[0] + T[1:]), dict(line_first=[0, 3, 3, 7]),
                 dict(lab_off=[0, 30, 30, 104]), dict(row_off=row_off + 10 ** 6)):
        a = dict(row_off=row_off, T=T, line_first=line_first, lo=lo, hi=hi, lab_off=lab_off)
        a.update(over)
        with pytest.raises(ValueError):
            forced.forced_page_alignment(probs, a["row_off"], a["T"], a["line_first"], a["lo"], a["hi"], labels, a["lab_off"])
    with pytest.raises(ValueError):
        forced.forced_page_alignment(probs.double(), row_off, T, line_first, lo, hi, labels, lab_off)


def test_align_page_lines_on_three_tiny_line_images():
    """three raw line images of one page and one text: frames and score equal the checker's on the probabilities
    downloaded from that very run, every character lies on exactly one line, x is the .llocs position of t_peak"""
    from oracle import ocr_ref_f64 as OR
    from test_errs_gpu import _strip
    from text_alignment_amd import forced, ocr, train
    om = OR.synthetic_model(7001, no=40)
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    rng = np.random.default_rng(21)
    strips = [_strip(rng, 40, 90), _strip(rng, 44, 120), _strip(rng, 40, 70)]
    text = "et in terra pax hominibus"
    lines, score, run = forced.align_page_lines(rec, strips, text, want_run=True)
    P = run["probs"].cpu().numpy()
    T = [int(t) for t in run["T"]]
    Ps = [P[int(r):int(r) + t] for r, t in zip(run["row_off"], T)]
    cs = train.encode_text(om.codec, text)
    st, want_score, frames, _ = R.align_page(Ps, cs, [0] * 3, [len(cs)] * 3)
    assert st == R.OK and score == want_score and np.array_equal(run["frames"], frames)
    assert "".join(c[0] for ln in lines for c in ln) == text
    for k, ln in enumerate(lines):
        mine = frames[frames[:, 0] == k]
        assert [list(c[1:4]) for c in ln] == mine[:, 1:].tolist()
        assert [c[4] for c in ln] == FR.peak_x(mine[:, 3], T[k], strips[k].shape[1], ocr.PAD).tolist()
    # windows of the caller's: the first line may hold "et in" alone, the last "hominibus" alone
    n = len(cs)
    lo, hi = [0, 3, 16], [5, 16, n]
    lines2, score2, run2 = forced.align_page_lines(rec, strips, text, windows=(lo, hi), want_run=True)
    st, want2, frames2, _ = R.align_page(Ps, cs, lo, hi)
    assert st == R.OK and score2 == want2 and np.array_equal(run2["frames"], frames2) and score2 <= score
    assert len(lines2[0]) <= 5 and len(lines2[2]) <= n - 16
    with pytest.raises(ValueError):
        forced.align_page_lines(rec, strips, "é")
    with pytest.raises(ValueError):
        forced.align_page_lines(rec, strips, "")
    with pytest.raises(ValueError):
        forced.align_page_lines(rec, strips, "a" * 1024)
    with pytest.raises(ValueError):
        forced.align_page_lines(rec, strips[:1], "ab" * T[0])                # more characters than frames: no path
    with pytest.raises(ValueError):
        forced.align_page_lines(rec, strips, text, windows=([0, 6, 16], [5, 16, n]))     # character 5 in no window


def test_rforced_page_writes_llocs_for_the_lines_of_one_page(tmp_path):
    """tools/rforced.py --page in process: the .png files of a directory in name order against one text file; every
    NAME.llocs holds the characters align_page_lines put on that line, and together they hold the text"""
    from PIL import Image
    from oracle import ocr_ref_f64 as OR
    from test_errs_gpu import _strip
    from text_alignment_amd import forced, model_io, ocr
    from tools import rforced
    om = OR.synthetic_model(7001, no=40)
    path = str(tmp_path / "m.pyrnn.gz")
    model_io.save_pyrnn(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec), path)
    rng = np.random.default_rng(22)
    strips = [_strip(rng, 40, 100), _strip(rng, 48, 80), _strip(rng, 40, 110)]
    for k, img in enumerate(strips):
        Image.fromarray(img).save(str(tmp_path / ("line%d.png" % k)))
    (tmp_path / "page.txt").write_text("gloria in\nexcelsis  deo\n", encoding="utf-8")
    text = "gloria in excelsis deo"
    written, score = rforced.main([str(tmp_path), "-m", path, "--page", str(tmp_path / "page.txt")])
    want, want_score = forced.align_page_lines(path, strips, text)
    assert score == want_score and [w[0] for w in written] == [str(tmp_path / ("line%d.llocs" % k)) for k in range(3)]
    rows = [[r.split("\t") for r in open(w[0], encoding="utf-8").read().split("\n") if r] for w in written]
    assert "".join(r[0] for ln in rows for r in ln) == text
    for ln, chars, w in zip(rows, want, written):
        assert w[1] == len(chars) and [r[1] for r in ln] == ["%.1f" % c[4] for c in chars]
