"""The page-scope forced-alignment kernel with omission (csrc/ta_forced_page_omit.hip) on the GPU against the checker
tests/forced_page_omit_ref.py: the cases of tests/forced_page_omit_cases.py through the library with real device pointers
and through forced.forced_page_alignment(omit_q=), the refusals, forced.align_page_lines(omit=) end to end and
tools/rforced.py --page --page-omit in process.  Every output is an integer and is compared for equality; everything is
poisoned first."""
import numpy as np
import pytest

import forced_page_omit_cases as C
import forced_page_omit_ref as R
import forced_ref as FR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

UNIT = C.UNIT


class _Device(object):
    """a packed case's arrays on the device; back() copies the outputs into the packed case"""

    def __init__(self, pk):
        self.pk = pk
        self.t = {name: torch.from_numpy(getattr(pk, name)).cuda() for name in C.INPUTS + C.OUTPUTS + ("ws",)}

    def ptr(self, name):
        return self.t[name].data_ptr()

    def call(self, lib, omit, **over):
        return C.call(lib, self.pk, self.ptr, omit, torch.cuda.current_stream().cuda_stream, **over)

    def back(self):
        for name in C.OUTPUTS + ("ws",):
            getattr(self.pk, name)[...] = self.t[name].cpu().numpy()
        return self.pk


@pytest.fixture(scope="module")
def lib():
    from text_alignment_amd import _native
    return _native.lib


def _flat(pages):
    """the arguments of forced.forced_page_alignment for a list of pages, without gaps"""
    Ps = [P for pg in pages for P in pg[0]]
    T = [len(P) for P in Ps]
    return dict(probs=torch.from_numpy(np.ascontiguousarray(np.concatenate(Ps), dtype=np.float32)).cuda(),
                row_off=np.cumsum([0] + T[:-1]), T=T, line_first=np.cumsum([0] + [len(pg[0]) for pg in pages]),
                lo=np.concatenate([pg[2] for pg in pages]), hi=np.concatenate([pg[3] for pg in pages]),
                labels=np.concatenate([pg[1] for pg in pages]), lab_off=np.cumsum([0] + [len(pg[1]) for pg in pages]))


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_kernel_equals_the_checker(lib, case):
    from text_alignment_amd import forced
    name, no, omit, pages = case
    want = C.want(name, pages, omit)
    d = _Device(C.pack(lib, pages, no))
    assert d.call(lib, omit) == 0
    C.check(d.back(), want)
    if name.startswith(C.STRICT):
        C.check(d.pk, C.strict_want(pages))
    # the same case through the device-level Python call: its own layout, poisoned
    a = _flat(pages)
    got = forced.forced_page_alignment(a["probs"], a["row_off"], a["T"], a["line_first"], a["lo"], a["hi"], a["labels"],
                                       a["lab_off"], host=True, _fill=0xEE, omit_q=omit)
    assert got["status"].tolist() == [0] * len(pages)
    assert np.array_equal(got["frames"], np.concatenate([w[2] for w in want]))
    assert got["score"].tolist() == [w[1] for w in want]


def test_a_page_refused_through_its_data_leaves_its_neighbours_alone(lib):
    rng = np.random.default_rng(7)
    omit = 2 * UNIT
    pages = [C._page(rng, (12, 11), 8, (0, 3), (4, 8), 6), C._page(rng, (4, 3, 5), 14, (0, 1, 8), (6, 9, 14), 6), C._wide(rng, 70)]
    want = [R.answer(*pg, omit) for pg in pages]
    a = int(C.pack(lib, pages, 6).lab_off[1])
    edits = [(R.LABEL, "labels", a + 2, 6), (R.LABEL, "labels", a + 13, 0), (R.BOUNDS, "lo", 2, 1), (R.BOUNDS, "hi", 4, 13),
             (R.BOUNDS, "lo", 3, 7), (R.BOUNDS, "lo", 4, 0), (R.BOUNDS, "hi", 3, 5), (R.BOUNDS, "hi", 3, 1030),
             (R.BOUNDS, "T", 3, 0), (R.BOUNDS, "T", 3, 5001), (R.BOUNDS, "row_off", 4, 10 ** 9), (R.BOUNDS, "row_off", 2, -3),
             (R.BOUNDS, "ws_off", 2, 8), (R.BOUNDS, "ws_off", 3, 10 ** 12), (R.BOUNDS, "ws_off", 4, -16)]
    for status, name, k, v in edits:
        pk = C.pack(lib, pages, 6)
        host = {h: getattr(pk, h[:-5]).copy() for h in C.HOST}                # the host's copies stay right
        getattr(pk, name)[k] = v
        d = _Device(pk)
        assert d.call(lib, omit, **host) == 0
        w = list(want)
        w[1] = (status, None, None)
        C.check(d.back(), w)
    # the device's windows ask for a variant that the host's copies did not launch
    wide = C._page(np.random.default_rng(8), (15, 12), 73, (0, 68), (70, 73), 6)
    pk = C.pack(lib, [pages[0], wide], 6)
    narrow, early = pk.hi.copy(), pk.lo.copy()
    narrow[2], early[3] = 60, 58
    d = _Device(pk)
    assert d.call(lib, omit, hi_host=narrow, lo_host=early) == 0
    assert d.back().status.tolist() == [R.OK, R.BOUNDS]


def test_host_side_refusals_touch_nothing_and_the_good_call_then_runs(lib):
    from text_alignment_amd import _native
    rng = np.random.default_rng(9)
    omit = 2 * UNIT
    pages = [C._page(rng, (12, 11), 8, (0, 3), (4, 8), 6), C._page(rng, (4, 3, 5), 14, (0, 1, 8), (6, 9, 14), 6)]
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
    long_hi, long_lab = pk.hi.copy(), pk.lab_off.copy()
    long_hi[1] = (1 << 20) + 1
    long_lab[1:] += (1 << 20) + 1 - 8
    many = 6711                                          # 6711 lines of 5000 frames: more than 2^25
    T_many = np.full(many + 3, 5000, np.int32)
    lf_many = np.asarray([0, many, many + 3], np.int64)
    lo_many = np.concatenate([[0], np.full(many - 1, pk.lo[1]), pk.lo[2:5]]).astype(np.int32)
    hi_many = np.concatenate([[pk.hi[0]], np.full(many - 1, pk.hi[1]), pk.hi[2:5]]).astype(np.int32)
    for what, code, over in (
            ("omit -1", EINVAL, dict(omit_q=-1)), ("omit above the maximum", EINVAL, dict(omit_q=(1 << 26) + 1)),
            ("2^20 + 1 characters", ELIMIT, dict(hi_host=long_hi, lab_off_host=long_lab, nlabels=1 << 22)),
            ("more than 2^25 frames", ELIMIT, dict(T_host=T_many, line_first_host=lf_many, lo_host=lo_many, hi_host=hi_many,
                                                   nlines=many + 3, rows=1 << 40, workspace_bytes=1 << 40)),
            ("null probs", EINVAL, dict(probs=None)), ("null status", EINVAL, dict(status=None)),
            ("negative nlabels", EINVAL, dict(nlabels=-1)), ("no = 129", EINVAL, dict(no=129)),
            ("workspace too small", EINVAL, dict(workspace_bytes=256)),
            ("workspace misaligned", EINVAL, dict(workspace=d.ptr("ws") + 4)),
            ("non-monotone window", EINVAL, dict(lo_host=arr("lo", 4, 0))),
            ("lo_0 != 0", EINVAL, dict(lo_host=arr("lo", 0, 1))), ("hi_last != n", EINVAL, dict(hi_host=arr("hi", 1, 7))),
            ("width 1024", ELIMIT, dict(hi_host=wide_hi, lab_off_host=wide_lab, nlabels=10 ** 6)),
            ("T > 5000", ELIMIT, dict(T_host=arr("T", 1, 5001)))):
        assert d.call(lib, omit, **over) == code, what
    with pytest.raises(_native.NativeArgumentError):
        _native.check(d.call(lib, omit, no=1), "ta_forced_align_pages_omit")
    torch.cuda.synchronize()
    d.back()
    assert (pk.frames == C.POISON32).all() and (pk.score == C.POISON64).all() and (pk.status == C.POISON32).all()
    assert (pk.ws == C.POISON_BYTE).all()
    assert d.call(lib, omit) == 0
    C.check(d.back(), [R.answer(*pg, omit) for pg in pages])


def test_forced_page_alignment_python_call_with_omit_q():
    """pages of different variants in one call, two of them pages the strict lattice has no path for, omit_q=None byte for
    byte the strict call, and the refusals"""
    from text_alignment_amd import forced
    rng = np.random.default_rng(10)
    pages = [C._page(rng, (40, 33, 21), 30, (0, 8, 19), (14, 24, 30), 30), C._wide(rng, 66, no=30),
             C._page(rng, (2, 1), 5, (0, 2), (4, 5), 30)]
    omit = 3 * UNIT
    want = [R.answer(*pg, omit) for pg in pages]
    a = _flat(pages)
    args = (a["probs"], a["row_off"], a["T"], a["line_first"], a["lo"], a["hi"], a["labels"], a["lab_off"])
    got = forced.forced_page_alignment(*args, host=True, _fill=0xEE, omit_q=omit)
    assert got["status"].tolist() == [0, 0, 0]
    assert np.array_equal(got["frames"], np.concatenate([w[2] for w in want])) and got["score"].tolist() == [w[1] for w in want]
    assert (got["frames"][a["lab_off"][2]:] == forced.OMITTED).any()           # three frames cannot hold five characters
    f2, s2, st2 = forced.forced_page_alignment(*args, omit_q=np.int64(omit))
    assert np.array_equal(f2.cpu().numpy(), got["frames"]) and st2.cpu().tolist() == [0, 0, 0]
    strict = forced.forced_page_alignment(*args, host=True, _fill=0xEE)
    again = forced.forced_page_alignment(*args, host=True, _fill=0xEE, omit_q=None)
    assert strict["status"].tolist() == [0, forced.NOPATH, forced.NOPATH]       # pages 1 and 2: more characters than frames
    assert all(np.array_equal(strict[k], again[k]) for k in strict)
    for bad in (-1, (1 << 26) + 1, 1.5, True, "4"):
        with pytest.raises(ValueError):
            forced.forced_page_alignment(*args, omit_q=bad)
    bad_lo = a["lo"].copy()
    bad_lo[1] = 15
    with pytest.raises(ValueError):
        forced.forced_page_alignment(a["probs"], a["row_off"], a["T"], a["line_first"], bad_lo, a["hi"], a["labels"], a["lab_off"],
                                     omit_q=omit)
    # a page of 2^20 + 1 characters: the host's limit, before anything is uploaded or launched
    n, nl = (1 << 20) + 1, 1100                          # 1100 lines of one frame, windows of at most 1023 characters
    lo = np.minimum(np.arange(nl) * 1000, n)
    hi = np.minimum(lo + 1023, n)
    hi[-1] = n
    with pytest.raises(ValueError, match="2\\^20"):
        forced.forced_page_alignment(a["probs"], np.zeros(nl, np.int64), np.ones(nl, np.int64), [0, nl], lo, hi,
                                     np.ones(n, np.int32), [0, n], omit_q=omit)


def test_align_page_lines_with_omit_on_three_tiny_line_images():
    """three raw line images of one page and a text with letters the page lacks: frames and score equal the checker's on
    the probabilities downloaded from that very run, the present characters lie on one line each, the omitted ones are
    named, and a text with more characters than frames has a path"""
    from oracle import ocr_ref_f64 as OR
    from test_errs_gpu import _strip
    from text_alignment_amd import forced, ocr, train
    om = OR.synthetic_model(7001, no=40)
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    rng = np.random.default_rng(21)
    strips = [_strip(rng, 40, 90), _strip(rng, 44, 120), _strip(rng, 40, 70)]
    text = "et in terra pax hominibus"
    omit = 4.0
    lines, score, run, gone = forced.align_page_lines(rec, strips, text, want_run=True, omit=omit)
    P = run["probs"].cpu().numpy()
    T = [int(t) for t in run["T"]]
    Ps = [P[int(r):int(r) + t] for r, t in zip(run["row_off"], T)]
    cs = train.encode_text(om.codec, text)
    st, want_score, frames = R.answer(Ps, cs, [0] * 3, [len(cs)] * 3, forced.omit_units(omit))
    assert st == R.OK and score == want_score and np.array_equal(run["frames"], frames)
    assert gone == np.flatnonzero(frames[:, 0] == R.OMITTED).tolist()
    assert "".join(c[0] for ln in lines for c in ln) == "".join(ch for i, ch in enumerate(text) if i not in gone)
    for k, ln in enumerate(lines):
        mine = frames[frames[:, 0] == k]
        assert [list(c[1:4]) for c in ln] == mine[:, 1:].tolist()
        assert [c[4] for c in ln] == FR.peak_x(mine[:, 3], T[k], strips[k].shape[1], ocr.PAD).tolist()
    # without omit: three values, as before
    assert len(forced.align_page_lines(rec, strips, text, want_run=True)) == 3 and len(forced.align_page_lines(rec, strips, text)) == 2
    # more characters than frames: the strict call refuses, the call with omit answers and omits
    long_text = "ab" * T[0]
    with pytest.raises(ValueError):
        forced.align_page_lines(rec, strips[:1], long_text)
    lines3, score3, gone3 = forced.align_page_lines(rec, strips[:1], long_text, omit=omit)
    cs3 = train.encode_text(om.codec, long_text)
    st, want3, frames3 = R.answer(Ps[:1], cs3, [0], [len(cs3)], forced.omit_units(omit))
    assert score3 == want3 and len(gone3) >= len(long_text) - T[0] and len(lines3[0]) + len(gone3) == len(long_text)
    for bad in (-1.0, 1025, "4"):
        with pytest.raises(ValueError):
            forced.align_page_lines(rec, strips, text, omit=bad)
    with pytest.raises(ValueError):
        forced.align_page_lines(rec, strips, "a" * 1024, omit=omit)


def test_rforced_page_omit_writes_llocs_for_the_present_characters(tmp_path, capsys):
    """tools/rforced.py --page TEXT --page-omit BITS in process: every NAME.llocs holds the present characters
    align_page_lines(omit=) put on that line, the omitted ones are named on stderr; --page with --omit keeps exiting"""
    from PIL import Image
    from oracle import ocr_ref_f64 as OR
    from test_errs_gpu import _strip
    from text_alignment_amd import forced, model_io, ocr
    from tools import rforced
    om = OR.synthetic_model(7001, no=40)
    path = str(tmp_path / "m.pyrnn.gz")
    model_io.save_pyrnn(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec), path)
    rng = np.random.default_rng(22)
    strips = [_strip(rng, 40, 30), _strip(rng, 48, 24), _strip(rng, 40, 28)]
    for k, img in enumerate(strips):
        Image.fromarray(img).save(str(tmp_path / ("line%d.png" % k)))
    text = " ".join(["gloria in excelsis deo et in terra pax hominibus bone voluntatis"] * 3)
    (tmp_path / "page.txt").write_text(text.replace(" in ", "\nin "), encoding="utf-8")
    written, score = rforced.main([str(tmp_path), "-m", path, "--page", str(tmp_path / "page.txt"), "--page-omit", "4"])
    err = capsys.readouterr().err
    want, want_score, gone = forced.align_page_lines(path, strips, text, omit=4.0)
    assert score == want_score and [w[0] for w in written] == [str(tmp_path / ("line%d.llocs" % k)) for k in range(3)]
    assert gone and "omitted" in err and all("%d:%r" % (i, text[i]) in err for i in gone)
    rows = [[r.split("\t") for r in open(w[0], encoding="utf-8").read().split("\n") if r] for w in written]
    assert "".join(r[0] for ln in rows for r in ln) == "".join(ch for i, ch in enumerate(text) if i not in gone)
    for ln, chars, w in zip(rows, want, written):
        assert w[1] == len(chars) and [r[1] for r in ln] == ["%.1f" % c[4] for c in chars]
    with pytest.raises(SystemExit, match="--page-omit"):
        rforced.main([str(tmp_path), "-m", path, "--page", str(tmp_path / "page.txt"), "--omit", "4"])
    with pytest.raises(SystemExit):
        rforced.main([str(tmp_path), "-m", path, "--page", str(tmp_path / "page.txt"), "--page-omit", "-1"])
    with pytest.raises(SystemExit):
        rforced.main([str(tmp_path), "-m", path, "--page-omit", "4"])
