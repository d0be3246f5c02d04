"""The omission-tolerant forced-alignment kernel (csrc/ta_forced_omit.hip) on the GPU against the checker
tests/forced_omit_ref.py: the cases of tests/forced_omit_cases.py through the library with real device pointers (every
output and the workspace poisoned), the device-side refusals, then forced.forced_alignment(omit_q=...) and
forced.align_lines(omit=...).  Every output is an integer and is compared for equality."""
import numpy as np
import pytest

import forced_cases as C0
import forced_omit_cases as C
import forced_omit_ref as R
import forced_ref as R0

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
UNIT = C.UNIT


class _Device(object):
    """a packed case's arrays on the device"""

    def __init__(self, pk):
        self.pk = pk
        self.t = {name: torch.from_numpy(getattr(pk, name)).cuda() for name in C.INPUTS + C.OUTPUTS + ("ws",)}

    def ptr(self, name):
        return self.t[name].data_ptr()

    def call(self, lib, omit, **over):
        return C.call(lib, self.pk, self.ptr, omit, torch.cuda.current_stream().cuda_stream, **over)

    def host(self, name):
        return self.t[name].cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    from text_alignment_amd import _native
    return _native.lib


@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_kernel_equals_the_checker(lib, case):
    name, no, omit, lines = case
    d = _Device(C.pack(lib, lines, no))
    assert d.call(lib, omit) == 0
    frames, score = C.want(name, lines, omit)
    assert d.host("status").tolist() == [R0.OK] * len(lines)
    assert np.array_equal(C.gather(d.pk, d.host("frames")), frames)
    assert np.array_equal(d.host("score"), score)
    if name == C.STRICT:
        strict_frames, strict_score = R0.align_batch(lines)
        assert np.array_equal(frames, strict_frames) and np.array_equal(score, strict_score)


def test_a_line_refused_through_its_data_leaves_its_neighbours_alone(lib):
    rng = np.random.default_rng(5)
    omit = 2 * UNIT
    lines = [(C0.probs(rng, 30, 6), C0.text(rng, 7, 6)), (C0.probs(rng, 21, 6), C0.text(rng, 5, 6)),
             (C0.probs(rng, 140, 6), C0.text(rng, 66, 6))]
    frames, score = R.align_batch(lines, omit)
    keep = np.r_[0:7, 12:78]
    for edit, status in ((dict(labels_edit={1: (2, 6)}), R0.LABEL), (dict(L_dev={1: 11}), R0.BOUNDS),
                         (dict(L_dev={1: 0}), R0.BOUNDS)):
        d = _Device(C.pack(lib, lines, 6, **edit))
        assert d.call(lib, omit) == 0
        assert d.host("status").tolist() == [R0.OK, status, R0.OK]
        got = C.gather(d.pk, d.host("frames"))
        assert np.array_equal(got[keep], frames[keep]) and (got[7:12] == C.POISON32).all()
        sc = d.host("score")
        assert sc[1] == C.POISON64 and np.array_equal(sc[[0, 2]], score[[0, 2]])
    orig = C.pack(lib, lines, 6).ws_off.copy()
    for name, k, v in (("row_off", 2, 10 ** 9), ("lab_off", 1, -1), ("ws_off", 0, 8), ("ws_off", 2, 10 ** 12)):
        pk = C.pack(lib, lines, 6)
        getattr(pk, name)[k] = v
        d = _Device(pk)
        assert d.call(lib, omit) == 0
        want = [R0.OK] * 3
        want[k] = R0.BOUNDS
        assert d.host("status").tolist() == want, (name, v)
        if name == "ws_off":                             # the piece the refused line would have had stays poison too
            ws, a, b = d.host("ws"), int(orig[k]), int(orig[(k + 1) % 3])
            assert (ws[a:a + 256] == C.POISON_BYTE).all() and not (ws[b:b + 256] == C.POISON_BYTE).all()
    # the device's L asks for a variant that the host's copies did not launch
    pk = C.pack(lib, [lines[0], lines[2]], 6)
    pk.L_host[1] = 60
    d = _Device(pk)
    assert d.call(lib, omit) == 0 and d.host("status").tolist() == [R0.OK, R0.BOUNDS]


def test_host_side_refusals_touch_nothing_and_the_good_call_then_runs(lib):
    from text_alignment_amd import _native
    rng = np.random.default_rng(6)
    omit = 2 * UNIT
    lines = [(C0.probs(rng, 30, 6), C0.text(rng, 7, 6)), (C0.probs(rng, 21, 6), C0.text(rng, 5, 6))]
    d = _Device(C.pack(lib, lines, 6))
    for what, code, over in C.refusals(d.pk):
        if over == "misalign":
            over = dict(workspace=d.ptr("ws") + 4)
        assert d.call(lib, omit, **over) == code, what
    with pytest.raises(_native.NativeArgumentError):
        _native.check(d.call(lib, -5), "ta_forced_align_omit")
    torch.cuda.synchronize()
    assert (d.host("frames") == C.POISON32).all() and (d.host("score") == C.POISON64).all()
    assert (d.host("status") == C.POISON32).all() and (d.host("ws") == C.POISON_BYTE).all()
    assert d.call(lib, omit) == 0
    assert d.host("status").tolist() == [0, 0]
    assert np.array_equal(C.gather(d.pk, d.host("frames")), R.align_batch(lines, omit)[0])


def test_forced_alignment_python_call_with_omit_q():
    """the device-level Python call: its own workspace sizing, poisoned; omit_q=None stays the strict aligner"""
    from text_alignment_amd import forced
    rng = np.random.default_rng(8)
    lines = [(C0.probs(rng, T, 30), C0.text(rng, L, 30)) for T, L in ((90, 30), (300, 70), (40, 1), (171, 85))]
    lines.append(C.absent(rng, 40, 30, 12, 9))
    omit = forced.omit_units(3.5)
    frames, score = R.align_batch(lines, omit)
    assert (frames == R.OMITTED).any()
    T = [len(P) for P, _ in lines]
    L = [len(cs) for _, cs in lines]
    probs = torch.from_numpy(np.concatenate([P for P, _ in lines])).cuda()
    labels = np.concatenate([cs for _, cs in lines])
    row_off, lab_off = np.cumsum([0] + T[:-1]), np.cumsum([0] + L[:-1])
    got = forced.forced_alignment(probs, row_off, T, labels, lab_off, L, host=True, _fill=0xEE, omit_q=omit)
    assert got["status"].tolist() == [0] * 5 and np.array_equal(got["frames"], frames) and np.array_equal(got["score"], score)
    f2, s2, _ = forced.forced_alignment(probs, row_off, T, torch.from_numpy(labels).cuda(), lab_off, L, omit_q=np.int64(omit))
    assert np.array_equal(f2.cpu().numpy(), frames) and np.array_equal(s2.cpu().numpy(), score)
    strict = forced.forced_alignment(probs, row_off, T, labels, lab_off, L, host=True, omit_q=None)
    want = R0.align_batch(lines)
    assert np.array_equal(strict["frames"], want[0]) and np.array_equal(strict["score"], want[1])
    for bad in (-1, forced.OMIT_MAX + 1, 2.0, True, "3"):
        with pytest.raises(ValueError):
            forced.forced_alignment(probs, row_off, T, labels, lab_off, L, omit_q=bad)
    with pytest.raises(ValueError):
        forced.forced_alignment(probs, row_off, [90, 300, 2, 171, 86], labels, lab_off, L, omit_q=omit)


def test_align_lines_with_omit_equals_the_checker_on_the_runs_own_probabilities():
    """lines of a synthetic model: frames and scores equal the checker's on the probabilities downloaded from that very
    run; an omitted character's entry is (char, -1, -1, -1, None); omit=None is the strict call"""
    from oracle import ocr_ref_f64 as OR
    from text_alignment_amd import forced, ocr, train
    om = OR.synthetic_model(7001, no=40)
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    rng = np.random.default_rng(12)
    lines = [OR.synthetic_line(5200 + k, width=60 + 17 * k) for k in range(8)]
    letters = [c for c in om.codec[1:] if c and c != "~"]
    texts = ["".join(rng.choice(letters, size=int(rng.integers(1, (len(xs) - 1) // 2 + 1)))) for xs in lines]
    got, run = forced.align_lines(rec, lines, texts, want_run=True, omit=1.5)
    P = run["probs"].cpu().numpy()
    gone = 0
    for b, (xs, tx) in enumerate(zip(lines, texts)):
        Pb = P[int(run["row_off"][b]):int(run["row_off"][b]) + int(run["T"][b])]
        score, frames, _ = R.align_closed(Pb, train.encode_text(om.codec, tx), forced.omit_units(1.5))
        entries, sc = got[b]
        assert sc == score and [e[0] for e in entries] == list(tx)
        assert np.array_equal(np.asarray([e[1:4] for e in entries], dtype=np.int32), frames)
        for e in entries:
            if e[3] == forced.OMITTED:
                assert e[1:] == (-1, -1, -1, None)
                gone += 1
            else:
                T = int(run["T"][b])
                assert e[4] == float(R0.peak_x(e[3], T, T - 2 * ocr.PAD, ocr.PAD))
    assert gone > 0                                      # random texts on a random model: something had to go
    strict = forced.align_lines(rec, lines, texts)
    assert strict == forced.align_lines(rec, lines, texts, omit=None)
    assert all(e[4] is not None for entries, _ in strict for e in entries)
    with pytest.raises(ValueError):
        forced.align_lines(rec, lines, texts, omit=-1)


def test_rforced_with_omit_writes_the_present_characters_and_names_the_rest(tmp_path, capsys):
    """tools/rforced.py --omit in process: NAME.llocs holds a row per character the path shows, in order; the omitted
    ones go to stderr and their number into the summary"""
    from PIL import Image
    from oracle import ocr_ref_f64 as OR
    from test_errs_gpu import _strip
    from text_alignment_amd import forced, model_io, ocr
    from tools import rforced
    om = OR.synthetic_model(7001, no=40)
    model = ocr.LineModel(om.fwd, om.rev, om.W2, om.codec)
    path = str(tmp_path / "m.pyrnn.gz")
    model_io.save_pyrnn(model, path)
    rng = np.random.default_rng(4)
    strips = [_strip(rng, 40, 180), _strip(rng, 52, 260)]
    texts = ["et in terra pax hominibus", "gloria patri et filio"]
    for k, (img, tx) in enumerate(zip(strips, texts)):
        Image.fromarray(img).save(str(tmp_path / ("l%d.png" % k)))
        (tmp_path / ("l%d.gt.txt" % k)).write_text(tx + "\n", encoding="utf-8")
    written = rforced.main([str(tmp_path), "-m", path, "--omit", "0.5"])
    io = capsys.readouterr()
    want = forced.align_lines(path, strips, texts, omit=0.5)
    gone = 0
    for (out, score), (chars, sc) in zip(written, want):
        rows = [r.split("\t") for r in open(out, encoding="utf-8").read().split("\n")[:-1]]
        shown = [c for c in chars if c[4] is not None]
        assert score == sc and [r[0] for r in rows] == [c[0] for c in shown]
        assert [r[1] for r in rows] == ["%.1f" % c[4] for c in shown]
        gone += len(chars) - len(shown)
        for k, c in enumerate(chars):
            if c[4] is None:
                assert "%d:%r" % (k, c[0]) in io.err
    assert gone > 0 and "2 of 2 lines written, %d characters omitted" % gone in io.out
    with pytest.raises(SystemExit):
        rforced.main([str(tmp_path), "-m", path, "--omit", "-1"])
