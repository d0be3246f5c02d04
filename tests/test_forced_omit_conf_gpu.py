"""The confidence kernel of the lattice with omission (csrc/ta_forced_omit_conf.hip) on the GPU against the checker
tests/forced_omit_conf_ref.py: the cases of tests/forced_omit_conf_cases.py through the library with real device pointers
(every output and the workspace poisoned), the device-side refusals, the host-side ones, then
forced.forced_omit_confidence with host and device arrays.  Every output is an integer and is compared for equality."""
import numpy as np
import pytest

import forced_cases as C0
import forced_omit_conf_cases as C
import forced_omit_conf_ref as R
import forced_omit_ref as R1
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

    def call(self, lib, omit, **over):
        return C.call(lib, self.pk, self.ptr, omit, torch.cuda.current_stream().cuda_stream, **over)

    def host(self, name):
        return self.t[name].cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    from text_alignment_amd import _native
    return _native.lib


@pytest.mark.parametrize("which", C.SETS)
@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_kernel_equals_the_checker(lib, case, which):
    name, no, omit, lines = case
    qs, conf, rival = C.want(name, lines, omit)[which]
    d = _Device(C.pack(lib, lines, no, qs))
    assert d.call(lib, omit) == 0
    assert d.host("status").tolist() == [R0.OK] * len(lines)
    assert np.array_equal(C.gather(d.pk, d.host("confidence"), C.POISON64), conf)
    assert np.array_equal(C.gather(d.pk, d.host("rival"), C.POISON32), rival)
    assert (d.host("ws")[~C.pieces(lib, d.pk)] == C.POISON_BYTE).all()     # outside every line's piece: still poison


def test_a_line_refused_through_its_data_leaves_its_neighbours_alone(lib):
    rng = np.random.default_rng(5)
    omit = 3 * C.UNIT
    lines = C.three(rng)
    qs = C.three_queries(rng, lines)
    want = [R.query_list(R.tables_closed(P, cs, omit)[2], *q) for (P, cs), q in zip(lines, qs)]
    conf, rival = np.concatenate([c for c, _ in want]), np.concatenate([r for _, r in want])
    a, b = len(qs[0][0]), len(qs[0][0]) + len(qs[1][0])
    packs = [(C.pack(lib, lines, 6, qs, labels_edit={1: (2, 6)}), R0.LABEL), (C.pack(lib, lines, 6, qs, L_dev={1: 11}), R0.BOUNDS),
             (C.pack(lib, lines, 6, qs, L_dev={1: 0}), R0.BOUNDS), (C.pack(lib, lines, 6, qs, nq_dev={1: -1}), R.QUERY),
             (C.pack(lib, lines, 6, qs, nq_dev={1: 11}), R.QUERY)]
    for frames, chars in (([-1, 3, 9, 9, 20], qs[1][0]), ([0, 3, 9, 9, 21], qs[1][0]), ([0, 3, 9, 8, 20], qs[1][0]),
                          ([20, 20, 20, 20, 0], qs[1][0]), (qs[1][1], [0, 1, 5, 2, 3]), (qs[1][1], [-1, 1, 4, 2, 3])):
        mine = (np.asarray(chars, np.int32), np.asarray(frames, np.int32))
        packs.append((C.pack(lib, lines, 6, [qs[0], mine, qs[2]]), R.QUERY))
    for pk, status in packs:
        d = _Device(pk)
        assert d.call(lib, omit) == 0
        assert d.host("status").tolist() == [R0.OK, status, R0.OK]
        for name, want, poison in (("confidence", conf, C.POISON64), ("rival", rival, C.POISON32)):
            got = C.gather(pk, d.host(name), poison)
            assert np.array_equal(got[:a], want[:a]) and np.array_equal(got[b:], want[b:]) and (got[a:b] == poison).all()
        o = int(pk.ws_off[1])                            # the refused line's piece stays poison too
        assert (d.host("ws")[o:o + 5 * 1024] == C.POISON_BYTE).all()
    for name, k, v in (("row_off", 2, 10 ** 9), ("lab_off", 1, -1), ("ws_off", 0, 8), ("ws_off", 2, 10 ** 12), ("q_off", 0, -1),
                       ("q_off", 1, 10 ** 9)):
        pk = C.pack(lib, lines, 6, qs)
        getattr(pk, name)[k] = v
        d = _Device(pk)
        assert d.call(lib, omit) == 0
        want = [R0.OK] * 3
        want[k] = R0.BOUNDS
        assert d.host("status").tolist() == want, (name, v)
    # the device's L asks for a variant that the host's copies did not launch
    pk = C.pack(lib, [lines[0], lines[2]], 6, [qs[0], qs[2]])
    pk.L_host[1] = 60
    d = _Device(pk)
    assert d.call(lib, omit) == 0 and d.host("status").tolist() == [R0.OK, R0.BOUNDS]


def test_host_side_refusals_touch_nothing_and_the_good_call_then_runs(lib):
    rng = np.random.default_rng(6)
    omit = 2 * C.UNIT
    lines = C.three(rng)[:2]
    qs = C.three_queries(rng, lines)
    d = _Device(C.pack(lib, lines, 6, qs))
    for what, code, over in C.refusals(d.pk):
        if over == "misalign":
            over = dict(workspace=d.ptr("ws") + 4)
        assert d.call(lib, omit, **over) == code, what
    assert d.call(lib, omit, nlines=0) == 0
    torch.cuda.synchronize()
    assert (d.host("confidence") == C.POISON64).all() and (d.host("rival") == C.POISON32).all()
    assert (d.host("status") == C.POISON32).all() and (d.host("ws") == C.POISON_BYTE).all()
    assert d.call(lib, omit) == 0
    assert d.host("status").tolist() == [0, 0]
    want = [R.query_list(R.tables_closed(P, cs, omit)[2], *q) for (P, cs), q in zip(lines, qs)]
    assert np.array_equal(C.gather(d.pk, d.host("confidence"), C.POISON64), np.concatenate([c for c, _ in want]))
    assert np.array_equal(C.gather(d.pk, d.host("rival"), C.POISON32), np.concatenate([r for _, r in want]))


def test_workspace_bytes(lib):
    f = lib.ta_forced_omit_confidence_workspace_bytes
    assert f(3, 1, 0) == 0 and f(3, 1, 2) == 2048 and f(129, 64, 128) == 2048 * 128 and f(2047, 1023, 2046) == 16384 * 2046
    for T, L, nq in ((2, 1, 1), (5001, 5, 1), (4000, 1024, 1), (9, 3, -1), (9, 3, 7)):
        assert f(T, L, nq) == -1


def test_forced_omit_confidence_python_call_with_host_and_device_arrays():
    """the device-level Python call: its own workspace sizing, poisoned; queries and labels from the host or the device"""
    from text_alignment_amd import forced
    rng = np.random.default_rng(8)
    lines = [(C0.probs(rng, T, 30), C0.text(rng, L, 30)) for T, L in ((90, 30), (300, 70), (40, 1), (171, 85))]
    lines.append(C.C1.absent(rng, 40, 30, 12, 9))
    omit = forced.omit_units(3.5)
    kinds = ("L", "2L", "0", "1", "rule")
    qs = [C.seeded_queries(rng, len(P), len(cs), k) if k != "rule" else
          C.rule_queries(R1.align_closed(P, cs, omit)[1], len(P)) for (P, cs), k in zip(lines, kinds)]
    want = [R.query_list(R.tables_closed(P, cs, omit)[2], *q) for (P, cs), q in zip(lines, qs)]
    conf, rival = np.concatenate([c for c, _ in want]), np.concatenate([r for _, r in want])
    T = [len(P) for P, _ in lines]
    L = [len(cs) for _, cs in lines]
    nq = [len(qc) for qc, _ in qs]
    probs = torch.from_numpy(np.concatenate([P for P, _ in lines])).cuda()
    labels = np.concatenate([cs for _, cs in lines])
    q_char, q_frame = np.concatenate([qc for qc, _ in qs]), np.concatenate([qf for _, qf in qs])
    row_off, lab_off, q_off = np.cumsum([0] + T[:-1]), np.cumsum([0] + L[:-1]), np.cumsum([0] + nq[:-1])
    got = forced.forced_omit_confidence(probs, row_off, T, labels, lab_off, L, q_char, q_frame, q_off, nq, omit, host=True, _fill=0xEE)
    assert got["status"].tolist() == [0] * 5
    assert np.array_equal(got["confidence"], conf) and np.array_equal(got["rival"], rival)
    assert got["confidence"].dtype == np.int64 and got["rival"].dtype == np.int32
    c2, r2, s2 = forced.forced_omit_confidence(probs, row_off, T, torch.from_numpy(labels).cuda(), lab_off, L,
                                               torch.from_numpy(q_char).cuda(), torch.from_numpy(q_frame).cuda(), q_off, nq,
                                               np.int64(omit))
    assert np.array_equal(c2.cpu().numpy(), conf) and np.array_equal(r2.cpu().numpy(), rival) and not s2.any()
    c3 = forced.forced_omit_confidence(probs, row_off, T, labels, lab_off, L, q_char, torch.from_numpy(q_frame).cuda(), q_off, nq,
                                       omit, host=True, _fill=0x11)
    assert np.array_equal(c3["confidence"], conf)
    # a line whose frames decrease is refused by the kernel, by status; its rows keep the fill
    bad = q_frame.copy()
    bad[q_off[1] + 3] = bad[q_off[1] + 2] - 1 if bad[q_off[1] + 2] > 0 else 5000
    got = forced.forced_omit_confidence(probs, row_off, T, labels, lab_off, L, q_char, bad, q_off, nq, omit, host=True, _fill=0xEE)
    assert got["status"].tolist() == [0, forced.CONF_QUERY, 0, 0, 0]
    mine = np.r_[q_off[1]:q_off[1] + nq[1]]
    assert (got["rival"][mine] == np.int32(-0x11111112)).all()
    rest = np.setdiff1d(np.arange(len(q_frame)), mine)
    assert np.array_equal(got["confidence"][rest], conf[rest])
    a = dict(probs=probs, row_off=row_off, T=T, labels=labels, lab_off=lab_off, L=L, q_char=q_char, q_frame=q_frame, q_off=q_off,
             nq=nq, omit_q=omit)
    for over in (dict(q_frame=q_frame[:-1]), dict(T=[90, 300, 2, 171, 86]), dict(nq=[30, 141, 0, 1, nq[4]]), dict(nq=nq[:-1]),
                 dict(q_char=torch.from_numpy(q_char.astype(np.int64)).cuda()), dict(omit_q=-1), dict(omit_q=2.0), dict(omit_q=None),
                 dict(q_off=np.asarray(q_off) + 1)):
        b = dict(a)
        b.update(over)
        with pytest.raises(ValueError):
            forced.forced_omit_confidence(**b)


def _synthetic_lines():
    from oracle import ocr_ref_f64 as OR
    from text_alignment_amd import ocr
    om = OR.synthetic_model(7001, no=40)
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    rng = np.random.default_rng(12)
    lines = [OR.synthetic_line(5200 + k, width=60 + 17 * k) for k in range(8)]
    letters = [c for c in om.codec[1:] if c and c != "~"]
    texts = ["".join(rng.choice(letters, size=int(rng.integers(1, (len(xs) - 1) // 2 + 1)))) for xs in lines]
    return om, rec, lines, texts


def test_align_lines_with_omit_confidence_equals_the_checker_on_the_runs_own_probabilities():
    """lines of a synthetic model: the (value, rival) pairs equal the checker's on the probabilities downloaded from that
    very run; everything else align_lines returns is what it returns without the switch"""
    from text_alignment_amd import forced, train
    om, rec, lines, texts = _synthetic_lines()
    got, run, conf = forced.align_lines(rec, lines, texts, want_run=True, omit=1.5, omit_confidence=True)
    plain = forced.align_lines(rec, lines, texts, omit=1.5)
    assert got == plain and forced.align_lines(rec, lines, texts, omit=1.5, omit_confidence=False) == plain
    got2, conf2 = forced.align_lines(rec, lines, texts, omit=1.5, omit_confidence=True)
    assert got2 == plain and all(np.array_equal(a, b) for a, b in zip(conf, conf2))
    P = run["probs"].cpu().numpy()
    gone = 0
    for b, tx in enumerate(texts):
        Pb = P[int(run["row_off"][b]):int(run["row_off"][b]) + int(run["T"][b])]
        G = R.tables_closed(Pb, train.encode_text(om.codec, tx), forced.omit_units(1.5))[2]
        entries, sc = got[b]
        frames = np.asarray([e[1:4] for e in entries], dtype=np.int32)
        value, rival = R.line_values(G, frames)
        assert conf[b].dtype == np.int64 and conf[b].shape == (len(tx), 2)
        assert np.array_equal(conf[b][:, 0], value) and np.array_equal(conf[b][:, 1], rival)
        here = frames[:, 0] >= 0
        assert (value[here] >= 0).all() and (value[~here] <= 0).all() and (G.max(axis=1) == sc).all()
        gone += int((~here).sum())
    assert gone > 0
    for over in (dict(omit_confidence=True), dict(omit=1.5, confidence=True), dict(omit=1.5, confidence=True, omit_confidence=True)):
        with pytest.raises(ValueError):
            forced.align_lines(rec, lines, texts, **over)
    assert forced.align_lines(rec, [], [], omit=1.5, omit_confidence=True) == ([], [])


def test_rforced_with_omit_confidence_writes_a_row_per_character_and_marks_the_omitted(tmp_path, capsys):
    """tools/rforced.py --omit BITS --omit-confidence in process: NAME.conf holds a row per character of the TEXT --
    character, bits, the rival's character -- and a fourth field `omitted` on the rows of the characters NAME.llocs lacks"""
    from PIL import Image
    from oracle import ocr_ref_f64 as OR
    from test_errs_gpu import _strip
    from text_alignment_amd import forced, model_io, ocr
    from tools import rforced
    om = OR.synthetic_model(7001, no=40)
    path = str(tmp_path / "m.pyrnn.gz")
    model_io.save_pyrnn(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec), path)
    rng = np.random.default_rng(4)
    strips = [_strip(rng, 40, 180), _strip(rng, 52, 260)]
    texts = ["et in terra pax hominibus", "gloria patri et filio"]
    for k, (img, tx) in enumerate(zip(strips, texts)):
        Image.fromarray(img).save(str(tmp_path / ("l%d.png" % k)))
        (tmp_path / ("l%d.gt.txt" % k)).write_text(tx + "\n", encoding="utf-8")
    written = rforced.main([str(tmp_path), "-m", path, "--omit", "0.5", "--omit-confidence"])
    io = capsys.readouterr()
    want, conf = forced.align_lines(path, strips, texts, omit=0.5, omit_confidence=True)
    gone, lowest, nearest = 0, None, None
    for (out, score), (chars, sc), cf, tx in zip(written, want, conf, texts):
        llocs = [r.split("\t") for r in open(out, encoding="utf-8").read().split("\n")[:-1]]
        assert score == sc and [r[0] for r in llocs] == [c[0] for c in chars if c[4] is not None]
        rows = [r.split("\t") for r in open(out[:-len(".llocs")] + ".conf", encoding="utf-8").read().split("\n")[:-1]]
        assert len(rows) == len(tx)
        for row, ch, c, (v, s) in zip(rows, tx, chars, cf.tolist()):
            absent = c[4] is None
            assert row[:3] == [ch, "%.3f" % (v / 65536.0), tx[(s - 1) // 2] if s & 1 else "~"]
            assert row[3:] == (["omitted"] if absent else []) and (v <= 0 if absent else v >= 0)
            gone += absent
            if absent:
                nearest = v if nearest is None else max(nearest, v)
            else:
                lowest = v if lowest is None else min(lowest, v)
    assert gone > 0
    assert ("2 of 2 lines written, %d characters omitted, lowest confidence of a present character %.3f bits, the omission "
            "nearest to 0 %.3f bits" % (gone, lowest / 65536.0, nearest / 65536.0)) in io.out
    for bad in (["--omit-confidence"], ["--omit", "0.5", "--omit-confidence", "--page", str(tmp_path / "l0.gt.txt")]):
        with pytest.raises(SystemExit):
            rforced.main([str(tmp_path), "-m", path] + bad)
