"""The confidence kernel (csrc/ta_forced_conf.hip) on the GPU against the checker tests/forced_conf_ref.py: the cases of
tests/forced_conf_cases.py through the library with real device pointers (every output and the workspace poisoned), the
device-side refusals, then forced.forced_confidence with host and device arrays and forced.align_lines(confidence=True).
Every output is an integer and is compared for equality."""
import numpy as np
import pytest

import forced_cases as C0
import forced_conf_cases as C
import forced_conf_ref as R
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


@pytest.mark.parametrize("which", C.SETS)
@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_kernel_equals_the_checker(lib, case, which):
    name, no, lines = case
    tqs, conf, rival = C.want(name, lines)[which]
    d = _Device(C.pack(lib, lines, no, tqs))
    assert d.call(lib) == 0
    assert d.host("status").tolist() == [R0.OK] * len(lines)
    assert np.array_equal(C.gather(d.pk, d.host("confidence"), C.POISON64), conf)
    assert np.array_equal(C.gather(d.pk, d.host("rival"), C.POISON32), rival)
    piece = np.zeros(d.pk.ws_bytes, dtype=bool)          # the workspace outside every line's piece stays poison
    for o, t, l in zip(d.pk.ws_off, d.pk.T_host, d.pk.L_host):
        piece[o:o + lib.ta_forced_confidence_workspace_bytes(int(t), int(l))] = True
    assert (d.host("ws")[~piece] == C.POISON_BYTE).all()


def test_a_line_refused_through_its_data_leaves_its_neighbours_alone(lib):
    rng = np.random.default_rng(5)
    lines = [(C0.probs(rng, 30, 6), C0.text(rng, 7, 6)), (C0.probs(rng, 21, 6), C0.text(rng, 5, 6)),
             (C0.probs(rng, 140, 6), C0.text(rng, 66, 6))]
    tqs = [C.seeded_queries(rng, len(P), len(cs)) for P, cs in lines]
    conf, rival = R.query_batch(lines, tqs)
    keep = np.r_[0:7, 12:78]
    packs = [(C.pack(lib, lines, 6, tqs, labels_edit={1: (2, 6)}), R0.LABEL), (C.pack(lib, lines, 6, tqs, L_dev={1: 11}), R0.BOUNDS),
             (C.pack(lib, lines, 6, tqs, L_dev={1: 0}), R0.BOUNDS)]
    for mine in ([-1, 3, 9, 9, 20], [0, 3, 9, 9, 21], [0, 3, 9, 8, 20], [20, 20, 20, 20, 0]):
        packs.append((C.pack(lib, lines, 6, [tqs[0], np.asarray(mine, np.int32), tqs[2]]), R.QUERY))
    for pk, status in packs:
        d = _Device(pk)
        assert d.call(lib) == 0
        assert d.host("status").tolist() == [R0.OK, status, R0.OK]
        for name, want, poison in (("confidence", conf, C.POISON64), ("rival", rival, C.POISON32)):
            got = C.gather(pk, d.host(name), poison)
            assert np.array_equal(got[keep], want[keep]) and (got[7:12] == poison).all()
        a = int(pk.ws_off[1])                            # the refused line's piece stays poison too
        assert (d.host("ws")[a:a + 5 * 1024] == C.POISON_BYTE).all()
    for name, k, v in (("row_off", 2, 10 ** 9), ("lab_off", 1, -1), ("ws_off", 0, 8), ("ws_off", 2, 10 ** 12)):
        pk = C.pack(lib, lines, 6, tqs)
        getattr(pk, name)[k] = v
        d = _Device(pk)
        assert d.call(lib) == 0
        want = [R0.OK] * 3
        want[k] = R0.BOUNDS
        assert d.host("status").tolist() == want, (name, v)
    # the device's L asks for a variant that the host's copies did not launch
    pk = C.pack(lib, [lines[0], lines[2]], 6, [tqs[0], tqs[2]])
    pk.L_host[1] = 60
    d = _Device(pk)
    assert d.call(lib) == 0 and d.host("status").tolist() == [R0.OK, R0.BOUNDS]


def test_host_side_refusals_touch_nothing_and_the_good_call_then_runs(lib):
    rng = np.random.default_rng(6)
    lines = [(C0.probs(rng, 30, 6), C0.text(rng, 7, 6)), (C0.probs(rng, 21, 6), C0.text(rng, 5, 6))]
    tqs = [C.seeded_queries(rng, len(P), len(cs)) for P, cs in lines]
    d = _Device(C.pack(lib, lines, 6, tqs))
    for what, code, over in C0.refusals(d.pk) + [("null t_query", -1, dict(t_query=None)), ("null rival", -1, dict(rival=None))]:
        if over == "misalign":
            over = dict(workspace=d.ptr("ws") + 4)
        assert d.call(lib, **over) == code, what
    assert d.call(lib, nlines=0) == 0
    torch.cuda.synchronize()
    assert (d.host("confidence") == C.POISON64).all() and (d.host("rival") == C.POISON32).all()
    assert (d.host("status") == C.POISON32).all() and (d.host("ws") == C.POISON_BYTE).all()
    assert d.call(lib) == 0
    assert d.host("status").tolist() == [0, 0]
    conf, rival = R.query_batch(lines, tqs)
    assert np.array_equal(C.gather(d.pk, d.host("confidence"), C.POISON64), conf)
    assert np.array_equal(C.gather(d.pk, d.host("rival"), C.POISON32), rival)


def test_forced_confidence_python_call_with_host_and_device_arrays():
    """the device-level Python call: its own workspace sizing, poisoned; queries and labels from the host or the device"""
    from text_alignment_amd import forced
    rng = np.random.default_rng(8)
    lines = [(C0.probs(rng, T, 30), C0.text(rng, L, 30)) for T, L in ((90, 30), (300, 70), (40, 1), (171, 85))]
    tqs = [C.seeded_queries(rng, len(P), len(cs)) for P, cs in lines]
    conf, rival = R.query_batch(lines, tqs)
    T = [len(P) for P, _ in lines]
    L = [len(cs) for _, cs in lines]
    probs = torch.from_numpy(np.concatenate([P for P, _ in lines])).cuda()
    labels, tq = np.concatenate([cs for _, cs in lines]), np.concatenate(tqs)
    row_off, lab_off = np.cumsum([0] + T[:-1]), np.cumsum([0] + L[:-1])
    got = forced.forced_confidence(probs, row_off, T, labels, lab_off, L, tq, host=True, _fill=0xEE)
    assert got["status"].tolist() == [0] * 4
    assert np.array_equal(got["confidence"], conf) and np.array_equal(got["rival"], rival)
    assert got["confidence"].dtype == np.int64 and got["rival"].dtype == np.int32
    c2, r2, s2 = forced.forced_confidence(probs, row_off, T, torch.from_numpy(labels).cuda(), lab_off, L,
                                          torch.from_numpy(tq).cuda())
    assert np.array_equal(c2.cpu().numpy(), conf) and np.array_equal(r2.cpu().numpy(), rival) and not s2.any()
    c3 = forced.forced_confidence(probs, row_off, T, labels, lab_off, L, torch.from_numpy(tq).cuda(), host=True, _fill=0x11)
    assert np.array_equal(c3["confidence"], conf)
    # a line whose queries decrease is refused by the kernel, by status; its rows keep the fill
    bad = tq.copy()
    bad[lab_off[1] + 3] = bad[lab_off[1] + 2] - 1 if bad[lab_off[1] + 2] > 0 else 5000
    got = forced.forced_confidence(probs, row_off, T, labels, lab_off, L, bad, host=True, _fill=0xEE)
    assert got["status"].tolist() == [0, forced.CONF_QUERY, 0, 0] and forced.CONF_QUERY in forced.STATUS
    mine = np.r_[lab_off[1]:lab_off[1] + L[1]]
    assert (got["rival"][mine] == np.int32(-0x11111112)).all()
    rest = np.setdiff1d(np.arange(len(tq)), mine)
    assert np.array_equal(got["confidence"][rest], conf[rest])
    assert np.array_equal(forced.confidence_bits(conf), conf / 65536.0)
    for over in (dict(t_query=tq[:-1]), dict(T=[90, 300, 2, 171]), dict(t_query=torch.from_numpy(tq.astype(np.int64)).cuda())):
        a = dict(probs=probs, row_off=row_off, T=T, labels=labels, lab_off=lab_off, L=L, t_query=tq)
        a.update(over)
        with pytest.raises(ValueError):
            forced.forced_confidence(**a)


def test_align_lines_with_confidence_equals_the_checker_on_the_runs_own_probabilities():
    """lines of a synthetic model: the (confidence, rival) pairs at the run's own peaks equal the checker's on the
    probabilities downloaded from that very run; everything else align_lines returns is what it returns without"""
    from oracle import ocr_ref_f64 as OR
    from text_alignment_amd import forced, ocr, train
    om = OR.synthetic_model(7001, no=40)
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    rng = np.random.default_rng(12)
    lines = [OR.synthetic_line(5200 + k, width=60 + 17 * k) for k in range(8)]
    letters = [c for c in om.codec[1:] if c and c != "~"]
    texts = ["".join(rng.choice(letters, size=int(rng.integers(1, (len(xs) - 1) // 2 + 1)))) for xs in lines]
    got, run, conf = forced.align_lines(rec, lines, texts, want_run=True, confidence=True)
    plain = forced.align_lines(rec, lines, texts)
    assert got == plain
    got2, conf2 = forced.align_lines(rec, lines, texts, confidence=True)
    assert got2 == plain and all(np.array_equal(a, b) for a, b in zip(conf, conf2))
    P = run["probs"].cpu().numpy()
    for b, tx in enumerate(texts):
        Pb = P[int(run["row_off"][b]):int(run["row_off"][b]) + int(run["T"][b])]
        cs = train.encode_text(om.codec, tx)
        entries, sc = got[b]
        A, B, G = R.tables(Pb, cs)
        c, r, own = R.query_tables(G, [e[3] for e in entries])
        assert conf[b].dtype == np.int64 and conf[b].shape == (len(tx), 2)
        assert np.array_equal(conf[b][:, 0], c) and np.array_equal(conf[b][:, 1], r)
        assert (own == sc).all() and (c >= 0).all()
    with pytest.raises(ValueError):
        forced.align_lines(rec, lines, texts, omit=1.5, confidence=True)
    assert forced.align_lines(rec, [], [], confidence=True) == ([], [])
