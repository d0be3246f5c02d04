"""The posterior kernel (csrc/ta_forced_post.hip) on the GPU against the checker tests/forced_post_ref.py: the cases of
tests/forced_post_cases.py through the library with real device pointers (every output and the workspace poisoned), the
device-side refusals, one line of L = 1023 and T = 2047, then forced.forced_posterior with host and device arrays and
forced.align_lines(posterior=True).  Every output word is compared for equality, the float64 ones through their int64
view."""
import numpy as np
import pytest

import forced_cases as C0
import forced_post_cases as C
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


@pytest.mark.parametrize("which", C.SETS)
@pytest.mark.parametrize("case", C.cases(), ids=lambda c: c[0])
def test_kernel_equals_the_checker_bit_for_bit(lib, case, which):
    name, no, lines = case
    tqs, wanted = C.want(name, lines)[which]
    d = _Device(C.pack(lib, lines, no, tqs))
    assert d.call(lib) == 0
    assert d.host("status").tolist() == [R0.OK] * len(lines)
    assert C.differing(d.pk, d.host, wanted) == []
    piece = np.zeros(d.pk.ws_bytes, dtype=bool)          # the workspace outside every line's piece stays poison
    for o, t, l in zip(d.pk.ws_off, d.pk.T_host, d.pk.L_host):
        piece[o:o + lib.ta_forced_posterior_workspace_bytes(int(t), int(l))] = True
    assert (d.host("ws")[~piece] == C.POISON_BYTE).all()


def test_one_line_of_1023_characters_on_2047_frames(lib):
    rng = np.random.default_rng(2047)
    lines = [(C0.probs(rng, 2047, 40), C0.text(rng, 1023, 40))]
    tqs = [np.arange(1, 2047, 2, dtype=np.int32)]        # T = S: the only frame character i can hold
    d = _Device(C.pack(lib, lines, 40, tqs))
    assert d.call(lib) == 0 and d.host("status").tolist() == [R0.OK]
    assert C.differing(d.pk, d.host, R.query_batch(lines, tqs)) == []


def test_a_line_refused_through_its_data_leaves_its_neighbours_alone(lib):
    rng = np.random.default_rng(5)
    lines = [(C0.probs(rng, 30, 6), C0.text(rng, 7, 6)), (C0.probs(rng, 21, 6), C0.text(rng, 5, 6)),
             (C0.probs(rng, 140, 6), C0.text(rng, 66, 6))]
    tqs = [C.seeded_queries(rng, len(P), len(cs)) for P, cs in lines]
    wanted = R.query_batch(lines, tqs)
    keep = np.r_[0:7, 12:78]
    packs = [(C.pack(lib, lines, 6, tqs, labels_edit={1: (2, 6)}), R0.LABEL), (C.pack(lib, lines, 6, tqs, L_dev={1: 11}), R0.BOUNDS),
             (C.pack(lib, lines, 6, tqs, L_dev={1: 0}), R0.BOUNDS)]
    for mine in ([-1, 3, 9, 9, 20], [0, 3, 9, 9, 21], [0, 3, 9, 8, 20], [20, 20, 20, 20, 0]):
        packs.append((C.pack(lib, lines, 6, [tqs[0], np.asarray(mine, np.int32), tqs[2]]), R.QUERY))
    for pk, status in packs:
        d = _Device(pk)
        assert d.call(lib) == 0
        assert d.host("status").tolist() == [R0.OK, status, R0.OK]
        for name in C.PER_LABEL:
            got = C.gather(pk, d.host(name))
            assert np.array_equal(got[keep], C.words(wanted[name])[keep]) and (got[7:12] == C.poison_of(got)).all(), name
        for name in C.PER_LINE:
            got = C.words(d.host(name))
            assert np.array_equal(got[[0, 2]], C.words(wanted[name])[[0, 2]]) and got[1] == C.poison_of(got), name
        a = int(pk.ws_off[1])                            # the refused line's piece stays poison too
        assert (d.host("ws")[a:a + 5 * 1536] == C.POISON_BYTE).all()
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
    more = [("null t_query", -1, dict(t_query=None))] + [("null " + n, -1, {n: None}) for n in C.OUTPUTS]
    for what, code, over in C0.refusals(d.pk) + more:
        if over == "misalign":
            over = dict(workspace=d.ptr("ws") + 4)
        assert d.call(lib, **over) == code, what
    assert d.call(lib, nlines=0) == 0
    torch.cuda.synchronize()
    assert C.untouched(d.host)
    assert d.call(lib) == 0
    assert d.host("status").tolist() == [0, 0]
    assert C.differing(d.pk, d.host, R.query_batch(lines, tqs)) == []


def test_forced_posterior_python_call_with_host_and_device_arrays():
    """the device-level Python call: its own workspace sizing, poisoned; queries and labels from the host or the device"""
    from text_alignment_amd import forced
    rng = np.random.default_rng(8)
    lines = [(C0.probs(rng, T, 30), C0.text(rng, L, 30)) for T, L in ((90, 30), (300, 70), (40, 1), (171, 85))]
    tqs = [C.seeded_queries(rng, len(P), len(cs)) for P, cs in lines]
    wanted = R.query_batch(lines, tqs)
    T = [len(P) for P, _ in lines]
    L = [len(cs) for _, cs in lines]
    probs = torch.from_numpy(np.concatenate([P for P, _ in lines])).cuda()
    labels, tq = np.concatenate([cs for _, cs in lines]), np.concatenate(tqs)
    row_off, lab_off = np.cumsum([0] + T[:-1]), np.cumsum([0] + L[:-1])

    def same(got, rows=slice(None), lines_=slice(None)):
        for name in C.PER_LABEL:
            assert got[name].dtype == R.DTYPES[name]
            assert np.array_equal(C.words(got[name])[rows], C.words(wanted[name])[rows]), name
        for name in C.PER_LINE:
            assert np.array_equal(C.words(got[name])[lines_], C.words(wanted[name])[lines_]), name
    got = forced.forced_posterior(probs, row_off, T, labels, lab_off, L, tq, host=True, _fill=0xEE)
    assert got["status"].tolist() == [0] * 4 and sorted(got) == sorted(forced.POSTERIOR_OUTPUTS)
    same(got)
    dev = forced.forced_posterior(probs, row_off, T, torch.from_numpy(labels).cuda(), lab_off, L, torch.from_numpy(tq).cuda())
    assert all(t.is_cuda for t in dev.values())
    same({k: t.cpu().numpy() for k, t in dev.items()})
    same(forced.forced_posterior(probs, row_off, T, labels, lab_off, L, torch.from_numpy(tq).cuda(), host=True, _fill=0x11))
    # a line whose queries decrease is refused by the kernel, by status; its rows keep the fill
    bad = tq.copy()
    bad[lab_off[1] + 3] = bad[lab_off[1] + 2] - 1 if bad[lab_off[1] + 2] > 0 else 5000
    got = forced.forced_posterior(probs, row_off, T, labels, lab_off, L, bad, host=True, _fill=0xEE)
    assert got["status"].tolist() == [0, forced.CONF_QUERY, 0, 0]
    mine = np.r_[lab_off[1]:lab_off[1] + L[1]]
    assert (got["rival_state"][mine] == np.int32(-0x11111112)).all() and got["z_x"][1] == np.int32(-0x11111112)
    same(got, np.setdiff1d(np.arange(len(tq)), mine), [0, 2, 3])
    # the two host formulas
    z_m, z_x = np.repeat(wanted["z_m"], L), np.repeat(wanted["z_x"], L)
    post = forced.posterior_values(wanted["own_m"], wanted["own_x"], z_m, z_x)
    assert post.dtype == np.float64 and R.same_bits(post, np.ldexp(wanted["own_m"] / z_m, wanted["own_x"].astype(np.int64) - z_x))
    assert R.same_bits(forced.loglik_bits(wanted["z_m"], wanted["z_x"]), np.log2(wanted["z_m"]) + wanted["z_x"])
    for over in (dict(t_query=tq[:-1]), dict(T=[90, 300, 2, 171]), dict(t_query=torch.from_numpy(tq.astype(np.int64)).cuda())):
        a = dict(probs=probs, row_off=row_off, T=T, labels=labels, lab_off=lab_off, L=L, t_query=tq)
        a.update(over)
        with pytest.raises(ValueError):
            forced.forced_posterior(**a)


def test_align_lines_with_posterior_equals_the_checker_on_the_runs_own_probabilities():
    """eight lines of a synthetic model: the posteriors at the run's own peaks equal the checker's on the probabilities
    downloaded from that very run; everything else align_lines returns is what it returns without the switch"""
    from oracle import ocr_ref_f64 as OR
    from text_alignment_amd import forced, ocr, train
    om = OR.synthetic_model(7001, no=40)
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    rng = np.random.default_rng(12)
    lines = [OR.synthetic_line(5200 + k, width=60 + 17 * k) for k in range(8)]
    letters = [c for c in om.codec[1:] if c and c != "~"]
    texts = ["".join(rng.choice(letters, size=int(rng.integers(1, (len(xs) - 1) // 2 + 1)))) for xs in lines]
    got, run, post = forced.align_lines(rec, lines, texts, want_run=True, posterior=True)
    plain = forced.align_lines(rec, lines, texts)
    assert got == plain
    got2, conf2, post2 = forced.align_lines(rec, lines, texts, confidence=True, posterior=True)
    plain2, conf = forced.align_lines(rec, lines, texts, confidence=True)
    assert got2 == plain == plain2 and all(np.array_equal(a, b) for a, b in zip(conf, conf2))
    P = run["probs"].cpu().numpy()
    for b, tx in enumerate(texts):
        Pb = P[int(run["row_off"][b]):int(run["row_off"][b]) + int(run["T"][b])]
        want = R.query(Pb, train.encode_text(om.codec, tx), [e[3] for e in got[b][0]])
        for lp in (post[b], post2[b]):
            assert isinstance(lp, forced.LinePosterior) and lp.posterior.shape == (len(tx),) and lp.posterior.dtype == np.float64
            assert R.same_bits(lp.posterior, R.posterior(want["own_m"], want["own_x"], want["z_m"], want["z_x"]))
            assert R.same_bits(lp.rival_posterior, R.posterior(want["rival_m"], want["rival_x"], want["z_m"], want["z_x"]))
            assert np.array_equal(lp.rival_state, want["rival_state"]) and lp.rival_state.dtype == np.int32
            assert lp.loglik_bits == float(R.loglik_bits(want["z_m"], want["z_x"])) and lp.loglik_bits < 0
            assert (lp.posterior > 0).all() and (lp.posterior <= 1 + 8 * len(Pb) * 2.0 ** -53).all()
    with pytest.raises(ValueError):
        forced.align_lines(rec, lines, texts, omit=1.5, posterior=True)
    assert forced.align_lines(rec, [], [], posterior=True) == ([], [])
    assert forced.align_lines(rec, [], [], confidence=True, posterior=True) == ([], [], [])
