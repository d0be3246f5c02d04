"""GPU tests of line-model training (text_alignment_amd/train.py, csrc/ta_train.hip) against the float64 numpy
checker tests/train_ref.py.

Two tolerances hold every comparison with the checker, both computed on the CPU from the checker alone:
  * the checker's own float32-versus-float64 gap on the same inputs (the same loops with every array cast to float32):
    the GPU result must be closer to the float64 checker than that gap by the factor RATIO_BOUND = 0.1, which a float32
    implementation, sitting at a ratio around 1, cannot pass;
  * the float64 checker's distance from its own long-double run (train_ref.noise64): the GPU result must lie within
    train_ref.bound64 = 64 x max(noise64, 4 ulp of the array's largest reference magnitude), which a float64
    implementation that drops a small term cannot pass (tests/test_train_cases.py shows it on the edge cases).
tools/train_agreement.py measures both and writes them to profiles/train_agreement.json, recorded on an MI355X: ratios
below 6e-9 against the float32 gap and quotients error / max(noise64, 4 ulp) below 2.2 of the 64 allowed on these batches.  The edges of the
kernels are in tests/test_train_edges_gpu.py."""
import numpy as np
import pytest

import train_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RATIO_BOUND = 0.1


def _within_noise(got, ref64, refld, what):
    """the second tolerance: `got` within bound64 of the float64 checker"""
    err, noise = R.distance(got, ref64), R.noise64(ref64, refld)
    print("%s: error %.3g, noise64 %.3g, bound %.3g" % (what, err, noise, R.bound64(ref64, noise)))
    assert err <= R.bound64(ref64, noise), what


def _trainer(fwd, rev, W2, codec, **kw):
    from text_alignment_amd import ocr, train
    return train.LineTrainer(model=ocr.LineModel(fwd, rev, W2, codec), **kw)


def _flat(g):
    return [("fwd " + k, g["fwd"][k]) for k in R.GATES + R.PEEPS] + [("rev " + k, g["rev"][k]) for k in R.GATES + R.PEEPS] + [("W2", g["W2"])]


def test_aligned_targets_match_the_checker():
    """`align` on lines of T = 40 .. 400: the lattice alone is compared -- the checker aligns the PRODUCT's outputs"""
    fwd, rev, W2, codec, lines, texts, codes = R.spec_batch()
    got = _trainer(fwd, rev, W2, codec).align(lines, texts, want_probs=True)
    assert [a.shape[0] for a, _ in got] == [40, 97, 150, 233, 400]
    for (al, probs), cs in zip(got, codes):
        ref64 = R.ctc_align_targets(probs, cs)
        ref32 = R.ctc_align_targets(probs, cs, dtype=np.float32)
        err, gap, ratio = R.closeness(al, ref64, ref32)
        print("aligned T=%d: error %.3g, float32 gap %.3g, ratio %.3g" % (al.shape[0], err, gap, ratio))
        assert ratio <= RATIO_BOUND
        _within_noise(al, ref64, R.ctc_align_targets(probs, cs, dtype=np.longdouble), "aligned T=%d" % al.shape[0])
        assert np.abs(al.sum(axis=1) - 1).max() < 1e-12


def test_gradients_match_the_checker():
    """`gradients` of the same batch: every weight array of every line against the checker on the same weights"""
    fwd, rev, W2, codec, lines, texts, codes = R.spec_batch()
    got = _trainer(fwd, rev, W2, codec).gradients(lines, texts)
    for g, xs, cs in zip(got, lines, codes):
        ref64 = R.gradients(fwd, rev, W2, xs, cs)
        ref32 = R.gradients(fwd, rev, W2, xs, cs, dtype=np.float32)
        refld = R.gradients(fwd, rev, W2, xs, cs, dtype=np.longdouble)
        for (name, a), (_, b), (_, c), (_, e) in zip(_flat(g), _flat(ref64), _flat(ref32), _flat(refld)):
            err, gap, ratio = R.closeness(a, b, c)
            print("T=%d %s: error %.3g, float32 gap %.3g, ratio %.3g" % (xs.shape[0], name, err, gap, ratio))
            assert a.shape == b.shape and ratio <= RATIO_BOUND, name
            _within_noise(a, b, e, "T=%d %s" % (xs.shape[0], name))
        assert abs(g["error"] - ref64["error"]) <= RATIO_BOUND * max(abs(ref32["error"] - ref64["error"]), 1e-9)
        assert g["decoded"] == "".join(codec[c] for c in R.translate_back(ref64["probs"]))


def _twenty_lines():
    fwd, rev, W2, codec, _, _, _ = R.spec_batch()
    lengths = [40 + 8 * k for k in range(20)]                      # T 40 .. 192
    _, _, _, _, lines, texts, codes = R.spec_batch(seed=32, lengths=lengths)
    return fwd, rev, W2, codec, lines, texts, codes


def test_twenty_sequential_updates_match_the_checker():
    """20 updates over 20 lines, one line each (ocropy's schedule): the final weights against the checker's 20 updates.
    A large rate (1e-2) so that the updates move the weights by more than rounding."""
    fwd, rev, W2, codec, lines, texts, codes = _twenty_lines()
    tr = _trainer(fwd, rev, W2, codec, lrate=1e-2, momentum=0.9, lines_per_update=1)
    res = tr.train(lines, texts)
    assert len(res) == 20 and all(np.isfinite(r["error"]) for r in res)
    c64 = R.Trainer(fwd, rev, W2, lrate=1e-2, momentum=0.9)
    c32 = R.Trainer(fwd, rev, W2, lrate=1e-2, momentum=0.9, dtype=np.float32)
    cld = R.Trainer(fwd, rev, W2, lrate=1e-2, momentum=0.9, dtype=np.longdouble)
    for xs, cs in zip(lines, codes):
        c64.update([xs], [cs])
        c32.update([xs], [cs])
        cld.update([xs], [cs])
    m = tr.model()
    got = {"fwd": m.fwd, "rev": m.rev, "W2": m.W2}
    for (name, a), (_, b), (_, c), (_, e) in zip(_flat(got), _flat({"fwd": c64.fwd, "rev": c64.rev, "W2": c64.W2}),
                                                 _flat({"fwd": c32.fwd, "rev": c32.rev, "W2": c32.W2}),
                                                 _flat({"fwd": cld.fwd, "rev": cld.rev, "W2": cld.W2})):
        err, gap, ratio = R.closeness(a, b, c)
        print("%s after 20 updates: error %.3g, float32 gap %.3g, ratio %.3g" % (name, err, gap, ratio))
        assert ratio <= RATIO_BOUND, name
        _within_noise(a, b, e, name + " after 20 updates")
    assert np.abs(m.W2 - W2).max() > 1e-4                          # the weights did move


def test_batched_update_is_the_sum_of_the_single_line_gradients():
    """lines_per_update = 4: one update from the four lines' gradients against the SAME weights.  The only difference
    from adding up `gradients` is the order of float64 additions (one product over the four lines' rows instead of
    four): bound 1e-12 of the largest entry of the update."""
    fwd, rev, W2, codec, lines, texts, _ = R.spec_batch()
    lines, texts = lines[:4], texts[:4]
    single = _trainer(fwd, rev, W2, codec).gradients(lines, texts)
    tr = _trainer(fwd, rev, W2, codec, lrate=1e-3, momentum=0.9, lines_per_update=4)
    res = tr.train(lines, texts)
    assert np.allclose([r["error"] for r in res], [g["error"] for g in single], rtol=1e-12, atol=0)
    m = tr.model()
    moved = {"fwd": {k: m.fwd[k] - fwd[k] for k in fwd}, "rev": {k: m.rev[k] - rev[k] for k in rev}, "W2": m.W2 - W2}
    for k, (name, a) in enumerate(_flat(moved)):
        want = 1e-3 * sum(_flat(g)[k][1] for g in single)
        # (W + ds) - W loses the bits of ds below W's last place: half a unit of that per entry on top
        assert np.abs(a - want).max() <= 1e-12 * np.abs(want).max() + 2.3e-16, name
        assert np.abs(want).max() > 0


@pytest.fixture(scope="module")
def learned():
    """2000 single-line updates on the synthetic glyph task (tests/train_ref.py: glyph_task / glyph_line), fresh model,
    lrate 3e-3, momentum 0.9.  The condition was confirmed with the checker alone on the CPU (same seeds): every line of
    the last 250 decoded exactly before its update from update 1750 on, and 100 of 100 fresh lines afterwards."""
    from text_alignment_amd import train
    glyphs = R.glyph_task(0)
    rng = np.random.default_rng(1)
    pairs = [R.glyph_line(glyphs, rng) for _ in range(2000)]
    tr = train.LineTrainer(charset="abcde", lrate=3e-3, momentum=0.9, lines_per_update=1, seed=0)
    assert tr.codec == ["", " ", "~", "a", "b", "c", "d", "e"]
    texts = ["".join(tr.codec[c] for c in cs) for _, cs in pairs]
    res = tr.train([xs.astype(np.float32) for xs, _ in pairs], texts)
    return tr, glyphs, res, texts


def _fresh_lines(tr, glyphs):
    rng = np.random.default_rng(2)
    pairs = [R.glyph_line(glyphs, rng) for _ in range(100)]
    return [xs.astype(np.float32) for xs, _ in pairs], ["".join(tr.codec[c] for c in cs) for _, cs in pairs]


def _read(model, lines):
    from text_alignment_amd import ocr
    rec = ocr.LineRecognizer(model)                                # the default precision
    return ["".join(model.codec[c] for _, c in dec) for dec in rec.recognise(lines)]


def test_it_learns(learned):
    tr, glyphs, res, texts = learned
    print("error per timestep: first %.3g, last %.3g; decoded exactly before their update among the last 250: %d"
          % (res[0]["error"] / 72, res[-1]["error"] / 72, sum(1 for r, t in zip(res[-250:], texts[-250:]) if r["decoded"] == t)))
    lines, texts = _fresh_lines(tr, glyphs)
    got = _read(tr.model(), lines)
    nright = sum(1 for a, b in zip(got, texts) if a == b)
    print("fresh lines decoded exactly: %d of 100" % nright)
    assert nright >= 99


def test_trained_model_reloads(learned, tmp_path):
    from text_alignment_amd import model_io
    tr, glyphs, _, _ = learned
    lines, _ = _fresh_lines(tr, glyphs)
    path = str(tmp_path / "glyphs.pyrnn.gz")
    model_io.save_pyrnn(tr.model(), path)
    assert _read(model_io.load_pyrnn(path), lines) == _read(tr.model(), lines)


def test_ctc_align_targets_on_device_tensors():
    from text_alignment_amd import train
    rng = np.random.default_rng(8)
    T, labels, no = [30, 12], [[3, 3, 4], [5]], 7
    P = rng.random((sum(T), no))
    P /= P.sum(axis=1, keepdims=True)
    al, de, err = train.ctc_align_targets(torch.from_numpy(P).cuda(), T, labels)
    al, de, err = al.cpu().numpy(), de.cpu().numpy(), err.cpu().numpy()
    for k, (a, b) in enumerate([(0, 30), (30, 42)]):
        ref = R.ctc_align_targets(P[a:b], labels[k])
        _within_noise(al[a:b], ref, R.ctc_align_targets(P[a:b], labels[k], dtype=np.longdouble), "aligned, line %d" % k)
        assert np.abs(al[a:b] - ref).max() < 1e-12
        assert np.abs(de[a:b] - (ref - P[a:b])).max() < 1e-12 and abs(err[k] - ((ref - P[a:b]) ** 2).sum()) < 1e-12
    with pytest.raises(ValueError):
        train.ctc_align_targets(torch.from_numpy(P).cuda(), T, [[3, 3, 4], [5, 5, 5, 5, 5, 5]])     # 13 states, T = 12
