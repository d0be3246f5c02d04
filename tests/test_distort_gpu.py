"""Line distortion on the GPU (csrc/ta_distort.hip, text_alignment_amd/augment.py) against the
numpy checker tests/distort_ref.py, and through the normaliser and the trainer."""
import numpy as np
import pytest
import torch

import distort_ref as R

pytestmark = pytest.mark.gpu

SEED, FIRST = 12345, 7
DISTORT = 3.0
# 9 x 33 at dsigma 10 (radius 40: more than 2 h and more than w, both axes reflect several times); 20 x 70; 33 x 64 (the
# dsigma 2.5 case); 48 x 300 (made bilevel); 61 x 1400: several column tiles with a partial tail, two row tiles;
# 130 x 257: taller than a usual strip, odd sizes; 1 x 40: a single row; 3 x 1793: the narrowest strip with nine outputs
# per lane in the row pass (the others take five or seven)
SHAPES = [(9, 33), (20, 70), (33, 64), (48, 300), (61, 1400), (130, 257), (1, 40), (3, 1793)]
SIGMAS = [10.0, 2.5]        # a call has ONE sigma: the whole batch runs in one call at each


def _strip(rng, h, w, wobble=0.0):
    """word-like ink blobs around a (possibly curved) baseline, grey-level antialiasing"""
    yy = np.arange(h)[:, None]
    base = h / 2.0 + wobble * np.sin(np.arange(w) / 97.0)[None, :]
    dens = 0.6 * np.exp(-0.5 * ((yy - base) / (h / 7.0)) ** 2)
    ink = rng.random((h, w)) < dens
    gaps = np.zeros(w, bool)
    x = int(rng.integers(5, 40))
    while x < w:
        g = int(rng.integers(8, 30))
        gaps[x:x + g] = True
        x += g + int(rng.integers(40, 120))
    ink[:, gaps] = False
    grey = np.where(ink, rng.integers(0, 90, size=(h, w)), rng.integers(235, 256, size=(h, w)))
    return grey.astype(np.uint8)


@pytest.fixture(scope="module")
def strips():
    rng = np.random.default_rng(17)
    out = [_strip(rng, h, w, wobble=(3.0 if k % 2 else 0.0)) for k, (h, w) in enumerate(SHAPES)]
    out[3] = np.where(out[3] < 128, 0, 255).astype(np.uint8)             # bilevel, as the page cutter saves them
    return out


@pytest.fixture(scope="module")
def reference(strips):
    """the checker's (out, v, d) of every strip at every sigma, computed once"""
    return {sig: [R.distort_strip(s, DISTORT, sig, SEED, FIRST + k) for k, s in enumerate(strips)] for sig in SIGMAS}


def _host(dstrips):
    return [d.cpu().numpy() for d in dstrips]


def test_fields_and_pixels_match_the_checker(strips, reference):
    from text_alignment_amd import augment
    close = total = 0
    for sig in SIGMAS:
        out, fields = augment.distort_strips(strips, DISTORT, sig, seed=SEED, first_counter=FIRST, want_fields=True)
        assert all(o.buffer is out[0].buffer for o in out)                # ONE packed buffer
        assert [o.start for o in out] == np.cumsum([0] + [s.size for s in strips])[:-1].tolist()
        for k, (o, f, (ref_out, v, d), s) in enumerate(zip(_host(out), fields, reference[sig], strips)):
            f = f.cpu().numpy()
            assert o.shape == s.shape and o.dtype == np.uint8 and f.shape == (2,) + s.shape
            err = np.abs(f - d).max()
            print("%s sigma %g: max |D_gpu - D_ref| = %.3g" % (SHAPES[k], sig, err))
            # float64 rounding through ~330 additions and a few-ulp log / cos is ~1e-13 relative; a float32 field sits at 1e-7
            assert err <= 1e-9 * DISTORT
            # a pixel may differ only where v lies within 1e-6 of a half-integer (field bound x the steepest gradient, 255)
            near = np.abs(v - np.floor(v) - 0.5) < 1e-6
            close += int(near.sum())
            total += near.size
            assert np.array_equal(o[~near], ref_out[~near]), (SHAPES[k], sig)
            if sig == 10.0 and k == 4:
                # something was moved: most pixels of a grey strip differ from the input
                moved = float((o != s).mean())
                print("pixels of the 61 x 1400 strip that differ from the input: %.1f %%" % (100 * moved))
                assert moved > 0.5
    print("pixels within 1e-6 of a half-integer: %d of %d" % (close, total))
    assert close <= 0.001 * total


def test_determinism_and_keys(strips):
    from text_alignment_amd import augment, page
    batch = [strips[1], strips[3], strips[5], strips[6]]
    before = [s.copy() for s in batch]
    a, fa = augment.distort_strips(batch, seed=SEED, first_counter=FIRST, want_fields=True)
    b = augment.distort_strips(batch, seed=SEED, first_counter=FIRST)
    assert torch.equal(a[0].buffer, b[0].buffer)
    for k, s in enumerate(batch):                                          # a line's result is its own
        alone = augment.distort_strips([s], seed=SEED, first_counter=FIRST + k)
        assert torch.equal(alone[0].tensor(), a[k].tensor())
    # device tensors and DeviceStrips (in one buffer, and not in order) give what host arrays give
    dev = [torch.from_numpy(s).cuda() for s in batch]
    dev_before = [t.clone() for t in dev]
    c = augment.distort_strips(dev, seed=SEED, first_counter=FIRST)
    assert torch.equal(a[0].buffer, c[0].buffer)
    packed = torch.cat([t.reshape(-1) for t in dev[::-1]])
    offs = np.cumsum([0] + [t.numel() for t in dev[::-1]])[:-1][::-1]
    spans = [page.DeviceStrip(packed, int(o), *t.shape) for o, t in zip(offs, dev)]
    packed_before = packed.clone()
    d = augment.distort_strips(spans, seed=SEED, first_counter=FIRST)
    assert torch.equal(a[0].buffer, d[0].buffer)
    mixed = augment.distort_strips([batch[0], dev[1], spans[2], batch[3]], seed=SEED, first_counter=FIRST)
    assert torch.equal(a[0].buffer, mixed[0].buffer)
    # another seed or counter is another field
    _, fs = augment.distort_strips(batch[:1], seed=SEED + 1, first_counter=FIRST, want_fields=True)
    _, fc = augment.distort_strips(batch[:1], seed=SEED, first_counter=FIRST + 1, want_fields=True)
    _, fh = augment.distort_strips(batch[:1], seed=SEED, first_counter=FIRST + 2 ** 32, want_fields=True)
    for other in (fs, fc, fh):
        assert float((other[0] - fa[0]).abs().max()) > 0.1
    assert float((fa[0] - fa[1][:, :fa[0].shape[1], :fa[0].shape[2]]).abs().max()) > 0.1      # line 1 is not line 0's field
    # the inputs are as they were
    assert all(np.array_equal(x, y) for x, y in zip(batch, before))
    assert all(torch.equal(x, y) for x, y in zip(dev, dev_before)) and torch.equal(packed, packed_before)


def test_through_the_normaliser(strips):
    from text_alignment_amd import augment, lineest_gpu
    batch = [strips[3], strips[4], strips[5]]
    out = augment.distort_strips(batch, seed=SEED, first_counter=FIRST)
    x0, T0, _ = lineest_gpu.normalize_strips(out)
    x1, T1, _ = lineest_gpu.normalize_strips(_host(out))
    assert np.array_equal(T0, T1) and torch.equal(x0, x1)
    assert [o.shape for o in out] == [s.shape for s in batch]


def test_trainer_distorts_reproducibly():
    from text_alignment_amd import augment, train
    rng = np.random.default_rng(23)
    lines = [_strip(rng, h, w) for h, w in [(44, 600), (50, 420), (61, 800), (38, 256)]]
    texts = ["abc", "dcab", "abcde", "badcab"]

    def run(distort, feed=None):
        tr = train.LineTrainer(charset="abcde", seed=5, lines_per_update=2, lrate=1e-2, distort=distort)
        for call in range(2):
            tr.train(lines if feed is None else feed(call), texts)
        assert tr.lines_seen == 8
        return [a.clone() for a in (tr.W, tr.peep, tr.W2)]
    aug = run(3.0)
    fed = run(None, lambda call: augment.distort_strips(lines, 3.0, 10.0, seed=5, first_counter=4 * call))
    plain, again = run(None), run(None)
    assert all(torch.equal(a, b) for a, b in zip(aug, fed))
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    assert all(not torch.equal(a, b) for a, b in zip(aug, plain))
    # gradients() and align() never distort
    tr = train.LineTrainer(charset="abcde", seed=5, distort=3.0)
    ref = train.LineTrainer(charset="abcde", seed=5)
    g, g0 = tr.gradients(lines[:2], texts[:2]), ref.gradients(lines[:2], texts[:2])
    assert all(np.array_equal(a["W2"], b["W2"]) for a, b in zip(g, g0)) and tr.lines_seen == 0
    assert all(np.array_equal(a, b) for a, b in zip(tr.align(lines[:2], texts[:2]), ref.align(lines[:2], texts[:2])))
