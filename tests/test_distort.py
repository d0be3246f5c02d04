"""Line distortion without a GPU: the numpy checker tests/distort_ref.py against the Philox
known answers and scipy.ndimage, and everything the C ABI and the Python layers refuse before the device is touched."""
import ctypes

import numpy as np
import pytest

import distort_ref as R

SHAPES = [(20, 70, 10.0), (48, 300, 10.0), (61, 1400, 20.0), (9, 33, 10.0), (33, 64, 2.5)]


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in R.philox4x32_10(*ctr, *key)) == want
    # the counter layout of the noise: pixel, 0, counter_lo, counter_hi; key seed_lo, seed_hi
    seed, counter = 0x299f31d0a4093822, 0x0370734413198a2e
    n = R.noise(1, 3, seed, counter)
    r = [int(v) for v in R.philox4x32_10(2, 0, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)]
    u = [(v + 0.5) * 2.0 ** -32 for v in r]
    assert n[0, 0, 2] == np.sqrt(-2.0 * np.log(u[0])) * np.cos(2.0 * np.pi * u[1])
    assert n[1, 0, 2] == np.sqrt(-2.0 * np.log(u[2])) * np.cos(2.0 * np.pi * u[3])


def test_weights_are_the_normalisers():
    from text_alignment_amd import lineest_gpu
    for sigma in (10.0, 20.0, 2.5, 0.1):
        a, ra = R.gauss_weights(sigma)
        b, rb = lineest_gpu._gauss_weights(sigma)
        assert ra == rb == int(4 * sigma + 0.5) and np.array_equal(a, b)


@pytest.mark.parametrize("h,w,dsigma", SHAPES)
def test_checker_against_scipy(h, w, dsigma):
    from scipy import ndimage
    rng = np.random.default_rng(h * 1000 + w)
    noise = R.noise(h, w, seed=99, counter=h)
    assert abs(noise.mean()) < 0.2 and 0.8 < noise.std() < 1.2
    for n in noise:
        diff = np.abs(R.smooth(n, dsigma) - ndimage.gaussian_filter(n, dsigma, mode="reflect")).max()
        print("fields %dx%d sigma %g: %.3g" % (h, w, dsigma, diff))
        assert diff <= 1e-15
    img = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
    out, v, d = R.distort_strip(img, 3.0, dsigma, seed=99, counter=h)
    assert np.abs(d[0]).max() == pytest.approx(3.0, abs=1e-12) and np.abs(d[1]).max() == pytest.approx(3.0, abs=1e-12)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ref = ndimage.map_coordinates(img.astype(np.float64), [yy + d[0], xx + d[1]], order=1, mode="constant",
                                  cval=float(img.max()))
    diff = np.abs(v - ref).max()
    print("pixels %dx%d: %.3g" % (h, w, diff))
    assert diff <= 1e-12
    assert out.dtype == np.uint8 and np.array_equal(out, np.floor(v + 0.5))


def test_abi_refuses_before_the_device(native):
    lib = native.lib
    assert lib.ta_line_distort_workspace_bytes(2, 100) == 24 * 2 + 32 * 100
    assert lib.ta_line_distort_workspace_bytes(-1, 100) == -1 and lib.ta_line_distort_workspace_bytes(1, -1) == -1
    hh, ww = (ctypes.c_int32 * 1)(60), (ctypes.c_int32 * 1)(100)
    p = ctypes.addressof(hh)                    # any non-null address: nothing is dereferenced on the device before the checks

    def call(n=1, distort=3.0, dsigma=10.0, pix=p, hh_host=hh, ww_host=ww, ws_bytes=1 << 30, out=p, fields=None):
        return lib.ta_line_distort(pix, p, p, p, p, n, ctypes.addressof(hh_host) if hh_host is not None else None,
                                   ctypes.addressof(ww_host) if ww_host is not None else None, distort, dsigma, 7,
                                   p, p, ws_bytes, out, fields, None)
    assert call(pix=None) == native.TA_EINVAL and b"null" in lib.ta_last_error()
    assert call(out=None) == native.TA_EINVAL and b"null" in lib.ta_last_error()
    assert call(hh_host=None) == native.TA_EINVAL
    assert call(n=-1) == native.TA_EINVAL
    assert call(distort=0.0) == native.TA_EINVAL and call(distort=-1.0) == native.TA_EINVAL
    assert call(distort=float("nan")) == native.TA_EINVAL
    assert call(dsigma=0.0) == native.TA_EINVAL and call(dsigma=-2.0) == native.TA_EINVAL
    assert call(dsigma=512.2) == native.TA_ELIMIT                  # radius 2049: 2048 is the last one taken
    assert call(dsigma=1e300) == native.TA_ELIMIT
    assert call(hh_host=(ctypes.c_int32 * 1)(513)) == native.TA_ELIMIT
    assert call(hh_host=(ctypes.c_int32 * 1)(0)) == native.TA_EINVAL
    assert call(ws_bytes=24 + 32 * 6000 - 1) == native.TA_EINVAL and b"workspace" in lib.ta_last_error()
    assert call(n=0) == native.TA_OK
    with pytest.raises(ValueError):
        native.check(call(distort=0.0), "ta_line_distort")


def test_python_refuses_before_the_device():
    from text_alignment_amd import augment
    strip = np.full((20, 30), 255, np.uint8)
    assert augment.distort_strips([]) == []
    assert augment.distort_strips([], want_fields=True) == ([], [])
    for kw in ({"distort": 0}, {"distort": -1.0}, {"dsigma": 0}, {"dsigma": -3}, {"dsigma": 600.0}, {"seed": -1},
               {"first_counter": 2 ** 64}, {"distort": float("nan")}):
        with pytest.raises(ValueError):
            augment.distort_strips([strip], **kw)
    with pytest.raises(ValueError):
        augment.distort_strips([np.zeros((513, 4), np.uint8)])
    with pytest.raises(ValueError):
        augment.distort_strips([np.zeros((0, 4), np.uint8)])
    with pytest.raises(TypeError):
        augment.distort_strips([strip.astype(np.float32)])
    with pytest.raises(TypeError):
        augment.distort_strips([strip.reshape(-1)])


def test_trainer_refuses_before_the_device():
    from text_alignment_amd import train
    with pytest.raises(ValueError):
        train.LineTrainer(charset="ab", distort=0)
    with pytest.raises(ValueError):
        train.LineTrainer(charset="ab", distort=3.0, dsigma=0.0)
    with pytest.raises(ValueError):
        train.LineTrainer(charset="ab", distort=3.0, dsigma=1000.0)
    tr = train.LineTrainer(charset="ab", distort=3.0)
    assert tr.distort == 3.0 and tr.dsigma == 10.0 and tr.lines_seen == 0
    with pytest.raises(ValueError, match="raw uint8 strips"):
        tr.train([np.zeros((40, 48))], ["ab"])
    with pytest.raises(ValueError, match="raw uint8 strips"):
        tr.train([np.full((30, 90), 255, np.uint8), np.zeros((40, 48))], ["ab", "ab"])
    assert tr.W is None and tr.lines_seen == 0                       # nothing reached the device
    plain = train.LineTrainer(charset="ab")
    assert plain.distort is None
