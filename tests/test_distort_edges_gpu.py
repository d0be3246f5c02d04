"""Line distortion on the GPU at the edges of its kernels' paths (csrc/ta_distort.hip): the cases
of tests/distort_cases.py -- every column tile from 64 columns down to one, LDS arrays filled to their last element, two
and three row tiles, the column kernel's second sweep, radius 0 .. 2048, a key and counters with high words, strips
whose maximum is not 255 -- through augment.distort_strips, one call per (sigma, distort), against the numpy checker
tests/distort_ref.py by distort_cases.check_case, the comparison tests/test_distort_sim.py makes of the host build.
Every launch runs once."""
import numpy as np
import pytest
import torch

import distort_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batched():
    """{name: (out, fields)} on the host, from ONE call per (sigma, distort) holding all of that pair's cases.  The
    sigma-10 call is the mixed batch: a 512-row strip sets the row grid, a 4700-column one the tile count, and the
    other seventeen lines' workgroups idle through the barriers beyond their own rows and tiles."""
    from text_alignment_amd import augment
    res = {}
    for (sigma, distort), names in C.groups():
        strips = [C.case(n).strip for n in names]
        out, fields = augment.distort_strips(strips, distort, sigma, seed=C.SEED, first_counter=C.FIRST, want_fields=True)
        assert all(o.buffer is out[0].buffer for o in out)
        for n, o, f in zip(names, out, fields):
            res[n] = (o.tensor().cpu().numpy(), f.cpu().numpy())
    return res


def test_the_sigma_10_call_is_the_mixed_batch():
    (key, names), = [g for g in C.groups() if g[0] == (10.0, 3.0)]
    shapes = [C.case(n).strip.shape for n in names]
    assert (512, 9) in shapes and (2, 4700) in shapes and (1, 1) in shapes and len(names) >= 19
    assert [C.case(n).counter for n in names] == [C.FIRST + k for k in range(len(names))]


@pytest.mark.parametrize("name", [name for name, _, _, _ in C.cases()])
def test_kernels_equal_the_checker(batched, name):
    C.check_case(name, *batched[name])


def test_largest_field_error(batched):
    worst = max(float(np.abs(batched[n][1] - C.want(n).d).max()) / d for n, _, _, d in C.cases())
    print("GPU: max |D - D_ref| over all cases = %.3g x distort" % worst)
    assert worst <= C.FIELD_BOUND


def test_a_strip_alone_equals_its_batch(batched):
    """a line's result is its own: distorted alone, with its own counter -- its own grids, no idle workgroups -- every
    strip gives the pixels and fields it gave in its batch, bit for bit"""
    from text_alignment_amd import augment
    for name, strip, sigma, distort in C.cases():
        out, fields = augment.distort_strips([strip], distort, sigma, seed=C.SEED, first_counter=C.case(name).counter,
                                             want_fields=True)
        assert out[0].tensor().cpu().numpy().tobytes() == batched[name][0].tobytes(), name
        assert fields[0].cpu().numpy().tobytes() == batched[name][1].tobytes(), name


@pytest.mark.parametrize("key", [(10.0, 3.0), (512.0, 0.75)])
def test_nothing_is_written_beyond_the_last_strip(batched, native, key):
    """the C entry with buffers larger than it owes: 64 poisoned bytes after `out` and after `fields` stay as they were,
    and what lies before them is the batch's result.  (10, 3): the mixed batch; (512, 0.75): its last strip is the one
    the column kernel sweeps twice."""
    from text_alignment_amd import lineest_gpu
    (_, names), = [g for g in C.groups() if g[0] == key]
    cs = [C.case(n) for n in names]
    sigma, distort = key
    hh = np.asarray([c.strip.shape[0] for c in cs], np.int32)
    ww = np.asarray([c.strip.shape[1] for c in cs], np.int32)
    pix_off = np.concatenate([[0], np.cumsum(hh.astype(np.int64) * ww)]).astype(np.int64)
    total, n = int(pix_off[-1]), len(cs)
    gw, _ = lineest_gpu._gauss_weights(sigma)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (
        np.concatenate([c.strip.reshape(-1) for c in cs]), pix_off[:-1], hh, ww,
        np.asarray([c.counter for c in cs], np.uint64).view(np.int64), np.asarray(gw, np.float64))]
    lib = native.lib
    ws_bytes = int(lib.ta_line_distort_workspace_bytes(n, total))
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    fields = torch.full((2 * total + 8,), float("nan"), dtype=torch.float64, device="cuda")
    native.check(lib.ta_line_distort(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                                     dev[4].data_ptr(), n, hh.ctypes.data, ww.ctypes.data, distort, sigma, C.SEED,
                                     dev[5].data_ptr(), ws.data_ptr(), ws_bytes, out.data_ptr(), fields.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "ta_line_distort")
    torch.cuda.synchronize()
    out, fields = out.cpu().numpy(), fields.cpu().numpy()
    assert (out[total:] == 0xA5).all() and np.isnan(fields[2 * total:]).all()
    assert out[:total].tobytes() == np.concatenate([batched[c.name][0].reshape(-1) for c in cs]).tobytes()
    assert fields[:2 * total].tobytes() == np.concatenate([batched[c.name][1].reshape(-1) for c in cs]).tobytes()


def test_trainer_meets_a_wide_line():
    """a line of 2400 columns -- a second row tile, 38 column tiles -- beside one of 600: the trainer with distort set
    has, after one train() call, the weights of a plain trainer fed augment.distort_strips of the same lines"""
    import lineest_cases
    from text_alignment_amd import augment, train
    rng = np.random.default_rng(29)
    lines = [lineest_cases.strip(rng, 44, 600), lineest_cases.strip(rng, 40, 2400, wobble=3.0)]
    texts = ["abc", "badcabedcab"]

    def run(distort, feed=None):
        tr = train.LineTrainer(charset="abcde", seed=5, lines_per_update=2, lrate=1e-2, distort=distort)
        tr.train(lines if feed is None else feed, texts)
        assert tr.lines_seen == 2
        return [a.clone() for a in (tr.W, tr.peep, tr.W2)]
    aug = run(3.0)
    fed = run(None, augment.distort_strips(lines, 3.0, 10.0, seed=5, first_counter=0))
    plain = run(None)
    assert all(torch.equal(a, b) for a, b in zip(aug, fed))
    assert all(not torch.equal(a, b) for a, b in zip(aug, plain))
