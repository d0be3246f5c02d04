"""The funnel fill of the two-phase aligner on the GPU (csrc/ta_nw2.hip BAND = 3, csrc/nw_band.h): whatever the region
and whether or not a problem's certificate passes, the alignment is the oracle's; the certificate's three words per
problem and the list of problems filled again in full are exactly the CPU replay's (tests/native/sim_nw_funnel.cpp)."""
import numpy as np
import pytest

from test_nw_band_gpu import _assert_oracle, _batch, _oracle, _pair, _random_pair, _shifted_pair
from test_nw_funnel_sim import _inside, load_sim, replay
from tools.nw_configs import DEFAULT_SYS

pytestmark = pytest.mark.gpu

OTHER = [10, -5, -7, -7, -2, -2]


@pytest.fixture(scope="module")
def sim():
    return load_sim()


def _run(probs, system, band, shape):
    import torch
    batch = _batch(probs, system, band, band_shape=shape)
    batch.run()
    torch.cuda.synchronize()
    return batch, batch.results(), batch.band_fallbacks()


def _against_replay(sim, batch, probs, systems, w, fb):
    """certificate words and fallback list, bit for bit; returns the replay's outcomes"""
    cert = batch.band_certificate()
    assert cert is not None and cert.shape == (len(probs), 3)
    outs = []
    for k, (t, o) in enumerate(probs):
        r = replay(sim, t, o, systems[k], w, 2064)
        print("problem", k, "v0", r["v0"], "exit", r["exit"], "u", r["u"], "count", r["count"], "gpu", cert[k].tolist())
        assert cert[k].tolist() == [r["v0"], r["exit"], r["count"]], (k, cert[k].tolist(), r)
        assert batch.band_plan()["u"][k] == r["u"] and batch.band_plan()["x0"][k] == r["exit0"]
        outs.append(r)
    assert fb == [k for k, r in enumerate(outs) if not r["ok"]]
    return outs


def test_funnel_in_a_forced_band_equals_the_replay(sim):
    probs = [_pair(1100, 1100, 11), _pair(1300, 900, 12)]
    batch, res, fb = _run(probs, DEFAULT_SYS, 600, "funnel")
    plan = batch.band_plan()
    assert plan["w"] == 600 and plan["shape"] == "funnel" and plan["share"] < plan["uniform_share"]
    assert any(gl > 0 for gl, gh in plan["ranges"]) and any(gh < plan["ranges"][-1][1] for gl, gh in plan["ranges"])
    _assert_oracle(probs, [DEFAULT_SYS] * 2, res)
    outs = _against_replay(sim, batch, probs, [DEFAULT_SYS] * 2, 600, fb)
    assert fb == [] and all(r["funnel"] for r in outs)


@pytest.mark.parametrize("k", [186, 420])
def test_path_that_leaves_the_region_falls_back(sim, k):
    t, o = _shifted_pair(k)
    batch, res, fb = _run([(t, o)], DEFAULT_SYS, 600, "funnel")
    _assert_oracle([(t, o)], [DEFAULT_SYS], res)
    outs = _against_replay(sim, batch, [(t, o)], [DEFAULT_SYS], 600, fb)
    leaves = not _inside(_oracle(t, o, DEFAULT_SYS), outs[0]["ranges"], len(o))
    if leaves:
        assert fb == [0]
    if k == 420:
        assert leaves            # inside the outer band (420 < 600), outside the funnel


def test_mixed_batch_a_system_per_problem(sim):
    probs = [_pair(1100, 1100, 11), _random_pair(1100, 1100, 5), _pair(1300, 900, 12), _pair(1100, 1100, 21),
             _random_pair(1200, 1000, 6), _pair(1024, 1153, 22), _pair(1100, 1100, 11), _pair(900, 1300, 13)]
    # the last two: systems under which the funnel is declined and the band's own ranges run under its certificate
    systems = [DEFAULT_SYS, DEFAULT_SYS, OTHER, OTHER, OTHER, DEFAULT_SYS, [4, -4, 0, 0, 1, 1], [0, -8, -1, -1, -1, -1]]
    batch, res, fb = _run(probs, np.array(systems), 600, "funnel")
    assert batch.params_stride == 6 and batch.band_plan()["shape"] == "funnel"
    _assert_oracle(probs, systems, res)
    outs = _against_replay(sim, batch, probs, systems, 600, fb)
    assert [r["funnel"] for r in outs] == [True] * 6 + [False] * 2
    # declined problems that certify, the first in a region cut on both sides: phase 2 walks the band's ranges
    assert outs[6]["ok"] and outs[7]["ok"] and outs[6]["ranges"][-1][0] > 0 and outs[6]["ranges"][0][1] < 291
    assert 0 < len(fb) < len(probs), fb
    # fill and traceback as two calls: certificate and fallback belong to the fill half
    batch.run(fill=True, traceback=False)
    batch.run(fill=False, traceback=True)
    _assert_oracle(probs, systems, batch.results())
    assert batch.band_fallbacks() == fb


def test_automatic_funnel_on_a_large_problem():
    probs = [_pair(3000, 3000, 31), _random_pair(3000, 3000, 32)]
    batch, res, fb = _run(probs, DEFAULT_SYS, 0, "auto")
    plan = batch.band_plan()
    assert plan["w"] == plan["rule_w"] > 0 and plan["shape"] == "funnel" and plan["funnel_own_ranges"]
    print("share", plan["share"], "uniform", plan["uniform_share"])
    assert plan["share"] < plan["uniform_share"] < 0.8
    _assert_oracle(probs, [DEFAULT_SYS] * 2, res)
    assert fb == [1]
    cert = batch.band_certificate()
    assert cert[0, 2] == cert[1, 2] == 12 and cert[0, 0] > cert[0, 1] and cert[0, 0] > plan["u"][0]
    assert not (cert[1, 0] > cert[1, 1] and cert[1, 0] > plan["u"][1])


def test_uniform_shape_is_the_uniform_band():
    """band_shape = "uniform" under the rule launches exactly what a forced width launches -- the uniform band's
    kernel and its in-kernel certificate: same workspace, byte for byte, same list"""
    import torch
    probs = [_pair(3000, 3000, 31), _random_pair(3000, 3000, 32)]
    uni = _batch(probs, DEFAULT_SYS, 0, band_shape="uniform")
    w = uni.band_plan()["w"]
    assert w == uni.band_plan()["rule_w"] > 0 and uni.band_plan()["shape"] == "uniform"
    forced = _batch(probs, DEFAULT_SYS, w)
    assert forced.band_plan()["shape"] == "uniform" and forced.band_plan()["ranges"] == uni.band_plan()["ranges"]
    assert forced.band_plan()["share"] == uni.band_plan()["share"]
    for b in (uni, forced):
        b.ws.zero_()
        b.run()
    torch.cuda.synchronize()
    assert torch.equal(uni.ws, forced.ws)
    assert uni.band_fallbacks() == forced.band_fallbacks() == [1] and uni.band_certificate() is None
    _assert_oracle(probs, [DEFAULT_SYS] * 2, uni.results())
