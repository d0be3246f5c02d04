"""nw_lcs_suffix_kernel's store schedule at its edges (csrc/ta_nw2.hip; the runs of csrc/nw_band.h: lcs_next_run): one
batch under the LCS-bounded funnel holding the smallest problems at which the schedule can go wrong -- the four phases
of n mod 4, a last strip of a single row (n = 256 k + 1: its lanes above 0 have no row), m at and just past a multiple
of 64 (where a strip's counts cross from one lane's word into the next, the upper lanes idle), m > n and n > m.  The
table against numpy bit for bit, the certificate's words against the CPU replay, the alignments against the oracle.
Every case must be one the LCS kernel covers (flag word 2): a declined problem would check nothing.
(The plan's last strip always reaches the last group, so it has no right edge: its lanes without a row matter to the
row stores and to column 0 here; a right edge that starts below such lanes is the CPU sweep's, tests/test_nw_lcs_runs.py.)"""
import numpy as np
import pytest

from test_nw_band_gpu import _assert_oracle, _batch, _pair
from test_nw_funnel_lcs_gpu import _suffix_lcs_rows
from test_nw_funnel_lcs_sim import lcs_words, load_sim, replay
from tools.nw_configs import DEFAULT_SYS

pytestmark = pytest.mark.gpu

W = 600
# (n, m): n = 1024 .. 1027 are the four phases; 1025 and 769 leave a last strip of one row; m = 1024, 1025, 1087 put
# the right edge's columns at, just past and 63 past a word's end; 769 x 1025 and 1024 x 1087 have m > n, 1027 x 1024
# and 1026 x 900 n > m
SHAPES = [(1024, 1024), (1025, 1025), (1026, 1087), (1027, 1024), (769, 1025), (1024, 1087), (1026, 900)]
PROBS = [_pair(n, m, 70 + k) for k, (n, m) in enumerate(SHAPES)]
SYSTEMS = [DEFAULT_SYS] * len(PROBS)


@pytest.fixture(scope="module")
def run():
    import torch
    batch = _batch(PROBS, DEFAULT_SYS, W, band_shape="funnel-lcs")
    batch.run()
    torch.cuda.synchronize()
    plan = batch.band_plan()
    sim = load_sim()
    return {"res": batch.results(), "fb": batch.band_fallbacks(), "cert": batch.band_certificate(),
            "flag": plan["cert_dev"].cpu().numpy().reshape(-1, 4)[:, 3].tolist(),
            "table": plan["lcs_dev"].cpu().numpy(), "plan": plan,
            "replay": [replay(sim, t, o, DEFAULT_SYS, W) for t, o in PROBS]}


def test_every_case_is_covered(run):
    assert run["plan"]["shape"] == "funnel" and run["plan"]["lcs"] and run["plan"]["w"] == W
    assert [r["flag"] for r in run["replay"]] == [2] * len(PROBS)
    assert run["flag"] == [2] * len(PROBS)
    # and every kind of strip occurs: with a right edge, without one, and a last strip of one row
    ngroups = [(m + 63 + 3) // 4 for n, m in SHAPES]
    ghs = [[int(gh) for gl, gh in r["ranges"]] for r in run["replay"]]
    assert any(gh < ng for g, ng in zip(ghs, ngroups) for gh in g) and any(gh >= ng for g, ng in zip(ghs, ngroups) for gh in g)


def test_table_equals_numpy_bit_for_bit(run):
    max_n = max(n for n, m in SHAPES)
    stride = lcs_words(max_n)
    row_off = (max_n + 1 + 63) & ~63
    assert run["table"].size >= stride * len(PROBS)
    for k, (t, o) in enumerate(PROBS):
        n, m = len(t), len(o)
        ranges = run["replay"][k]["ranges"]
        tab = run["table"][k * stride:(k + 1) * stride]
        L = _suffix_lcs_rows(t, o, set(range(0, n, 4)))
        ngroups = (m + 63 + 3) // 4
        for s in range((n + 255) // 256):
            grow = (L[256 * s][:-1] - L[256 * s][1:])[::-1]                 # reversed column c = m - j, bit c - 1
            bits = np.zeros(64 * 64, dtype=np.uint8)
            bits[:m] = grow
            words = np.packbits(bits.reshape(64, 64), axis=1, bitorder="little").view(np.uint64).reshape(64)
            got = tab[row_off + 192 * s: row_off + 192 * s + 128].view(np.uint64)
            assert (got == words).all(), (k, s)
            pref = np.concatenate([[0], np.cumsum(bits.reshape(64, 64).sum(axis=1))[:-1]])
            assert (tab[row_off + 192 * s + 128: row_off + 192 * s + 192] == pref).all(), (k, s)
            gh = int(ranges[s][1])
            want = [int(L[256 * s + 4 * l][4 * gh - l]) if gh < ngroups and 256 * s + 4 * l < n and 4 * gh - l <= m else 0
                    for l in range(64)]
            assert tab[64 * s: 64 * s + 64].tolist() == want, (k, s)


def test_certificates_equal_the_replay(run):
    for k, r in enumerate(run["replay"]):
        print("problem", k, SHAPES[k], "v0", r["v0"], "exit", r["exit"], "count", r["count"], "gpu", run["cert"][k].tolist())
        assert r["table_ok"] and r["exit"] == r["scan"]
        assert run["cert"][k].tolist() == [r["v0"], r["exit"], r["count"]], (k, run["cert"][k].tolist(), r["v0"], r["exit"])
        assert (k in run["fb"]) == (not r["ok"])


def test_alignments_are_the_oracles(run):
    _assert_oracle(PROBS, SYSTEMS, run["res"])
