"""The LCS-bounded funnel on the GPU (csrc/ta_nw2.hip: nw_lcs_suffix_kernel, nw_score_kernel<.., BAND = 4>;
csrc/nw_band.h): the table the LCS kernel leaves equals a numpy LCS bit for bit, the certificate's words are the CPU
replay's (tests/native/sim_nw_funnel_lcs.cpp; for problems the LCS kernel declines, sim_nw_funnel.cpp's), and whatever
the region and whether or not a problem certifies, the alignment is the oracle's, in all three traceback flows."""
import numpy as np
import pytest

from test_nw_band_gpu import _assert_oracle, _batch, _oracle, _pair, _random_pair
from test_nw_funnel_lcs_sim import lcs_words, load_sim, replay
from test_nw_funnel_sim import load_sim as load_static_sim, replay as static_replay
from tools.nw_configs import DEFAULT_SYS

pytestmark = pytest.mark.gpu

W = 600
NO_GAIN = [4, 4, -7, -7, -3, 0]        # mismatch >= match: a count of matches bounds nothing, the static funnel runs
# the smallest shapes that still band: m no multiple of 64, one with m > n, one with n > m; an unrelated pair (its
# certificate fails, the full fill runs) and a problem the LCS kernel declines (the static funnel's region and bound)
PROBS = [_pair(1024, 1100, 41), _pair(1280, 1024, 42), _pair(1537, 2049, 43), _random_pair(1100, 1100, 5),
         _pair(1100, 1100, 11)]
SYSTEMS = [DEFAULT_SYS, DEFAULT_SYS, DEFAULT_SYS, DEFAULT_SYS, NO_GAIN]


def _suffix_lcs_rows(t, o, rows):
    """{i: L(i, 0..m)} for the rows asked, L(i, j) = LCS(t[i:], o[j:]), by the plain recurrence row by row"""
    n, m = len(t), len(o)
    want, out = set(rows), {}
    prev = np.zeros(m + 1, dtype=np.int64)                     # row n
    if n in want:
        out[n] = prev.copy()
    orev = np.asarray(o)[::-1]
    for i in range(n - 1, -1, -1):
        # in reversed columns c = m - j: cur[c] = max(prev[c], prev[c-1] + eq, cur[c-1])
        p = prev[::-1]
        cand = p.copy()
        cand[1:] = np.maximum(p[1:], p[:-1] + (orev == t[i]))
        prev = np.maximum.accumulate(cand)[::-1]
        if i in want:
            out[i] = prev.copy()
    return out


@pytest.fixture(scope="module")
def run():
    import torch
    batch = _batch(PROBS, np.array(SYSTEMS), W, band_shape="funnel-lcs")
    batch.run()
    torch.cuda.synchronize()
    plan = batch.band_plan()
    return {"batch": batch, "res": batch.results(), "fb": batch.band_fallbacks(), "cert": batch.band_certificate(),
            "flag": plan["cert_dev"].cpu().numpy().reshape(-1, 4)[:, 3].tolist(),
            "table": plan["lcs_dev"].cpu().numpy(), "plan": plan}


def test_alignments_are_the_oracles(run):
    assert run["plan"]["shape"] == "funnel" and run["plan"]["lcs"]
    assert run["flag"] == [2, 2, 2, 2, 1]
    _assert_oracle(PROBS, SYSTEMS, run["res"])
    assert 3 in run["fb"] and not set(run["fb"]) & {0, 1, 2}, run["fb"]


def test_table_equals_numpy_bit_for_bit(run):
    max_n = max(len(t) for t, o in PROBS)
    stride = lcs_words(max_n)
    row_off = (max_n + 1 + 63) & ~63
    assert run["table"].size >= stride * len(PROBS)
    sim = load_sim()
    for k in range(4):
        t, o = PROBS[k]
        n, m = len(t), len(o)
        nstrips = (n + 255) // 256
        ranges = replay(sim, t, o, SYSTEMS[k], W)["ranges"]
        tab = run["table"][k * stride:(k + 1) * stride]
        L = _suffix_lcs_rows(t, o, set(range(0, n, 4)))
        ngroups = (m + 63 + 3) // 4
        for s in range(nstrips):
            # the whole row 256 s: growth bits and the counts of the words before
            grow = (L[256 * s][:-1] - L[256 * s][1:])[::-1]                 # reversed column c = m - j, bit c - 1
            bits = np.zeros(64 * 64, dtype=np.uint8)
            bits[:m] = grow
            words = np.packbits(bits.reshape(64, 64), axis=1, bitorder="little").view(np.uint64).reshape(64)
            got = tab[row_off + 192 * s: row_off + 192 * s + 128].view(np.uint64)
            assert (got == words).all(), (k, s)
            pref = np.concatenate([[0], np.cumsum(bits.reshape(64, 64).sum(axis=1))[:-1]])
            assert (tab[row_off + 192 * s + 128: row_off + 192 * s + 192] == pref).all(), (k, s)
            # the right edge's count per lane
            gh = int(ranges[s][1])
            for l in range(64):
                row0, jr = 256 * s + 4 * l, 4 * gh - l
                want = int(L[row0][jr]) if gh < ngroups and row0 < n and jr <= m else 0
                assert tab[64 * s + l] == want, (k, s, l)


def test_certificates_equal_the_replay(run):
    sim, static = load_sim(), load_static_sim()
    for k, (t, o) in enumerate(PROBS):
        if run["flag"][k] == 2:
            r = replay(sim, t, o, SYSTEMS[k], W)
        else:
            r = static_replay(static, t, o, SYSTEMS[k], W, 2064)
        print("problem", k, "v0", r["v0"], "exit", r["exit"], "count", r["count"], "gpu", run["cert"][k].tolist())
        assert run["cert"][k].tolist() == [r["v0"], r["exit"], r["count"]], (k, run["cert"][k].tolist(), r)
        assert (k in run["fb"]) == (not r["ok"])


@pytest.mark.parametrize("tb_waves", [1, 4, 3])
def test_three_traceback_flows(run, tb_waves):
    """nw_trace2_kernel, nw_trace2w_kernel, nw_trace2h_kernel on the LCS-bounded funnel's workspace (one system for the
    batch: the half-strip flow pairs problems)"""
    import torch
    probs = PROBS[:4]
    batch = _batch(probs, DEFAULT_SYS, W, band_shape="funnel-lcs", tb_waves=tb_waves)
    batch.run()
    torch.cuda.synchronize()
    _assert_oracle(probs, [DEFAULT_SYS] * 4, batch.results())
    assert batch.band_fallbacks() == [3]
    # fill and traceback as two calls: table, certificate and fallback belong to the fill half
    batch.run(fill=True, traceback=False)
    batch.run(fill=False, traceback=True)
    _assert_oracle(probs, [DEFAULT_SYS] * 4, batch.results())


def test_auto_runs_the_lcs_bounded_funnel():
    import torch
    probs = [_pair(3000, 3000, 31)]
    auto = _batch(probs, DEFAULT_SYS, 0)
    static = _batch(probs, DEFAULT_SYS, 0, band_shape="funnel")
    pa, ps = auto.band_plan(), static.band_plan()
    assert pa["shape"] == ps["shape"] == "funnel" and pa["lcs"] and not ps["lcs"]
    assert pa["share"] < ps["share"] == pa["static_share"]
    for b in (auto, static):
        b.run()
    torch.cuda.synchronize()
    _assert_oracle(probs, [DEFAULT_SYS], auto.results())
    _assert_oracle(probs, [DEFAULT_SYS], static.results())
    assert auto.band_fallbacks() == static.band_fallbacks() == []
