"""nw_lcs_suffix_kernel's two-level match masks on the GPU (csrc/ta_nw2.hip; layout in csrc/nw_band.h): at alphabets on
both sides of a multiple of 8, with one row of A, with all eight and with the largest the kernel takes, the table it
leaves equals a numpy LCS bit for bit -- the rows 256 s and the right edge's counts -- every alignment is the oracle's and
no related pair falls back; one symbol past the largest alphabet the kernel declines and the static funnel runs."""
import numpy as np
import pytest

from test_nw_band_gpu import _assert_oracle, _batch
from test_nw_funnel_lcs_gpu import _suffix_lcs_rows
from test_nw_funnel_lcs_sim import lcs_words, load_sim, replay
from tools.nw_configs import DEFAULT_SYS

pytestmark = pytest.mark.gpu

W = 600
ALPHABETS = [2, 8, 9, 17, 27, 57, 64]
SHAPES = [(1024, 1100), (1280, 1024)]          # the smallest that band (tests/test_nw_funnel_lcs_gpu.py)


def _related_pair(n, m, alphabet, seed):
    """o is t under about 10 % substitutions, 2 % deletions and 2 % insertions, cut or filled up to m symbols; the
    alphabet's last code stands in both, so that the batch's alphabet hint is `alphabet`"""
    rng = np.random.default_rng(1000 * alphabet + seed)
    t = rng.integers(0, alphabet, size=n)
    u = rng.random(size=(n, 2))
    s = rng.integers(0, alphabet, size=(n, 2))
    o = []
    for k in range(n):
        if u[k, 0] >= 0.02:
            o.append(int(s[k, 0]) if u[k, 0] < 0.12 else int(t[k]))
        if u[k, 1] < 0.02:
            o.append(int(s[k, 1]))
    o = (o + [int(x) for x in rng.integers(0, alphabet, size=m)])[:m]
    t, o = np.asarray(t, dtype=np.int32), np.asarray(o, dtype=np.int32)
    t[n // 2] = o[m // 3] = alphabet - 1
    return t, o


def _probs(alphabet):
    return [_related_pair(n, m, alphabet, k) for k, (n, m) in enumerate(SHAPES)]


def _run(alphabet):
    import torch
    probs = _probs(alphabet)
    assert max(int(max(t.max(), o.max())) for t, o in probs) == alphabet - 1
    batch = _batch(probs, DEFAULT_SYS, W, band_shape="funnel-lcs")
    batch.run()
    torch.cuda.synchronize()
    plan = batch.band_plan()
    assert plan["w"] == W and plan["shape"] == "funnel", "no band planned at alphabet %d" % alphabet
    return probs, batch, plan, plan["cert_dev"].cpu().numpy().reshape(-1, 4)[:, 3].tolist()


@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_table_and_alignments(alphabet):
    probs, batch, plan, flag = _run(alphabet)
    assert plan["shape"] == "funnel" and plan["lcs"]
    assert flag == [2, 2]
    table = plan["lcs_dev"].cpu().numpy()
    max_n = max(len(t) for t, o in probs)
    stride = lcs_words(max_n)
    row_off = (max_n + 1 + 63) & ~63
    assert table.size >= stride * len(probs)
    sim = load_sim()
    for k, (t, o) in enumerate(probs):
        n, m = len(t), len(o)
        nstrips, ngroups = (n + 255) // 256, (m + 63 + 3) // 4
        ranges = replay(sim, t, o, DEFAULT_SYS, W, alphabet=alphabet)["ranges"]
        tab = table[k * stride:(k + 1) * stride]
        L = _suffix_lcs_rows(t, o, set(range(0, n, 4)))
        for s in range(nstrips):
            # the whole row 256 s: growth bits and the counts of the words before
            grow = (L[256 * s][:-1] - L[256 * s][1:])[::-1]                 # reversed column c = m - j, bit c - 1
            bits = np.zeros(64 * 64, dtype=np.uint8)
            bits[:m] = grow
            words = np.packbits(bits.reshape(64, 64), axis=1, bitorder="little").view(np.uint64).reshape(64)
            got = tab[row_off + 192 * s: row_off + 192 * s + 128].view(np.uint64)
            assert (got == words).all(), (alphabet, k, s)
            pref = np.concatenate([[0], np.cumsum(bits.reshape(64, 64).sum(axis=1))[:-1]])
            assert (tab[row_off + 192 * s + 128: row_off + 192 * s + 192] == pref).all(), (alphabet, k, s)
            # the right edge's count per lane
            gh = int(ranges[s][1])
            for l in range(64):
                row0, jr = 256 * s + 4 * l, 4 * gh - l
                want = int(L[row0][jr]) if gh < ngroups and row0 < n and jr <= m else 0
                assert tab[64 * s + l] == want, (alphabet, k, s, l)
    _assert_oracle(probs, [DEFAULT_SYS] * len(probs), batch.results())
    assert batch.band_fallbacks() == []


def test_one_symbol_past_the_largest_alphabet_is_declined():
    """alphabet 65: no table, flag word 1, the static funnel's region; the alignments are the oracle's all the same"""
    probs, batch, plan, flag = _run(65)
    assert plan["shape"] == "funnel" and not plan["lcs"]
    assert flag == [1, 1]
    _assert_oracle(probs, [DEFAULT_SYS] * len(probs), batch.results())
    assert batch.band_fallbacks() == []
