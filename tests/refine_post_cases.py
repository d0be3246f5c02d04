"""The cases of ta_posterior_pages that tests/test_posterior_pages_sim.py (the host build of csrc/ta_refine_conf.hip) and
tests/test_posterior_pages_gpu.py (the real kernel) share, the layout both drive it with, and the checker's answers.

The pages are tests/refine_conf_cases.py's, with pairs in place of integers: `pack` is that module's (a small good page
in FRONT, no offset at 0, gaps between the slots' labels, two slots behind count[0] whose arrays are poison), every
label of a slot then gets a mass (own_m in [0.5, 1) or zero, own_x) and every slot its line's (z_m, z_x) -- seeded, or
the line's own "pairs" = [(m, x), ...] and "z" = (m, x).  Every output is poisoned; the float64 outputs carry the
poison's bit pattern and are compared through their int64 view.
"""
import numpy as np

import refine_conf_cases as PC
import refine_post_ref as R
from text_alignment_amd import _abi

POISON32, POISON64 = PC.POISON32, PC.POISON64
NAN = R.NO_POSTERIOR_BITS


def bind(lib):
    return _abi.bind(lib, ["ta_posterior_pages"])


def line(refined, tf, pairs, z, **more):
    """a line whose masses and whose line's mass are given"""
    ln = PC.line(refined, tf, len(pairs), **more)
    ln.update(pairs=pairs, z=z)
    return ln


def cases():
    out = list(PC.cases())
    h = 0.5
    out += [
        # characters 0 - 3 on one refined line, 4 - 6 on another whose Z is 2^40 times smaller: the syllable 2 .. 5 takes
        # the smallest QUOTIENT (0.125 of the second line), not the smallest mass
        ("a syllable across two refined lines with different z",
         [dict(n=8, lines=[line(True, 0, [(h, -10), (h, -11), (h, -10), (h, -11)], (h, -10)),
                           line(True, 4, [(h, -50), (h, -53), (h, -51)], (h, -50))], syls=[(0, 1), (2, 5), (6, 7), (7, 7)])]),
        ("zero masses", [dict(n=6, lines=[line(True, 0, [(0.0, 0), (h, -7), (0.0, 0)], (0.75, -5)),
                                          line(True, 3, [(0.0, 0)], (h, -2000))], syls=[(0, 0), (0, 2), (1, 1), (3, 5), (4, 5)])]),
    ]
    return out


# the device's division and ldexp against numpy's: own = z (exactly 1.0), a zero mass, quotients that round, and exponent
# differences down through the subnormal range to where the result is zero
OWN_M = (0.7, 0.5000000000000001, 0.5, 0.9, 0.9999999999999999, 0.75)
Z_M = (0.9, 0.9999999999999999, 0.5, 0.7, 0.5000000000000001)
DIFFS = (1, 0, -1, -60, -1021, -1022, -1023, -1050, -1074, -1075, -1076, -2000)


def division_pages():
    """a page per z_m whose one refined line holds own = z, a zero mass, then every own_m at every exponent difference;
    every character a syllable of its own, and one syllable over all of them"""
    pages = []
    for zm in Z_M:
        zx = -700
        pairs = [(zm, zx), (0.0, 0)] + [(m, zx + d) for d in DIFFS for m in OWN_M]
        n = len(pairs)
        pages.append(dict(n=n, lines=[line(True, 0, pairs, (zm, zx))], syls=[(i, i) for i in range(n)] + [(0, n - 1)]))
    return pages


def check_division(pk, pages, posterior_values):
    """the outputs of a call on pack(division_pages()) against posterior_values(m, x, z_m, z_x) on the host (the rule of
    forced.posterior_values), word for word; each figure is printed before it is asserted"""
    assert pk.status[:pk.nprob].tolist() == [0] * pk.nprob
    seen = set()
    for p, pg in enumerate(pages, start=1):              # page 0 is the front page
        pairs = pg["lines"][0]["pairs"]
        k = int(pk.slot[int(pk.line_first[p])])
        assert (pk.z_m[k], pk.z_x[k]) == pg["lines"][0]["z"]
        with np.errstate(all="ignore"):                  # (numpy reports the results that leave the normal range)
            want = posterior_values([m for m, _ in pairs], [x for _, x in pairs], pk.z_m[k], pk.z_x[k])
        a, s = int(pk.t_off[p]), int(pk.syl_off[p])
        got = np.ascontiguousarray(pk.char_post[a:a + len(pairs)])
        off = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
        print("z_m %r: %d of %d words differ" % (float(pk.z_m[k]), len(off), len(pairs)))
        assert len(off) == 0, [(pairs[i], float(got[i]).hex(), float(want[i]).hex()) for i in off]
        assert got[0] == 1.0 and got[1] == 0.0 and not np.signbit(got[1])
        per_syl = np.ascontiguousarray(pk.syl_post[s:s + len(pairs)])
        assert np.array_equal(per_syl.view(np.int64), want.view(np.int64))
        assert pk.syl_post[s + len(pairs)] == 0.0 and not np.signbit(pk.syl_post[s + len(pairs)])
        seen |= {("zero" if v == 0 else "subnormal" if v < 2.0 ** -1022 else "normal") for v in want[2:]}
    assert seen == {"zero", "subnormal", "normal"}
    compare(pk)


def pack(pages, seed=0, count=None):
    """host arrays of one call, the front page first.  count: the device's count[0] if not the number of slots"""
    pk = PC.pack(pages, seed=seed, count=count)
    rng = np.random.default_rng(seed + 1000)
    del pk.confidence, pk.char_conf, pk.syl_conf
    pk.own_m = np.full(pk.label_cap, POISON64, np.int64).view(np.float64)
    pk.own_x = np.full(pk.label_cap, POISON32, np.int32)
    pk.z_m = np.full(pk.nslots, POISON64, np.int64).view(np.float64)
    pk.z_x = np.full(pk.nslots, POISON32, np.int32)
    k = 0
    for pg in pk.pages:
        for ln in pg["lines"]:
            if not ln["slot"]:
                continue
            L, off = ln["L"], int(pk.lab_off[k])
            zm, zx = ln.get("z") or (0.5 + rng.random() / 2, int(rng.integers(-3000, -5)))
            pairs = ln.get("pairs")
            if pairs is None:                             # masses at and below the line's, a few of them zero
                pairs = [(0.0, 0) if rng.random() < 0.1 else (0.5 + rng.random() / 2, zx - int(rng.integers(0, 60)))
                         for _ in range(L)]
            pk.z_m[k], pk.z_x[k] = zm, zx
            pk.own_m[off:off + L] = [m for m, _ in pairs]
            pk.own_x[off:off + L] = [x for _, x in pairs]
            k += 1
    pk.char_post = np.full(pk.t_len, POISON64, np.int64).view(np.float64)
    pk.syl_post = np.full(pk.nsyl, POISON64, np.int64).view(np.float64)
    return pk


INPUTS = ("own_m", "own_x", "z_m", "z_x", "lab_off", "L", "count", "c_status", "table", "line_first", "refined", "slot", "t_off",
          "syl_first", "syl_last", "syl_off")
OUTPUTS = ("char_post", "syl_post", "status")


def call(lib, pk, ptr, stream=None, **over):
    """ta_posterior_pages on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to replace"""
    a = dict(nslots=pk.nslots, label_cap=pk.label_cap, nlines=pk.nlines, t_len=pk.t_len, nsyl=pk.nsyl, nprob=pk.nprob)
    for name in INPUTS + OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    return lib.ta_posterior_pages(a["own_m"], a["own_x"], a["z_m"], a["z_x"], a["lab_off"], a["L"], a["count"], a["c_status"],
                                  a["nslots"], a["label_cap"], a["table"], a["line_first"], a["refined"], a["slot"], a["nlines"],
                                  a["t_off"], a["t_len"], a["syl_first"], a["syl_last"], a["syl_off"], a["nsyl"], a["nprob"],
                                  a["char_post"], a["syl_post"], a["status"], stream)


def want(pk):
    """the checker's answer for a packed chunk, page by page: [(status, char_post, syl_post)]"""
    filled = max(0, min(int(pk.count[0]), pk.nslots))
    slots = [(int(pk.L[k]), int(pk.lab_off[k]), int(pk.c_status[k])) for k in range(pk.nslots)]
    out = []
    for p, pg in enumerate(pk.pages):
        a, b = int(pk.syl_off[p]), int(pk.syl_off[p + 1])
        out.append(R.posterior_page(pg["n"], int(pk.line_first[p]), int(pk.line_first[p + 1]), pk.table.tolist(),
                                    pk.refined.tolist(), pk.slot.tolist(), slots, filled, pk.own_m, pk.own_x, pk.z_m, pk.z_x,
                                    pk.label_cap, pk.syl_first[a:b].tolist(), pk.syl_last[a:b].tolist()))
    return out


def compare(pk, answer=None, skip=()):
    """every output word against the checker, bit for bit; a refused page's words, the words of the pages in `skip` and
    everything outside the pages must still be poison"""
    answer = answer or want(pk)
    cp, sp = np.full(pk.t_len, POISON64, np.int64), np.full(pk.nsyl, POISON64, np.int64)
    st = np.full(pk.nprob + 1, POISON32, np.int32)
    for p, (status, c, s) in enumerate(answer):
        if p in skip:
            continue
        st[p] = status
        if status == R.OK:
            cp[pk.t_off[p]:pk.t_off[p + 1]] = c.view(np.int64)
            sp[pk.syl_off[p]:pk.syl_off[p + 1]] = s.view(np.int64)
    for p in skip:
        st[p] = pk.status[p]                               # the caller checks these
    assert pk.status.tolist() == st.tolist()
    assert np.array_equal(np.ascontiguousarray(pk.char_post).view(np.int64), cp)
    assert np.array_equal(np.ascontiguousarray(pk.syl_post).view(np.int64), sp)
