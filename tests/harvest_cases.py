"""Pages for the harvest tests (TEST ONLY), as host id arrays -- no recogniser needed: tests/test_harvest_gpu.py aligns
them with the GPU aligner, tests/test_harvest_sim.py with the CPU restatement of it, both hand the SAME alignment columns
to the kernel and to the checker tests/harvest_ref.py.

A page: t (transcript ids), o (OCR ids), o_line (per OCR character its line IN the page, never decreasing), lines, T (per
line), t_class.  Ids 0 .. 3 are the letters a .. d, 4 is the space; the classes are those of train.make_codec("abcd"):
space 1, letters 3 .. 6, and on pages with `drop` those of make_codec("abc"): the letter d is not in the codec (class
0)."""
import numpy as np

import harvest_ref as R

SPACE = 4
LETTERS = "abcd "
STIFF = [8, -1, -20, -20, -10, -10]      # a gap costs far more than a mismatch: max(n, m) columns, no gap over a gap
DEFAULT = [8, -4, -7, -7, -3, 0]
SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 700)
NUM, DEN = 4, 5


def _words(rng, n):
    t = rng.integers(0, 4, size=n)
    t[rng.random(n) < 0.18] = SPACE
    return t.astype(np.int32)


def _noisy(rng, t, sub, dele, ins=0.0):
    out = []
    for c in t:
        if rng.random() < ins:
            out.append(int(rng.integers(0, 5)))
        r = rng.random()
        if r < dele:
            continue
        out.append(int(rng.integers(0, 4)) if r < dele + sub else int(c))
    return np.asarray(out, dtype=np.int32)


def _split(rng, m, nl, empty=()):
    """m OCR characters over nl lines in order; the lines in `empty` get none"""
    full = [l for l in range(nl) if l not in empty]
    if not full or m == 0:
        return np.zeros(m, dtype=np.int32) + (full[0] if full else 0)
    cuts = np.sort(rng.integers(0, m + 1, size=len(full) - 1))
    bounds = np.concatenate([[0], cuts, [m]])
    o_line = np.zeros(m, dtype=np.int32)
    for k, l in enumerate(full):
        o_line[bounds[k]:bounds[k + 1]] = l
    return o_line


def _page(rng, t, o, nl, empty=(), drop=False, T=None):
    cls = np.where(t == SPACE, 1, t + 3).astype(np.int32)
    if drop:
        cls[t == 3] = 0
    T = rng.integers(3, 60, size=nl).astype(np.int32) if T is None else np.asarray(T, dtype=np.int32)
    return {"t": np.asarray(t, dtype=np.int32), "o": np.asarray(o, dtype=np.int32), "o_line": _split(rng, len(o), nl, empty),
            "lines": nl, "T": T, "t_class": cls, "charset": "abc" if drop else "abcd"}


def sized_pages():
    """under STIFF every page has exactly len(t) columns: SIZES, then the page shapes"""
    rng = np.random.default_rng(11)
    pages = []
    for k, cols in enumerate(SIZES):
        t = _words(rng, cols)
        pages.append(_page(rng, t, _noisy(rng, t, 0.1, 0.15), 1 + k % 4 if cols else 2, drop=k % 3 == 0))
    t = _words(rng, 50)
    pages.append(_page(rng, t, _noisy(rng, t, 0.05, 0.05), 1, T=[200]))                       # one line
    t = _words(rng, 90)
    pages.append(_page(rng, t, _noisy(rng, t, 0.1, 0.1), 5, empty=(2,)))                      # five lines, one without OCR
    core = _words(rng, 60)
    t = np.concatenate([[0, 1, SPACE, 2, 3, SPACE], core, [SPACE, 3, 2, SPACE, 1, 0]]).astype(np.int32)
    pages.append(_page(rng, t, core.copy(), 3, T=[100, 100, 100]))                            # seams at both page ends
    pages.append(_page(rng, _words(rng, 40), np.zeros(0, np.int32), 3))                       # only op-1 columns
    pages.append(_page(rng, np.zeros(0, np.int32), _words(rng, 30), 2))                       # only op-2 columns
    return pages


def random_pages(seed=5, count=40):
    """small pages over four letters and the space, 1 .. 6 lines: ties and seams everywhere"""
    rng = np.random.default_rng(seed)
    pages = []
    for k in range(count):
        t = _words(rng, int(rng.integers(0, 70)))
        o = _noisy(rng, t, 0.15, 0.1, 0.1)
        nl = int(rng.integers(1, 7))
        empty = tuple(int(l) for l in range(nl) if rng.random() < 0.15)
        if len(empty) == nl:
            empty = empty[1:]
        pages.append(_page(rng, t, o, nl, empty=empty, drop=k % 4 == 1))
    return pages


def assemble(pages, ops_list, unfinished=()):
    """the batch-wide arrays the kernel reads, and the pages as the checker reads them (aligned lists)"""
    line_first = np.zeros(len(pages) + 1, dtype=np.int64)
    np.cumsum([pg["lines"] for pg in pages], out=line_first[1:])
    cat = lambda key, dt: np.concatenate([pg[key] for pg in pages]).astype(dt) if pages else np.zeros(0, dt)    # noqa: E731
    o_line = np.concatenate([pg["o_line"] + int(line_first[p]) for p, pg in enumerate(pages)]).astype(np.int32)
    ref = []
    for p, (pg, ops) in enumerate(zip(pages, ops_list)):
        tra, ocr = R.aligned_from_ops(list(ops), pg["t"].tolist(), pg["o"].tolist())
        ref.append({"tra": tra, "ocr": ocr, "o_line": (pg["o_line"] + int(line_first[p])).tolist(), "lines": pg["lines"],
                    "t_class": pg["t_class"].tolist(), "unfinished": p in unfinished})
    return {"line_first": line_first, "o_line": o_line, "t_class": cat("t_class", np.int32), "T": cat("T", np.int32),
            "ref": ref}


def expected(asm, num=NUM, den=DEN):
    """(table, refused flags, (acc_line, L, lab_off, labels)) from the checker"""
    table, refused = R.harvest_batch(asm["ref"], asm["T"].tolist(), num, den)
    return table, refused, R.pack(table, asm["ref"])
