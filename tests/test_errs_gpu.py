"""Held-out scoring on the GPU (csrc/ta_errs.hip, text_alignment_amd/errs.py) against the
plain-Python checker tests/errs_ref.py: every output is an integer and is compared for equality."""
import math

import numpy as np
import pytest
import torch

import errs_ref as R

pytestmark = pytest.mark.gpu

NO = 12                                   # classes 0 .. 11: "", " ", "~" and nine letters; 12 = not in the codec
KINDS = ("exact", "nospace")
# (n, m) under "exact": n = the decoded length AFTER the filter
SHAPES = [(0, 0), (0, 5), (5, 0), (1, 1), (63, 64), (64, 64), (65, 63), (64, 129), (300, 257), (17, 600), (2500, 40),
          (33, 32)]


def _lines():
    """[(raw decoded codes, target codes)] for SHAPES, in order"""
    rng = np.random.default_rng(2024)

    def glyphs(k, lo=2, hi=NO):
        return rng.integers(lo, hi, size=k).tolist()
    out = []
    out.append(([], []))                                                        # (0, 0)
    out.append(([1, 0, 1, 1, 0], glyphs(5)))                                    # (0, 5): only spaces and class 0
    out.append((glyphs(5), []))                                                 # (5, 0)
    out.append(([7], [7]))                                                      # (1, 1)
    a = glyphs(63, 2, 5)
    out.append((a, [3] + a))                                                    # (63, 64): one leading deletion, many ties
    a = glyphs(64)
    out.append((a, list(a)))                                                    # (64, 64): identical
    out.append((glyphs(65, 2, 7), glyphs(63, 7, NO)))                           # (65, 63): no character in common
    out.append((glyphs(64, 2, 6), glyphs(129, 2, 6)))                           # (64, 129)
    # (300, 257): words with single spaces between them; the raw codes carry class 0 everywhere and leading,
    # doubled and trailing spaces; the target is a mutated copy
    words = []
    while sum(len(w) for w in words) + len(words) - 1 < 300:
        words.append(glyphs(int(rng.integers(1, 9))))
    flat = [c for w in words for c in w + [1]][:-1][:300]
    if flat[-1] == 1:
        flat[-1] = 5
    assert R.filter_decoded(flat, "exact") == flat and len(flat) == 300
    raw = [1, 0, 1]
    for c in flat:
        raw.extend([0] * int(rng.integers(0, 3)))
        raw.extend([c, 0, 1, 1] if c == 1 and rng.random() < 0.5 else [c])
    raw.extend([0, 1, 1, 0])
    tgt = [c for c in flat if rng.random() > 0.2]
    tgt = [int(rng.integers(1, NO)) if rng.random() < 0.1 else c for c in tgt]
    tgt = (tgt + glyphs(257))[:257]
    out.append((raw, tgt))
    t = glyphs(600)
    t[5] = t[300] = NO                                                          # characters outside the codec
    out.append((glyphs(17), t))                                                 # (17, 600)
    out.append((glyphs(2500, 2, 6), glyphs(40, 2, 6)))                          # (2500, 40): the longest decoded line
    g = [4, 4, 4] + glyphs(29, 2, 5)
    out.append(([4] + g, g))                                                    # (33, 32): one leading insertion, the tie order decides
    return out


class Batch(object):
    """the lines packed as the decoder leaves them: dec_off with gaps (filled with a code no line may read), dec_n with
    a trailing status word"""

    def __init__(self, lines, bound_slack=None):
        self.codes = [a for a, _ in lines]
        self.targets = [g for _, g in lines]
        off, flat = [], []
        for k, a in enumerate(self.codes):
            flat.extend([99] * (3 + k % 5))
            off.append(len(flat))
            flat.extend(a)
        flat.extend([99] * 4)
        self.T = [max(2 * len(a) - 1, 0) for a in self.codes]                   # the bound (T + 1) // 2 is tight
        self.dec_c = torch.tensor(flat, dtype=torch.int32, device="cuda")
        self.dec_off = torch.tensor(off, dtype=torch.int64, device="cuda")
        self.dec_n = torch.tensor([len(a) for a in self.codes] + [0x5a5a], dtype=torch.int32, device="cuda")


@pytest.fixture(scope="module")
def lines():
    return _lines()


@pytest.fixture(scope="module")
def batch(lines):
    return Batch(lines)


@pytest.fixture(scope="module")
def reference(lines):
    """the checker's (per_line, conf) of the whole batch under both kinds, computed once"""
    return {kind: R.score([a for a, _ in lines], [g for _, g in lines], NO + 1, kind) for kind in KINDS}


def test_kernel_equals_the_checker(batch, reference):
    from text_alignment_amd import errs
    for kind in KINDS:
        res = errs.score_decoded(batch.dec_c, batch.dec_off, batch.dec_n, batch.T, batch.targets, NO, kind)
        per, conf = reference[kind]
        print(kind, res.per_line.tolist())
        assert res.per_line.dtype == np.int32 and res.per_line.shape == (len(SHAPES), 6)
        assert np.array_equal(res.per_line, per)
        assert res.conf.dtype == torch.int64 and res.conf.is_cuda and np.array_equal(res.confusions(), conf)
        assert R.totals(per) == {"errors": res.errors, "chars": res.chars, "lines": res.lines, "cer": res.cer}
    assert [tuple(r) for r in reference["exact"][0][:, 1:3].tolist()] == SHAPES
    ex = reference["exact"][0]
    assert ex[5].tolist() == [0, 64, 64, 0, 0, 0]                               # identical
    assert ex[6].tolist() == [65, 65, 63, 63, 2, 0]                             # nothing in common
    assert ex[4].tolist() == [1, 63, 64, 0, 0, 1] and ex[11].tolist() == [1, 33, 32, 0, 1, 0]
    assert reference["nospace"][0][8, 1] < 300                                  # the spaces of the long line are gone


def test_a_line_alone_equals_the_line_in_the_batch(batch, reference):
    from text_alignment_amd import errs
    for k in (1, 7, 8, 9):
        res = errs.score_decoded(batch.dec_c, batch.dec_off[k:k + 1], batch.dec_n[k:k + 1], batch.T[k:k + 1],
                                 batch.targets[k:k + 1], NO, "exact")
        assert res.per_line[0].tolist() == reference["exact"][0][k].tolist()
        assert np.array_equal(res.confusions(), R.score_line(batch.codes[k], batch.targets[k], NO + 1, "exact")[1])


def test_two_calls_add_into_one_matrix(batch, reference):
    from text_alignment_amd import errs
    conf = torch.zeros((NO + 1, NO + 1), dtype=torch.int64, device="cuda")
    h = 6
    r1 = errs.score_decoded(batch.dec_c, batch.dec_off[:h], batch.dec_n[:h], batch.T[:h], batch.targets[:h], NO,
                            "nospace", conf=conf)
    r2 = errs.score_decoded(batch.dec_c, batch.dec_off[h:], batch.dec_n[h:], batch.T[h:], batch.targets[h:], NO,
                            "nospace", conf=conf)
    assert r1.conf is conf and r2.conf is conf
    per, want = reference["nospace"]
    assert np.array_equal(np.concatenate([r1.per_line, r2.per_line]), per)
    assert np.array_equal(conf.cpu().numpy(), want)


def test_a_line_over_its_bound_is_refused_not_read(lines, reference):
    """line 1 of three decoded more characters than the bound its workspace was sized for: the kernel declines it
    before reading anything through its numbers; the neighbours are scored as ever"""
    from text_alignment_amd import errs
    pick = [7, 6, 3]
    b = Batch([lines[k] for k in pick])
    T = list(b.T)
    T[1] -= 2                                                                    # (T + 1) // 2 = 64 < dec_n = 65
    with pytest.raises(RuntimeError, match="refused line") as ei:
        errs.score_decoded(b.dec_c, b.dec_off, b.dec_n, T, b.targets, NO, "exact")
    assert ei.value.per_line[1].tolist() == [-1, 0, 0, 0, 0, 0]
    res = errs.score_decoded(b.dec_c, b.dec_off, b.dec_n, T, b.targets, NO, "exact", check=False)
    assert res.per_line[1].tolist() == [-1, 0, 0, 0, 0, 0]
    per = reference["exact"][0]
    assert res.per_line[0].tolist() == per[7].tolist() and res.per_line[2].tolist() == per[3].tolist()
    want = sum(R.score_line(*lines[k], NO + 1, "exact")[1] for k in (7, 3))
    assert np.array_equal(res.confusions(), want)                                # the refused line added nothing
    # a code outside the classes (the gap filler, read through a wrong offset) is declined the same way
    off = b.dec_off.clone()
    off[2] -= 1
    res = errs.score_decoded(b.dec_c, off, b.dec_n, b.T, b.targets, NO, "exact", check=False)
    assert res.per_line[2].tolist() == [-1, 0, 0, 0, 0, 0] and res.per_line[0].tolist() == per[7].tolist()


# ---- end to end -------------------------------------------------------------------------------------------------------
def _strip(rng, h, w):
    """word-like ink blobs around a baseline, grey-level antialiasing"""
    yy = np.arange(h)[:, None]
    dens = 0.6 * np.exp(-0.5 * ((yy - h / 2.0) / (h / 7.0)) ** 2) * np.ones((1, w))
    ink = rng.random((h, w)) < dens
    x = int(rng.integers(5, 40))
    while x < w:
        g = int(rng.integers(8, 30))
        ink[:, x:x + g] = False
        x += g + int(rng.integers(40, 120))
    return np.where(ink, rng.integers(0, 90, size=(h, w)), rng.integers(235, 256, size=(h, w))).astype(np.uint8)


@pytest.fixture(scope="module")
def e2e():
    from text_alignment_amd import ocr
    rng = np.random.default_rng(77)
    models = [ocr.LineModel.random(41), ocr.LineModel.random(42)]
    recs = [ocr.LineRecognizer(m) for m in models]
    prepared = [rng.random((int(t), 48)).astype(np.float32) for t in rng.integers(40, 201, size=24)]
    strips = [_strip(rng, int(h), int(w)) for h, w in zip(rng.integers(30, 60, size=6), rng.integers(60, 400, size=6))]
    letters = list("abcdefghijklmnopqrstuvwxyz   ~")
    texts = ["".join(rng.choice(letters, size=int(rng.integers(1, 60)))) for _ in range(24)]
    texts[3] = "abc ßdé f"                   # characters outside the codec
    texts[10] = ""
    texts[11] = "  two   spaces "
    return {"models": models, "recs": recs, "prepared": prepared, "strips": strips, "texts": texts}


def _want(rec, lines, texts, kind):
    codec = rec.model.codec
    codes = [[c for _, c in line] for line in rec.recognise(lines)]
    per, conf = R.score(codes, [R.encode_target(codec, t, kind) for t in texts], len(codec) + 1, kind)
    want = R.totals(per)
    want.update(per_line=per, confusions=R.confusions(conf, codec))
    return want


def _same(got, want):
    assert sorted(got) == ["cer", "chars", "confusions", "errors", "lines", "per_line"]
    assert (got["errors"], got["chars"], got["lines"]) == (want["errors"], want["chars"], want["lines"])
    assert got["cer"] == want["cer"] or (math.isnan(got["cer"]) and math.isnan(want["cer"]))
    assert got["per_line"].dtype == np.int32 and np.array_equal(got["per_line"], want["per_line"])
    assert got["confusions"] == want["confusions"]


def test_evaluate_equals_the_checker_on_recognised_lines(e2e):
    from text_alignment_amd import errs
    for kind in KINDS:
        want = _want(e2e["recs"][0], e2e["prepared"], e2e["texts"], kind)
        got = errs.evaluate(e2e["recs"][0], e2e["prepared"], e2e["texts"], kind=kind)
        print(kind, got["errors"], got["chars"], got["cer"], got["confusions"][:3])
        _same(got, want)
        assert got["chars"] > 0 and got["per_line"][10, 2] == 0 and any(t == "?" for _, _, t in got["confusions"])
    # a LineModel in place of the recogniser: the same numbers
    _same(errs.evaluate(e2e["models"][0], e2e["prepared"], e2e["texts"], kind="nospace"), want)
    empty = errs.evaluate(e2e["recs"][0], [], [])
    assert (empty["errors"], empty["chars"], empty["lines"], empty["confusions"]) == (0, 0, 0, []) and math.isnan(empty["cer"])


def test_evaluate_from_raw_strips_and_several_models(e2e):
    from text_alignment_amd import errs
    texts = e2e["texts"][:6]
    wants = [_want(rec, e2e["strips"], texts, "exact") for rec in e2e["recs"]]
    _same(errs.evaluate(e2e["recs"][0], e2e["strips"], texts), wants[0])
    both = errs.evaluate_models(e2e["recs"], e2e["strips"], texts)
    assert len(both) == 2
    for got, want, rec in zip(both, wants, e2e["recs"]):
        _same(got, want)
        _same(got, errs.evaluate(rec, e2e["strips"], texts))
    for got, rec in zip(errs.evaluate_models(e2e["recs"], e2e["prepared"], e2e["texts"], kind="nospace"), e2e["recs"]):
        _same(got, errs.evaluate(rec, e2e["prepared"], e2e["texts"], kind="nospace"))


def test_trainer_evaluates_its_current_weights(e2e):
    from text_alignment_amd import errs, train
    m = e2e["models"][1]
    tr = train.LineTrainer(model=m)
    got = tr.evaluate(e2e["prepared"], e2e["texts"])
    _same(got, errs.evaluate(e2e["recs"][1], e2e["prepared"], e2e["texts"]))
    assert tr.lines_seen == 0 and tr.W is None                   # nothing was trained, nothing distorted
