"""Checker of record for the held-out scoring of line models: the definitions stated directly
in plain Python.  Imports no product code.

A line is (a, g): a = the decoded class codes in translate_back order, g = the ground-truth text.  Codes: 0 = "" (never
a character), 1 = " ", No = len(codec) = "not in the codec".
"""
import unicodedata

import numpy as np

KINDS = ("exact", "nospace")


def normalise_text(s, kind="exact"):
    """NFC, then the kind's whitespace rule: "exact" collapses whitespace runs to one space and strips both ends,
    "nospace" removes all whitespace"""
    if kind not in KINDS:
        raise ValueError("unknown text kind %r" % (kind,))
    s = unicodedata.normalize("NFC", s)
    return " ".join(s.split()) if kind == "exact" else "".join(s.split())


def encode_target(codec, s, kind="exact"):
    """class codes of the normalised text; a character the codec lacks becomes len(codec)"""
    index = {ch: k for k, ch in enumerate(codec) if k > 0 and ch != ""}
    return [index.get(ch, len(codec)) for ch in normalise_text(s, kind)]


def filter_decoded(codes, kind="exact"):
    """class 0 dropped; then class 1 by the kind's rule; nothing else touched"""
    if kind not in KINDS:
        raise ValueError("unknown text kind %r" % (kind,))
    out = [int(c) for c in codes if c != 0]
    if kind == "nospace":
        return [c for c in out if c != 1]
    res = []
    for c in out:
        if c == 1 and (not res or res[-1] == 1):
            continue
        res.append(c)
    if res and res[-1] == 1:
        res.pop()
    return res


def distance_matrix(a, g):
    n, m = len(a), len(g)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    for j in range(m + 1):
        D[0][j] = j
    for i in range(1, n + 1):
        D[i][0] = i
        for j in range(1, m + 1):
            D[i][j] = min(D[i - 1][j - 1] + (a[i - 1] != g[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    return D


def align(a, g):
    """(errors, pairs): the recorded (decoded code or 0, truth code or 0) pairs of the walk from (n, m), last column
    first.  Tie order: diagonal, then insertion, then deletion."""
    D = distance_matrix(a, g)
    i, j = len(a), len(g)
    pairs = []
    while i > 0 or j > 0:
        if i > 0 and j > 0:
            cost = int(a[i - 1] != g[j - 1])
            if D[i][j] == D[i - 1][j - 1] + cost:
                pairs.append((a[i - 1], g[j - 1])); i -= 1; j -= 1
            elif D[i][j] == D[i - 1][j] + 1:
                pairs.append((a[i - 1], 0)); i -= 1
            else:
                pairs.append((0, g[j - 1])); j -= 1
        elif j == 0:
            pairs.append((a[i - 1], 0)); i -= 1
        else:
            pairs.append((0, g[j - 1])); j -= 1
    return D[len(a)][len(g)], pairs


def score_line(codes, target, nclasses, kind="exact"):
    """(six-tuple, conf): errors, n, m, substitutions, insertions, deletions of one line and its (nclasses, nclasses)
    int64 confusion counts; `codes` unfiltered, `target` encoded"""
    a = filter_decoded(codes, kind)
    g = [int(c) for c in target]
    errors, pairs = align(a, g)
    conf = np.zeros((nclasses, nclasses), dtype=np.int64)
    subs = ins = dels = 0
    for x, y in pairs:
        conf[x, y] += 1
        if y == 0:
            ins += 1
        elif x == 0:
            dels += 1
        elif x != y:
            subs += 1
    return (errors, len(a), len(g), subs, ins, dels), conf


def score(lines_codes, targets, nclasses, kind="exact"):
    """per_line (lines, 6) int32 and the summed conf of a batch"""
    per = np.zeros((len(lines_codes), 6), dtype=np.int32)
    conf = np.zeros((nclasses, nclasses), dtype=np.int64)
    for b, (codes, tgt) in enumerate(zip(lines_codes, targets)):
        per[b], c = score_line(codes, tgt, nclasses, kind)
        conf += c
    return per, conf


def totals(per_line):
    """errors, chars, lines, cer = sum errors / sum m (nan without characters)"""
    errors, chars = int(per_line[:, 0].sum()), int(per_line[:, 2].sum())
    return {"errors": errors, "chars": chars, "lines": int(per_line.shape[0]),
            "cer": errors / chars if chars else float("nan")}


def confusions(conf, codec):
    """off-diagonal (count, decoded char, truth char), count descending then by the two codes; "_" = nothing,
    "?" = not in the codec"""
    no = len(codec)

    def name(c):
        return "_" if c == 0 else ("?" if c == no else codec[c])
    out = [(int(conf[x, y]), x, y) for x in range(conf.shape[0]) for y in range(conf.shape[1]) if x != y and conf[x, y]]
    out.sort(key=lambda t: (-t[0], t[1], t[2]))
    return [(n, name(x), name(y)) for n, x, y in out]
