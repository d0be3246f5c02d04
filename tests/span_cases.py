"""Inputs shared by the span tests (tests/test_span*.py): the scoring systems of record, random small cases, planted noisy
spans over a fixed word list.  Deterministic: every generator takes its seed."""
import numpy as np

SYSTEMS = [[8, -4, -7, -7, -3, 0], [10, -5, -10, -10, -1, -1], [2, -1, 0, 0, -1, -1],
           [3, -2, 1, -1, 0, -2], [5, -5, -3, -8, 2, -1], [1, -1, -1, -1, 0, 0]]

WORDS = ("ad te levavi animam meam deus meus in te confido non erubescam neque irrideant me inimici mei etenim "
         "universi qui te expectant non confundentur vias tuas domine demonstra mihi et semitas tuas edoce me "
         "gloria patri et filio et spiritui sancto sicut erat in principio et nunc et semper et in secula seculorum "
         "amen dominus dixit ad me filius meus es tu ego hodie genui te quare fremuerunt gentes et populi meditati "
         "sunt inania puer natus est nobis et filius datus est nobis cuius imperium super humerum eius").split()


def small_case(seed):
    """n <= 12, m <= 9 over a 2- or 4-letter alphabet, every fourth case with a planted substring, now and then an
    empty side; returns (t, o, system) as int lists"""
    rng = np.random.RandomState(seed)
    alpha = 2 if seed % 2 else 4
    n = int(rng.randint(0, 13))
    m = int(rng.randint(0, 10))
    if seed % 37 == 0:
        n = 0
    if seed % 41 == 0:
        m = 0
    t = rng.randint(0, alpha, size=n)
    o = rng.randint(0, alpha, size=m)
    if seed % 4 == 0 and n >= 2 and m >= 1:
        a = int(rng.randint(0, n - 1))
        o = t[a:a + m].copy()
        if len(o) > 2 and seed % 8 == 0:
            o[int(rng.randint(0, len(o)))] ^= 1
    return t.tolist(), o.tolist(), SYSTEMS[seed % len(SYSTEMS)]


def text_of_words(rng, nchars):
    out = []
    size = 0
    while size < nchars:
        w = WORDS[int(rng.randint(0, len(WORDS)))]
        out.append(w)
        size += len(w) + 1
    return " ".join(out)


def noisy(rng, text, keep):
    """an "OCR reading" of text: each character kept with probability `keep`, else substituted, dropped or doubled"""
    letters = "abcdefghilmnopqrstuvx "
    out = []
    for ch in text:
        if rng.random_sample() < keep:
            out.append(ch)
            continue
        kind = int(rng.randint(0, 3))
        if kind == 0:
            out.append(letters[int(rng.randint(0, len(letters)))])
        elif kind == 2:
            out.append(ch); out.append(ch)
    return "".join(out)


def planted(seed, before, own, after, keep):
    """(transcript, ocr, (a, b)): the page's own text transcript[a:b] between `before` and `after` characters of other
    text, and its noisy reading"""
    rng = np.random.RandomState(seed)
    head = text_of_words(rng, before) + " " if before else ""
    body = text_of_words(rng, own)
    tail = " " + text_of_words(rng, after) if after else ""
    return head + body + tail, noisy(rng, body, keep), (len(head), len(head) + len(body))


def codes(*strings):
    """strings -> int32 arrays of code points shifted into 0 .. (what the kernels take: ids < 65535)"""
    return [np.frombuffer(s.encode("utf-32-le"), dtype="<u4").astype(np.int32) - 32 if len(s) else np.zeros(0, np.int32)
            for s in strings]
