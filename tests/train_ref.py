"""tests/train_ref.py -- numpy restatement of line-model TRAINING: the forward pass of
SURVEY.md Appendix B.3 / B.4 with its states kept, the CTC alignment, back-propagation through time and the momentum
update.  TEST INFRASTRUCTURE ONLY: the checker the training kernels (csrc/ta_train.hip) are compared with.

PARITY UNPINNED, as for Appendix B: the arithmetic follows ocropy 1.3.3 (`SeqRecognizer.trainSequence`,
`ctc_align_targets`, `LSTM.backward`, `Network.update`) as restated in DESIGN.md section 14; ocropy itself is not
available to compare with.  tests/test_train.py pins this file: its gradients against central differences, its lattice
against a brute-force enumeration of paths.

Every function takes `dtype`: np.float64 is the checker of record; np.float32 runs the same loops with every array
cast to single precision (the GPU tests measure their tolerance from the gap between the two), np.longdouble with
every array in extended precision: `noise64` is the float64 checker's own distance from that run, the yardstick of
`bound64`.
"""
import numpy as np

GATES = ("WGI", "WGF", "WGO", "WCI")
PEEPS = ("WIP", "WFP", "WOP")


def _sigmoid(x):
    return (1.0 / (1.0 + np.exp(np.clip(-x, -20, 20)))).astype(x.dtype)


def fresh_weights(seed, no, ni=48, ns=100):
    """(fwd, rev, W2): every weight uniform in (-0.1, 0.1), drawn in this order from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    na = 1 + ni + ns

    def lstm():
        d = {k: rng.uniform(-0.1, 0.1, size=(ns, na)) for k in GATES}
        d.update({k: rng.uniform(-0.1, 0.1, size=(ns,)) for k in PEEPS})
        return d
    fwd, rev = lstm(), lstm()
    return fwd, rev, rng.uniform(-0.1, 0.1, size=(no, 1 + 2 * ns))


def lstm_forward_states(w, xs, dtype=np.float64):
    """One direction of Appendix B.3 over xs (T, ni), keeping what BPTT needs: dict of (T, ns) arrays gi gf go ci c h
    and src (T, 1 + ni + ns), the step's input [1, x_t, h_{t-1}]."""
    W = {k: np.asarray(v, dtype=dtype) for k, v in w.items()}
    xs = np.asarray(xs, dtype=dtype)
    T, ni = xs.shape
    ns = W["WGI"].shape[0]
    st = {k: np.zeros((T, ns), dtype=dtype) for k in ("gi", "gf", "go", "ci", "c", "h")}
    st["src"] = np.zeros((T, 1 + ni + ns), dtype=dtype)
    h = np.zeros(ns, dtype=dtype)
    c = np.zeros(ns, dtype=dtype)
    one = np.ones(1, dtype=dtype)
    for t in range(T):
        src = np.concatenate((one, xs[t], h))
        gi, gf, go = W["WGI"].dot(src), W["WGF"].dot(src), W["WGO"].dot(src)
        ci = np.tanh(W["WCI"].dot(src))
        if t > 0:
            gi = gi + W["WIP"] * c
            gf = gf + W["WFP"] * c
        gi, gf = _sigmoid(gi), _sigmoid(gf)
        c_new = ci * gi
        if t > 0:
            c_new = c_new + gf * c
            go = go + W["WOP"] * c_new
        go = _sigmoid(go)
        c = c_new
        h = np.tanh(c) * go
        for k, v in (("gi", gi), ("gf", gf), ("go", go), ("ci", ci), ("c", c), ("h", h)):
            st[k][t] = v
        st["src"][t] = src
    return st


def net_forward(fwd, rev, W2, xs, dtype=np.float64):
    """Both directions and the softmax layer (Appendix B.4).  Returns dict: f, r (the directions' states; r in the
    reversed sequence's own order), y (T, 2 ns), probs (T, No)."""
    xs = np.asarray(xs, dtype=dtype)
    f = lstm_forward_states(fwd, xs, dtype)
    r = lstm_forward_states(rev, xs[::-1], dtype)
    y = np.concatenate([f["h"], r["h"][::-1]], axis=1)
    T = y.shape[0]
    z = np.concatenate([np.ones((T, 1), dtype=dtype), y], axis=1).dot(np.asarray(W2, dtype=dtype).T)
    p = np.exp(np.clip(z, -100, 100))
    p = p / p.sum(axis=1, keepdims=True)
    return {"f": f, "r": r, "y": y, "probs": p.astype(dtype)}


def logadd(x, y):
    with np.errstate(over="ignore"):
        return np.where(np.abs(x - y) > 10, np.maximum(x, y), np.log(np.exp(x - y) + 1) + y).astype(x.dtype)


def _lattice(lm, stats=None):
    """the forward recursion over lm (T, S): entry penalties -5 s before t = 0 and -5 t into state 0"""
    T, S = lm.shape
    dt = lm.dtype
    v = (-5.0 * np.arange(S)).astype(dt)
    A = np.zeros((T, S), dtype=dt)
    for t in range(T):
        w = np.concatenate((np.array([-5.0 * t], dtype=dt), v[:-1]))
        if stats is not None:
            gap = np.abs(v - w).astype(np.float64)
            stats["max_logadd_gap"] = max(stats.get("max_logadd_gap", 0.0), float(gap.max()))
            stats["min_logadd_gap"] = min(stats.get("min_logadd_gap", np.inf), float(gap.min()))
            stats["min_threshold_distance"] = min(stats.get("min_threshold_distance", np.inf),
                                                  float(np.abs(gap - 10.0).min()))
        v = logadd(v, w) + lm[t]
        A[t] = v
    return A


def ctc_labels(cs):
    lab = np.zeros(2 * len(cs) + 1, dtype=np.int64)
    lab[1::2] = cs
    return lab


def match_matrix(P, cs, dtype=np.float64):
    P = np.asarray(P, dtype=dtype)
    Q = np.maximum(P, dtype(1e-5))
    Q = Q / Q.sum(axis=1, keepdims=True)
    return np.log(Q[:, ctc_labels(cs)]).astype(dtype)


def normalise_paths(both, lab, no):
    """both = A + B (T, S) -> aligned (T, No): the spec's column normalisation, scatter into classes, clamp, row
    normalisation"""
    dt = both.dtype
    E = np.exp(both - both.max())
    l = E.sum(axis=0)
    E = E / np.where(l == 0, dt.type(1e-9), l)[None, :]
    aligned = np.zeros((both.shape[0], no), dtype=dt)
    for s in range(len(lab)):
        aligned[:, lab[s]] += E[:, s]
    aligned = np.maximum(aligned, dt.type(1e-5))
    l = aligned.sum(axis=1)
    return (aligned / np.where(l == 0, dt.type(1e-9), l)[:, None]).astype(dt)


def ctc_align_targets(P, cs, dtype=np.float64, stats=None):
    """aligned (T, No) for one line's softmax outputs P (T, No) and target codes cs.
    stats (a dict): receives max_logadd_gap and min_logadd_gap, the largest and the smallest |x - y| any logadd of the
    two recursions saw, and min_threshold_distance, the smallest ||x - y| - 10|: how close any of them came to the
    shortcut's threshold, where the result jumps by log(1 + exp(-10)) = 4.5e-5."""
    P = np.asarray(P, dtype=dtype)
    cs = [int(c) for c in cs]
    T, no = P.shape
    if 2 * len(cs) + 1 > T:
        raise ValueError("target of %d characters does not fit %d timesteps" % (len(cs), T))
    lm = match_matrix(P, cs, dtype)
    A = _lattice(lm, stats)
    B = _lattice(lm[::-1, ::-1], stats)[::-1, ::-1]
    return normalise_paths(A + B, ctc_labels(cs), no)


def lstm_backward(w, st, dy, dtype=np.float64):
    """BPTT of one direction: dy (T, ns) is d(-CE)/dh in the direction's own step order.  Returns the weight gradients
    (dict like w) and the gate errors e (T, 4, ns) in the order gi, gf, go, ci."""
    W = {k: np.asarray(v, dtype=dtype) for k, v in w.items()}
    dy = np.asarray(dy, dtype=dtype)
    T, ns = dy.shape
    nh = W["WGI"].shape[1] - ns
    gi, gf, go, ci, c = st["gi"], st["gf"], st["go"], st["ci"], st["c"]
    e = np.zeros((T, 4, ns), dtype=dtype)
    ec_next = np.zeros(ns, dtype=dtype)
    herr = np.zeros(ns, dtype=dtype)
    for t in range(T - 1, -1, -1):
        oe = dy[t] + herr if t < T - 1 else dy[t]
        tc = np.tanh(c[t])
        e_go = go[t] * (1 - go[t]) * tc * oe
        e_c = (1 - tc * tc) * go[t] * oe
        if t > 0:
            e_c = e_c + e_go * W["WOP"]
        if t < T - 1:
            e_c = e_c + e[t + 1, 1] * W["WFP"] + e[t + 1, 0] * W["WIP"] + ec_next * gf[t + 1]
        e_gf = gf[t] * (1 - gf[t]) * e_c * c[t - 1] if t > 0 else np.zeros(ns, dtype=dtype)
        e_gi = gi[t] * (1 - gi[t]) * e_c * ci[t]
        e_ci = (1 - ci[t] * ci[t]) * e_c * gi[t]
        e[t, 0], e[t, 1], e[t, 2], e[t, 3] = e_gi, e_gf, e_go, e_ci
        ec_next = e_c
        herr = (e_gi.dot(W["WGI"]) + e_gf.dot(W["WGF"]) + e_go.dot(W["WGO"]) + e_ci.dot(W["WCI"]))[nh:]
    g = {name: e[:, k].T.dot(st["src"]) for k, name in enumerate(GATES)}
    g["WIP"] = (e[1:, 0] * c[:-1]).sum(axis=0)
    g["WFP"] = (e[1:, 1] * c[:-1]).sum(axis=0)
    g["WOP"] = (e[1:, 2] * c[1:]).sum(axis=0)
    return g, e


def gradients(fwd, rev, W2, xs, cs, dtype=np.float64, aligned=None):
    """One line: forward, alignment (unless `aligned` is given: held fixed), deltas, and the derivative of -CE with
    respect to every weight array.  Returns dict: fwd, rev (dicts), W2, probs, aligned, deltas, error."""
    out = net_forward(fwd, rev, W2, xs, dtype)
    P = out["probs"]
    if aligned is None:
        aligned = ctc_align_targets(P, cs, dtype)
    aligned = np.asarray(aligned, dtype=dtype)
    deltas = aligned - P
    T = P.shape[0]
    ns = out["f"]["h"].shape[1]
    W2 = np.asarray(W2, dtype=dtype)
    DW2 = deltas.T.dot(np.concatenate([np.ones((T, 1), dtype=dtype), out["y"]], axis=1))
    dy = deltas.dot(W2[:, 1:])
    gf_, _ = lstm_backward(fwd, out["f"], dy[:, :ns], dtype)
    gr_, _ = lstm_backward(rev, out["r"], dy[::-1, ns:], dtype)
    return {"fwd": gf_, "rev": gr_, "W2": DW2, "probs": P, "aligned": aligned, "deltas": deltas,
            "error": float((deltas.astype(np.float64) ** 2).sum())}


def cross_entropy(fwd, rev, W2, xs, aligned):
    """CE = -sum aligned log P, float64 (the function whose negative the gradients differentiate)"""
    P = net_forward(fwd, rev, W2, xs)["probs"]
    return float(-(aligned * np.log(P)).sum())


class Trainer(object):
    """ocropy's Network.update around gradients(): ds = momentum ds + lrate DW; W += ds, one update per call."""

    def __init__(self, fwd, rev, W2, lrate=1e-4, momentum=0.9, dtype=np.float64):
        self.dtype = dtype
        self.fwd = {k: np.array(v, dtype=dtype) for k, v in fwd.items()}
        self.rev = {k: np.array(v, dtype=dtype) for k, v in rev.items()}
        self.W2 = np.array(W2, dtype=dtype)
        self.lrate, self.momentum = dtype(lrate), dtype(momentum)
        self.ds = None

    def arrays(self):
        return [self.fwd[k] for k in GATES + PEEPS] + [self.rev[k] for k in GATES + PEEPS] + [self.W2]

    def update(self, lines, texts_codes):
        """one update from the summed gradients of the given lines (one line: ocropy's own schedule)"""
        total, outs = None, []
        for xs, cs in zip(lines, texts_codes):
            g = gradients(self.fwd, self.rev, self.W2, xs, cs, self.dtype)
            outs.append(g)
            flat = [g["fwd"][k] for k in GATES + PEEPS] + [g["rev"][k] for k in GATES + PEEPS] + [g["W2"]]
            total = flat if total is None else [a + b for a, b in zip(total, flat)]
        if self.ds is None:
            self.ds = [np.zeros_like(a) for a in total]
        for a, d, dw in zip(self.arrays(), self.ds, total):
            d *= self.momentum
            d += self.lrate * dw
            a += d
        return outs


def translate_back(outputs, threshold=0.7):
    """Appendix B.5 (as oracle/ocr_ref_f64.py): classes of the maxima of the runs below threshold"""
    T = outputs.shape[0]
    res, t = [], 0
    while t < T:
        if outputs[t, 0] < threshold:
            s = t
            while t < T and outputs[t, 0] < threshold:
                t += 1
            seg = outputs[s:t]
            res.append(int(np.argmax(seg)) % seg.shape[1])
        else:
            t += 1
    return res


# ---- the synthetic task of the learning test (tests/test_train_gpu.py) ------------------------------------------------
def glyph_task(seed=0, nclasses=8):
    """glyphs[c]: 6 columns x 48 rows of Bernoulli(0.4) ink for every class (only 3 .. nclasses - 1 are drawn)"""
    rng = np.random.default_rng(seed)
    return (rng.random((nclasses, 6, 48)) < 0.4).astype(np.float64)


def glyph_line(glyphs, rng, nchars=5):
    """(xs (72, 48), codes): nchars characters of classes 3 .. 7, each in an 8-column cell, 16 columns of padding"""
    codes = rng.integers(3, glyphs.shape[0], size=nchars)
    xs = np.zeros((32 + 8 * nchars, 48))
    for k, c in enumerate(codes):
        xs[16 + 8 * k + 1:16 + 8 * k + 7] = glyphs[c]
    return xs, [int(c) for c in codes]


# ---- the batch the GPU tests and tools/train_agreement.py compare on ---------------------------------------------------
def spec_batch(seed=31, no=20, lengths=(40, 97, 150, 233, 400)):
    """(fwd, rev, W2, codec, lines, texts, codes): seeded weights (LSTM +-0.2, output layer +-0.5), lines of mixed
    length (blurred random ink between 16 columns of padding, float32 values) and random texts of about T / 8
    characters with repeated characters in them"""
    rng = np.random.default_rng(seed)
    na = 1 + 48 + 100

    def lstm():
        d = {k: rng.uniform(-0.2, 0.2, size=(100, na)) for k in GATES}
        d.update({k: rng.uniform(-0.2, 0.2, size=(100,)) for k in PEEPS})
        return d
    fwd, rev = lstm(), lstm()
    W2 = rng.uniform(-0.5, 0.5, size=(no, 201))
    codec = ["", " ", "~"] + [chr(ord("a") + k) for k in range(no - 3)]
    lines, texts, codes = [], [], []
    for T in lengths:
        ink = (rng.random((T - 32, 48)) < 0.15).astype(np.float64)
        img = ink.copy()
        img[1:] += 0.5 * ink[:-1]
        img[:, 1:] += 0.5 * ink[:, :-1]
        xs = np.zeros((T, 48), dtype=np.float32)
        xs[16:T - 16] = np.clip(img, 0, 1)
        cs = [int(c) for c in rng.integers(1, no, size=max(1, T // 8))]
        if len(cs) > 2:
            cs[1] = cs[0]                                   # a repeated character
        lines.append(xs)
        codes.append(cs)
        texts.append("".join(codec[c] for c in cs))
    return fwd, rev, W2, codec, lines, texts, codes


def closeness(got, ref64, ref32):
    """(error of `got` against the float64 checker, the float32 checker's own gap to it, their ratio): max-abs over the
    array.  The GPU tests require ratio <= their bound: a float32 implementation sits at a ratio around 1."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    err = float(np.abs(np.asarray(got, dtype=np.float64) - ref64).max())
    gap = float(np.abs(np.asarray(ref32, dtype=np.float64) - ref64).max())
    return err, gap, (err / gap if gap > 0 else float("inf") if err > 0 else 0.0)


# ---- the yardstick taken from the checker alone ------------------------------------------------------------------------
FACTOR64 = 64.0


def noise64(ref64, refld):
    """max-abs distance of the float64 checker's array from the long-double checker's on the same input: what float64
    rounding alone moves this array by (one sample of it)"""
    return float(np.abs(np.asarray(ref64, dtype=np.longdouble) - np.asarray(refld, dtype=np.longdouble)).max(initial=0.0))


def bound64(ref64, noise, factor=FACTOR64):
    """factor x max(noise64, 4 ulp of the array's largest reference magnitude): the distance from the float64 checker a
    float64 implementation may have.  The factor is fixed in advance (another order of summation, device exp / log /
    tanh of 1 - 2 ulp where libm has 0.5, and noise64 being one sample of a rounding walk); it is not measured from
    the kernels."""
    top = float(np.abs(np.asarray(ref64, dtype=np.float64)).max(initial=0.0))
    return factor * max(float(noise), 4.0 * float(np.spacing(top)))


def distance(got, ref64):
    """max-abs distance of `got` from the checker's array; a non-finite or missing entry counts as infinite"""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    if got.shape != ref64.shape:
        return float("inf")
    d = np.abs(got - ref64)
    return float("inf") if not np.isfinite(d).all() else float(d.max(initial=0.0))
