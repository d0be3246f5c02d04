"""The training cases that tests/test_train_cases.py (the cases against wrong variants of the checker, no kernel),
tests/test_train_sim.py (the host build of csrc/ta_train.hip) and tests/test_train_edges_gpu.py (the real kernels) share,
the layouts the last two drive the C ABI with, and the checker's answers with their yardstick, computed once per process.

The yardstick comes from the checker alone (tests/train_ref.py: noise64, bound64): every compared array may lie
64 x max(noise64, 4 ulp of its largest reference magnitude) from the float64 checker, noise64 being the float64 checker's
own distance from its long-double run on the same input.

Lattice cases are probability matrices built without the network: `lattice_cases()`.  Network cases are seeded
spec_batch-style models with short lines: `net_cases()`.  `pack_ctc` / `pack_net` lay a batch out the way a caller
would not: lines stored out of order with gap rows in front of each, labels of 999 -- a label no line may read -- around
the texts, workspace pieces that start 32 doubles in and lie 2 .. 4 doubles apart; the calls run with every output and
the workspace poisoned.
"""
import numpy as np

import train_ref as R
from text_alignment_amd import _abi

NI, NS = 48, 100
POISON = -7.77e77                      # finite: a poisoned cell compares equal to itself
MAX_T, MAX_STATES = 5000, 2049         # TA_TRAIN_MAX_T, TA_CTC_MAX_STATES (tests/test_train_cases.py holds them to the header)
OUT_ROWS = 8                           # csrc/ta_train.hip: kOutRows


def bind(lib):
    return _abi.bind(lib, ["ta_ctc_workspace_bytes", "ta_lstm_train_forward", "ta_lstm_train_backward", "ta_ctc_align"])


# ---- lattice cases ---------------------------------------------------------------------------------------------------------
LATTICE_SHAPES = ((1, 0, 5), (3, 1, 2), (64, 20, 2), (300, 0, 5), (255, 60, 20), (256, 60, 20), (257, 128, 7),
                  (257, 100, 128), (513, 256, 20), (600, 280, 20), (5000, 3, 20), (2049, 1024, 20))
SHARPNESS = (0.0, 0.95)
LATTICE_SEED = 1414                    # (a seed that fails a condition of tests/test_train_cases.py is changed; the condition is not)


def lattice_labels(L, no, seed=LATTICE_SEED):
    """L target codes in 1 .. no - 1, the first two equal, the last no - 1; a function of (L, no) alone, so T = 255 and
    T = 256 are aligned with the same text"""
    cs = np.random.default_rng([seed, L, no]).integers(1, no, size=L)
    if L > 1:
        cs[1] = cs[0]
    if L > 0:
        cs[-1] = no - 1
    return [int(c) for c in cs]


def lattice_probs(T, cs, no, sharp, seed=LATTICE_SEED):
    """(T, no) rows that sum to 1: (1 - sharp) of a random row plus `sharp` on the class of the state a straight line
    from (0, 0) to (T - 1, S - 1) occupies; about 10 % of the entries (never that class) exactly 0"""
    rng = np.random.default_rng([seed, T, len(cs), no, int(round(100 * sharp))])
    lab = R.ctc_labels(cs)
    S = len(lab)
    on = lab[np.rint(np.arange(T) * ((S - 1) / max(T - 1, 1))).astype(np.int64)]
    P = rng.random((T, no)) + 0.05
    P /= P.sum(axis=1, keepdims=True)
    P *= 1.0 - sharp
    P[np.arange(T), on] += sharp
    zero = rng.random((T, no)) < 0.1
    zero[np.arange(T), on] = False
    P[zero] = 0.0
    return P / P.sum(axis=1, keepdims=True)


_LATTICE = []


def lattice_cases():
    """[(name, P (T, no), cs)]: every shape at both sharpnesses"""
    if not _LATTICE:
        for T, L, no in LATTICE_SHAPES:
            cs = lattice_labels(L, no)
            for sharp in SHARPNESS:
                _LATTICE.append(("T%d L%d no%d sharp%g" % (T, L, no, sharp), lattice_probs(T, cs, no, sharp), cs))
    return _LATTICE


def lattice_case(name):
    return [c for c in lattice_cases() if c[0] == name][0]


def lattice_answer(P, cs, dtype=np.float64, stats=None):
    """{"aligned", "deltas", "err"} of one line, as ta_ctc_align returns them"""
    al = R.ctc_align_targets(P, cs, dtype=dtype, stats=stats)
    de = al - np.asarray(P, dtype=dtype)
    return {"aligned": al, "deltas": de, "err": np.asarray([(de * de).sum()], dtype=dtype)}


class Want(object):
    """the float64 checker's arrays of a case (ref), per array its noise64 and bound64, and for a lattice its stats"""

    def __init__(self, ref, refld, stats=None):
        self.ref, self.stats = ref, stats
        self.noise = {k: R.noise64(ref[k], refld[k]) for k in ref}
        self.bound = {k: R.bound64(ref[k], self.noise[k]) for k in ref}

    def miss(self, got, keys=None):
        """{array: distance / bound} of `got`'s arrays"""
        return {k: R.distance(got[k], self.ref[k]) / self.bound[k] for k in (keys or got)}

    def check(self, got, what, keys=None, record=None):
        miss = self.miss(got, keys)
        if record is not None:
            record.extend({"case": what, "array": k, "error": q * self.bound[k], "noise64": self.noise[k],
                           "quotient": q * R.FACTOR64} for k, q in miss.items())
        for k, q in miss.items():
            assert q <= 1.0, "%s, %s: %.3g from the checker, bound %.3g (noise64 %.3g)" % (
                what, k, q * self.bound[k], self.bound[k], self.noise[k])


_WANT = {}


def lattice_want(name):
    if ("lattice", name) not in _WANT:
        _, P, cs = lattice_case(name)
        stats = {}
        _WANT["lattice", name] = Want(lattice_answer(P, cs, stats=stats), lattice_answer(P, cs, dtype=np.longdouble), stats)
    return _WANT["lattice", name]


# ---- network cases ---------------------------------------------------------------------------------------------------------
def _lines(rng, lengths, no):
    """blurred random ink on every row (float32 values) and texts of (T - 1) // 2 codes, the first two equal"""
    lines, codes = [], []
    for T in lengths:
        ink = (rng.random((T, NI)) < 0.15).astype(np.float64)
        img = ink.copy()
        img[1:] += 0.5 * ink[:-1]
        img[:, 1:] += 0.5 * ink[:, :-1]
        lines.append(np.clip(img, 0, 1).astype(np.float32))
        cs = [int(c) for c in rng.integers(1, no, size=(T - 1) // 2)]
        if len(cs) > 1:
            cs[1] = cs[0]
        codes.append(cs)
    return lines, codes


def saturate(fwd, rev, W2):
    """copies with the gates' bias columns shifted by +30 (units 0, 4, ..) and -30 (units 2, 6, ..) and output biases of
    +150, -150 and +120 on classes 0, 1 and 2: past the sigmoid's +-20 and the logits' +-100"""
    fwd, rev = ({k: np.array(v) for k, v in w.items()} for w in (fwd, rev))
    for w in (fwd, rev):
        for k in R.GATES:
            w[k][0::4, 0] += 30.0
            w[k][2::4, 0] -= 30.0
    W2 = np.array(W2)
    W2[0, 0], W2[1, 0], W2[2, 0] = 150.0, -150.0, 120.0
    return fwd, rev, W2


_NET = []


def net_cases():
    """[(name, (fwd, rev, W2, codec), lines, codes)].  57 and 55 rows: output-layer tails of 1 and 7 rows and workgroups
    of 8 rows that straddle lines; T = 1, 2, 3: neither guard of the recurrences, no interior step, the first with one."""
    if not _NET:
        def add(name, seed, no, lengths, sat=False):
            fwd, rev, W2, codec, _, _, _ = R.spec_batch(seed=seed, no=no, lengths=())
            if sat:
                fwd, rev, W2 = saturate(fwd, rev, W2)
            lines, codes = _lines(np.random.default_rng([seed, no]), lengths, no)
            _NET.append((name, (fwd, rev, W2, codec[:no]), lines, codes))       # (spec_batch's codec has 3 entries at least)
        add("57 rows", 41, 20, (1, 2, 3, 9, 42))
        add("55 rows", 42, 20, (2, 3, 9, 41))
        for no in (2, 3, 127, 128):
            add("no %d" % no, 43, no, (3, 9, 14))
        add("saturated", 44, 20, (2, 3, 9, 21), sat=True)
    return _NET


def net_case(name):
    return [c for c in net_cases() if c[0] == name][0]


def texts_of(codec, codes):
    return ["".join(codec[c] for c in cs) for cs in codes]


def flat_names():
    return ["fwd " + k for k in R.GATES + R.PEEPS] + ["rev " + k for k in R.GATES + R.PEEPS] + ["W2"]


def line_answer(model, xs, cs, dtype=np.float64):
    """everything the kernels and LineTrainer leave of one line, in the kernels' layouts: probs (T, no), hout (T, 200),
    states (T, 2, 6, 100: gi gf go ci c h_prev), aligned, deltas, err, dy (T, 200), gate_err (T, 2, 400), dpeep
    (2, 3, 100) and the weight gradients by the names of flat_names().  The reversed direction is stored at the line's
    own rows.  The same steps as train_ref.gradients (tests/test_train_cases.py holds the two equal)."""
    fwd, rev, W2 = model[:3]
    out = R.net_forward(fwd, rev, W2, xs, dtype)
    P = out["probs"]
    T = P.shape[0]
    aligned = R.ctc_align_targets(P, cs, dtype)
    deltas = aligned - P
    W2d = np.asarray(W2, dtype=dtype)
    dy = deltas.dot(W2d[:, 1:])
    gf_, ef = R.lstm_backward(fwd, out["f"], dy[:, :NS], dtype)
    gr_, er = R.lstm_backward(rev, out["r"], dy[::-1, NS:], dtype)

    def fields(st):
        return np.stack([st[k] for k in ("gi", "gf", "go", "ci", "c")] + [st["src"][:, 1 + NI:]], axis=1)
    a = {"probs": P, "hout": out["y"], "states": np.stack([fields(out["f"]), fields(out["r"])[::-1]], axis=1),
         "aligned": aligned, "deltas": deltas, "err": np.asarray([(deltas * deltas).sum()], dtype=dtype), "dy": dy,
         "gate_err": np.stack([ef.reshape(T, 4 * NS), er[::-1].reshape(T, 4 * NS)], axis=1),
         "dpeep": np.stack([np.stack([g[k] for k in R.PEEPS]) for g in (gf_, gr_)]),
         "W2": deltas.T.dot(np.concatenate([np.ones((T, 1), dtype=dtype), out["y"]], axis=1))}
    for d, g in (("fwd ", gf_), ("rev ", gr_)):
        a.update({d + k: g[k] for k in R.GATES + R.PEEPS})
    return a


def net_want(name):
    """[Want] per line of a network case"""
    if ("net", name) not in _WANT:
        _, model, lines, codes = net_case(name)
        _WANT["net", name] = [Want(line_answer(model, xs, cs), line_answer(model, xs, cs, np.longdouble))
                              for xs, cs in zip(lines, codes)]
    return _WANT["net", name]


# ---- the C ABI with a caller's own layout ----------------------------------------------------------------------------------
class Packed(object):
    pass


def _p(a):
    return a.ctypes.data


def host_ptr(pk):
    return lambda name: _p(getattr(pk, name))


def _place(n, sizes, first, gap0):
    """offsets of n pieces stored in REVERSED order behind `first` cells, a gap of gap0 + (q % 3) cells in front of the
    q-th stored piece and one behind the last: (offsets by line, total)"""
    off, at = [0] * n, first
    for q, b in enumerate(reversed(range(n))):
        at += gap0 + q % 3
        off[b] = at
        at += int(sizes[b])
    return np.asarray(off, np.int64), at + gap0


def pack_ctc(lib, lines, no):
    """host arrays of one ta_ctc_align call on lines [(P, cs)]"""
    pk = Packed()
    n = pk.n = len(lines)
    pk.no = no
    pk.T = np.asarray([len(P) for P, _ in lines], np.int32)
    pk.L = np.asarray([len(cs) for _, cs in lines], np.int32)
    pk.row_off, pk.rows = _place(n, pk.T, 0, 1)
    pk.lab_off, pk.nlabels = _place(n, pk.L, 0, 2)
    need = [int(lib.ta_ctc_workspace_bytes(int(t), int(l), no)) for t, l in zip(pk.T, pk.L)]
    assert min(need) > 0 and all(b % 8 == 0 for b in need)
    pk.ws_size = np.asarray(need, np.int64) // 8
    pk.ws_off, ws_doubles = _place(n, pk.ws_size, 32, 2)
    pk.ws_bytes = 8 * ws_doubles
    pk.probs = np.full((pk.rows, no), 0.5)
    pk.labels = np.full(pk.nlabels, 999, np.int32)
    for b, (P, cs) in enumerate(lines):
        pk.probs[pk.row_off[b]:pk.row_off[b] + len(P)] = P
        pk.labels[pk.lab_off[b]:pk.lab_off[b] + len(cs)] = cs
    pk.ws = np.full(ws_doubles, POISON)
    pk.aligned, pk.deltas = np.full((pk.rows, no), POISON), np.full((pk.rows, no), POISON)
    pk.err = np.full(n, POISON)
    return pk


CTC_INPUTS = ("probs", "row_off", "T", "labels", "lab_off", "L", "ws_off")
CTC_OUTPUTS = ("aligned", "deltas", "err", "ws")


def call_ctc(lib, pk, ptr, stream=None, **over):
    """ta_ctc_align on pk's arrays, `ptr(array name)` giving each [device] pointer; over: arguments to replace (T_host
    and L_host as arrays)"""
    a = dict(n=pk.n, no=pk.no, rows=pk.rows, nlabels=pk.nlabels, T_host=pk.T, L_host=pk.L, ws_bytes=pk.ws_bytes)
    for name in CTC_INPUTS + CTC_OUTPUTS:
        a[name] = ptr(name)
    a.update(over)
    Th, Lh = np.ascontiguousarray(a["T_host"], np.int32), np.ascontiguousarray(a["L_host"], np.int32)
    return lib.ta_ctc_align(a["probs"], a["row_off"], a["T"], a["labels"], a["lab_off"], a["L"], a["ws_off"], a["n"],
                            a["no"], a["rows"], a["nlabels"], _p(Th), _p(Lh), a["ws"], a["ws_bytes"], a["aligned"],
                            a["deltas"], a["err"], stream)


def _rows_of(layout, b):
    return slice(int(layout.row_off[b]), int(layout.row_off[b]) + int(layout.T[b]))


def check_ctc(pk, layout, wants, refused=(), what="", record=None):
    """every output of a call: accepted lines within the bound of the checker, a refused line's err NaN and its rows and
    workspace piece still poison, as is every gap.  layout: the packing the HOST knows (a spoiled device copy may differ)"""
    own = np.zeros(pk.rows, dtype=bool)
    used = np.zeros(len(pk.ws), dtype=bool)
    for b, w in enumerate(wants):
        if b in refused:
            assert np.isnan(pk.err[b]), (what, b, pk.err[b])
            continue
        r = _rows_of(layout, b)
        w.check({"aligned": pk.aligned[r], "deltas": pk.deltas[r], "err": pk.err[b:b + 1]}, "%s line %d" % (what, b),
                record=record)
        assert np.abs(pk.aligned[r].sum(axis=1) - 1.0).max() <= w.bound["aligned"], (what, b)
        own[r] = True
        used[int(layout.ws_off[b]):int(layout.ws_off[b]) + int(layout.ws_size[b])] = True
    assert (pk.aligned[~own] == POISON).all() and (pk.deltas[~own] == POISON).all(), what + ": a row of no accepted line was written"
    assert (pk.ws[~used] == POISON).all(), what + ": the workspace was written outside the accepted lines' pieces"


def pack_net(model, lines, wants):
    """host arrays of ta_lstm_train_forward / _backward on prepared lines; dy is the checker's (wants: their Want)"""
    fwd, rev, W2 = model[:3]
    pk = Packed()
    n = pk.n = len(lines)
    pk.no = int(np.asarray(W2).shape[0])
    pk.T = np.asarray([len(x) for x in lines], np.int32)
    pk.max_T = int(pk.T.max())
    pk.row_off, pk.rows = _place(n, pk.T, 0, 1)
    pk.W = np.ascontiguousarray(np.stack([np.stack([np.asarray(w[k], np.float64) for k in R.GATES]) for w in (fwd, rev)]))
    pk.peep = np.ascontiguousarray(np.stack([np.stack([np.asarray(w[k], np.float64) for k in R.PEEPS]) for w in (fwd, rev)]))
    pk.W2 = np.ascontiguousarray(W2, np.float64)
    pk.gx = np.full((pk.rows, 2, 4 * NS), 0.25)
    pk.dy = np.full((pk.rows, 2 * NS), 0.25)
    Wx = pk.W[:, :, :, :1 + NI].reshape(8 * NS, 1 + NI)
    for b, xs in enumerate(lines):
        x1 = np.concatenate([np.ones((len(xs), 1)), np.asarray(xs, np.float64)], axis=1)
        pk.gx[_rows_of(pk, b)] = x1.dot(Wx.T).reshape(len(xs), 2, 4 * NS)
        pk.dy[_rows_of(pk, b)] = wants[b].ref["dy"]
    pk.states = np.full((pk.rows, 2, 6, NS), POISON)
    pk.hout = np.full((pk.rows, 2 * NS), POISON)
    pk.probs = np.full((pk.rows, pk.no), POISON)
    pk.gate_err = np.full((pk.rows, 2, 4 * NS), POISON)
    pk.dpeep = np.full((n, 2, 3, NS), POISON)
    return pk


NET_INPUTS = ("gx", "dy", "row_off", "T", "W", "peep", "W2")
NET_OUTPUTS = ("states", "hout", "probs", "gate_err", "dpeep")


def call_forward(lib, pk, ptr, stream=None):
    return lib.ta_lstm_train_forward(ptr("gx"), ptr("row_off"), ptr("T"), pk.n, pk.max_T, pk.rows, ptr("W"), ptr("peep"),
                                     ptr("W2"), pk.no, ptr("states"), ptr("hout"), ptr("probs"), stream)


def call_backward(lib, pk, ptr, stream=None):
    return lib.ta_lstm_train_backward(ptr("dy"), ptr("states"), ptr("row_off"), ptr("T"), pk.n, pk.max_T, pk.rows,
                                      ptr("W"), ptr("peep"), ptr("gate_err"), ptr("dpeep"), stream)


def check_net(pk, layout, wants, refused=(), what="", record=None):
    """both calls' outputs: accepted lines within the bound, a refused line's states, hout, gate_err and dpeep rows still
    poison (its probs rows are unspecified), as is every gap row of those four"""
    own = np.zeros(pk.rows, dtype=bool)
    for b, w in enumerate(wants):
        if b in refused:
            assert (pk.dpeep[b] == POISON).all(), (what, b)
            continue
        r = _rows_of(layout, b)
        w.check({"states": pk.states[r], "hout": pk.hout[r], "probs": pk.probs[r], "gate_err": pk.gate_err[r],
                 "dpeep": pk.dpeep[b]}, "%s line %d" % (what, b), record=record)
        own[r] = True
    for name in ("states", "hout", "gate_err"):
        assert (getattr(pk, name)[~own] == POISON).all(), "%s: %s was written outside the accepted lines" % (what, name)


# the device-side refusals of ta_ctc_align: (what, array, value for the MIDDLE line of three) -- the host's copies stay right
def ctc_edits(pk, b=1):
    T, L = int(pk.T[b]), int(pk.L[b])
    return [("T = 0", "T", b, 0), ("T = 5001", "T", b, MAX_T + 1), ("S = T + 1", "T", b, 2 * L),
            ("row_off negative", "row_off", b, -1), ("row_off past rows", "row_off", b, pk.rows - T + 1),
            ("labels past nlabels", "lab_off", b, pk.nlabels - L + 1), ("ws_off negative", "ws_off", b, -8),
            ("ws_off past the workspace", "ws_off", b, len(pk.ws) - int(pk.ws_size[b]) + 1),
            ("a label equal to no", "labels", int(pk.lab_off[b]) + L // 2, pk.no),
            ("a label equal to -1", "labels", int(pk.lab_off[b]) + L - 1, -1)]


def net_edits(pk, b=1):
    return [("T = 0", "T", b, 0), ("row_off negative", "row_off", b, -2),
            ("row_off past rows", "row_off", b, pk.rows - int(pk.T[b]) + 1)]


def three_lattice_lines():
    """a good line, the line the edits spoil (2 L + 1 == T, so T - 1 no longer holds its states), a good line with more
    states than lanes"""
    no = 7
    out = []
    for T, L, sharp in ((30, 9, 0.0), (21, 10, 0.95), (300, 140, 0.0)):
        cs = lattice_labels(L, no)
        out.append((lattice_probs(T, cs, no, sharp), cs))
    return no, out


def three_lattice_wants():
    if "three" not in _WANT:
        _WANT["three"] = [Want(lattice_answer(P, cs), lattice_answer(P, cs, dtype=np.longdouble))
                          for P, cs in three_lattice_lines()[1]]
    return _WANT["three"]


# ---- the same cases on the device (tests/test_train_edges_gpu.py, tools/train_agreement.py) --------------------------------
class Device(object):
    """a packing's arrays on the device; back() copies the outputs into the packing"""

    def __init__(self, pk, inputs, outputs, **over):
        import torch
        self.pk, self.outputs, self.torch = pk, outputs, torch
        self.t = {name: torch.from_numpy(over[name] if name in over else getattr(pk, name)).cuda()
                  for name in inputs + outputs}

    def ptr(self, name):
        return self.t[name].data_ptr()

    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def back(self):
        for name in self.outputs:
            getattr(self.pk, name)[...] = self.t[name].cpu().numpy()
        return self.pk


def device_lattice(name):
    """train.ctc_align_targets on a lattice case: {"aligned", "deltas", "err"}"""
    import torch
    from text_alignment_amd import train
    _, P, cs = lattice_case(name)
    al, de, err = train.ctc_align_targets(torch.from_numpy(P).cuda(), [len(P)], [cs])
    return {"aligned": al.cpu().numpy(), "deltas": de.cpu().numpy(), "err": err.cpu().numpy()}


DEVICE_NET_KEYS = ("probs", "aligned", "err") + tuple(flat_names())


def device_net(name):
    """LineTrainer.align and .gradients on a network case: per line the arrays of DEVICE_NET_KEYS"""
    from text_alignment_amd import ocr, train
    _, (fwd, rev, W2, codec), lines, codes = net_case(name)
    tr = train.LineTrainer(model=ocr.LineModel(fwd, rev, W2, codec))
    texts = texts_of(codec, codes)
    out = []
    for (al, probs), g in zip(tr.align(lines, texts, want_probs=True), tr.gradients(lines, texts)):
        a = {"probs": probs, "aligned": al, "err": np.asarray([g["error"]]), "W2": g["W2"]}
        for d in ("fwd", "rev"):
            a.update({d + " " + k: g[d][k] for k in R.GATES + R.PEEPS})
        out.append(a)
    return out
