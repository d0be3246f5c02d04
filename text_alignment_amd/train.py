"""Training of the line recogniser on MI355X -- the in-process replacement of `ocropus-rtrain`, the other half of the
reference's OCR workflow (reference README.md, "Training a New OCRopus model": every new manuscript needs a model).

The arithmetic is ocropy 1.3.3's `SeqRecognizer.trainSequence` in float64 as restated in DESIGN.md section 14: forward
pass of SURVEY.md Appendix B.3 / B.4, CTC alignment of the outputs with the target text, back-propagation through time,
momentum update.  PARITY UNPINNED, like the recogniser: ocropy is a third-party package that is not available to
compare with; the checker of record is tests/train_ref.py.

The sequential parts are HIP kernels (csrc/ta_train.hip: `ta_lstm_train_forward`, `ta_ctc_align`,
`ta_lstm_train_backward`); the products with no dependence between timesteps (input projection, the output layer's
error, the time-summed outer products) and the elementwise update are float64 torch operations on the same stream.
"""
import numpy as np
import torch

from . import _native
from .ocr import MAX_CLASSES, MAX_T, NI, NS, THRESHOLD, LineModel, _is_raw_strip

GATES = ("WGI", "WGF", "WGO", "WCI")
PEEPS = ("WIP", "WFP", "WOP")
NA = 1 + NI + NS
MAX_TARGET = (_native.TA_CTC_MAX_STATES - 1) // 2       # characters of one target text: 2 L + 1 states (csrc/ta_train.hip)
STATE_FIELDS = _native.TA_TRAIN_STATE_FIELDS


def make_codec(charset):
    """class 0 = "", 1 = " ", 2 = "~", then the sorted remaining characters of `charset` (a string or strings)"""
    chars = set()
    for s in ([charset] if isinstance(charset, str) else charset):
        chars.update(s)
    return ["", " ", "~"] + sorted(chars - {" ", "~"})


def fresh_model(charset, seed=0):
    """a LineModel with every weight drawn uniformly in (-0.1, 0.1) from numpy's default_rng(seed): the four gate
    matrices and three peepholes of the forward LSTM, those of the reversed one, then the output layer"""
    codec = make_codec(charset)
    rng = np.random.default_rng(seed)

    def lstm():
        d = {k: rng.uniform(-0.1, 0.1, size=(NS, NA)) for k in GATES}
        d.update({k: rng.uniform(-0.1, 0.1, size=(NS,)) for k in PEEPS})
        return d
    fwd, rev = lstm(), lstm()
    return LineModel(fwd, rev, rng.uniform(-0.1, 0.1, size=(len(codec), 1 + 2 * NS)), codec)


def encode_text(codec, text):
    """class codes of a target text; a character outside the codec is a ValueError"""
    index = {ch: k for k, ch in enumerate(codec) if k > 0 and ch != ""}
    out = []
    for ch in text:
        if ch not in index:
            raise ValueError("character %r is not in the model's codec" % ch)
        out.append(index[ch])
    return out


def check_target(T, L):
    """the limits of one (line, text) pair, before anything reaches the device"""
    if T > MAX_T:
        raise ValueError("a line of %d timesteps is longer than the %d the model takes" % (T, MAX_T))
    if 2 * L + 1 > T:
        raise ValueError("a text of %d characters (%d CTC states) does not fit a line of %d timesteps" % (L, 2 * L + 1, T))
    if L > MAX_TARGET:
        raise ValueError("a text of %d characters exceeds the CTC kernel's %d" % (L, MAX_TARGET))


def translate_back(outputs, threshold=THRESHOLD):
    """SURVEY.md Appendix B.5 on the host: class of the maximum of every run of timesteps with outputs[t, 0] < threshold"""
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


def _batch_meta(T, labels, no, device):
    """device copies of a batch's per-line numbers (one transfer) and the host numbers the C ABI wants"""
    n = len(T)
    T32 = np.asarray(T, dtype=np.int32)
    L32 = np.asarray([len(l) for l in labels], dtype=np.int32)
    for t, l in zip(T32, L32):
        check_target(int(t), int(l))
    row_off = np.zeros(n, dtype=np.int64)
    row_off[1:] = np.cumsum(T32.astype(np.int64))[:-1]
    lab_off = np.zeros(n, dtype=np.int64)
    lab_off[1:] = np.cumsum(L32.astype(np.int64))[:-1]
    flat = np.asarray([c for l in labels for c in l] or [0], dtype=np.int32)
    if flat.min() < 0 or flat.max() >= no or (int(L32.sum()) and flat.min() < 1):
        raise ValueError("target class codes must lie in 1 .. %d" % (no - 1))
    ws = np.asarray([_native.lib.ta_ctc_workspace_bytes(int(t), int(l), no) for t, l in zip(T32, L32)], dtype=np.int64)
    if (ws < 0).any():
        raise ValueError("a line's sizes are outside what ta_ctc_align takes")
    ws_off = np.zeros(n, dtype=np.int64)
    ws_off[1:] = np.cumsum(ws // 8)[:-1]
    d = _native.upload_packed([row_off, T32, flat, lab_off, L32, ws_off], device)
    return {"n": n, "T": T32, "L": L32, "row_off": row_off, "rows": int(T32.sum()), "nlabels": int(L32.sum()),
            "ws_bytes": int(ws.sum()), "d_row_off": d[0], "d_T": d[1], "d_labels": d[2], "d_lab_off": d[3], "d_L": d[4],
            "d_ws_off": d[5]}


def _ctc(probs, meta, no):
    dev = probs.device
    rows = meta["rows"]
    ws = torch.empty(max(meta["ws_bytes"] // 8, 1), dtype=torch.float64, device=dev)
    aligned = torch.empty((rows, no), dtype=torch.float64, device=dev)
    deltas = torch.empty((rows, no), dtype=torch.float64, device=dev)
    err = torch.empty(meta["n"], dtype=torch.float64, device=dev)
    _native.check(_native.lib.ta_ctc_align(
        probs.data_ptr(), meta["d_row_off"].data_ptr(), meta["d_T"].data_ptr(), meta["d_labels"].data_ptr(),
        meta["d_lab_off"].data_ptr(), meta["d_L"].data_ptr(), meta["d_ws_off"].data_ptr(), meta["n"], no, rows,
        max(meta["nlabels"], 1), meta["T"].ctypes.data, meta["L"].ctypes.data, ws.data_ptr(), ws.numel() * 8,
        aligned.data_ptr(), deltas.data_ptr(), err.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "ta_ctc_align")
    return aligned, deltas, err


def ctc_align_targets(probs, T, labels):
    """CTC alignment on the device.  probs: float64 device tensor (sum T, No), the softmax
    outputs of the lines one after the other; T: timesteps per line; labels: per line the target class codes.
    Returns (aligned, deltas, err): (sum T, No), (sum T, No) = aligned - probs, (lines,) = sum of deltas^2 per line.
    ValueError for a target whose 2 L + 1 states do not fit its line."""
    if probs.dtype != torch.float64 or probs.dim() != 2 or not probs.is_cuda or not probs.is_contiguous():
        raise ValueError("probs must be a contiguous float64 device tensor (rows, classes)")
    no = int(probs.shape[1])
    if len(T) != len(labels) or int(np.sum(T)) != probs.shape[0]:
        raise ValueError("T and labels describe other lines than probs holds")
    if not 2 <= no <= MAX_CLASSES:
        raise ValueError("2 .. %d classes" % MAX_CLASSES)
    if len(T) == 0:
        z = torch.zeros((0, no), dtype=torch.float64, device=probs.device)
        return z, z.clone(), torch.zeros(0, dtype=torch.float64, device=probs.device)
    with torch.cuda.device(probs.device):
        return _ctc(probs, _batch_meta(T, labels, no, probs.device), no)


class LineTrainer(object):
    """Trains a line model: `LineTrainer(charset=...)` starts a fresh one (weights uniform in (-0.1, 0.1), seeded),
    `LineTrainer(model=...)` continues from a LineModel (e.g. model_io.load_pyrnn).

    train(lines, texts) runs one update per `lines_per_update` lines, in order: ds = momentum ds + lrate DW; W += ds for
    every weight array (ocropy's Network.update; its defaults lrate 1e-4, momentum 0.9).  lines_per_update = 1 is
    ocropy's schedule.  lines_per_update = B > 1 is a DEPARTURE from ocropy: the gradients of B lines are computed
    against the same weights, summed and applied once -- B lines per launch is what fills the GPU.

    distort = D (pixels; None: off, the default) makes train() put every batch of raw strips through
    augment.distort_strips(distort=D, dsigma=dsigma) before the normaliser: ocropy's random line distortion, on the
    device (3.0 and 10.0 are `rdistort`'s defaults, unpinned).  The noise key is `seed`, the
    counter of a line the number of lines train() has seen before it (`lines_seen`), so a run is reproducible from
    `seed`.  gradients(), align() and evaluate() never distort."""

    def __init__(self, model=None, charset=None, device="cuda", lrate=1e-4, momentum=0.9, lines_per_update=1, seed=0,
                 distort=None, dsigma=10.0):
        if (model is None) == (charset is None):
            raise ValueError("pass either a model to continue from or a charset for a fresh one")
        if int(lines_per_update) < 1:
            raise ValueError("lines_per_update must be at least 1")
        if not lrate > 0 or not 0 <= momentum < 1:
            raise ValueError("lrate must be positive and momentum in [0, 1)")
        if distort is not None:
            from . import augment
            distort, dsigma = augment.check_params(distort, dsigma)
        self.distort, self.dsigma, self.seed, self.lines_seen = distort, float(dsigma), int(seed), 0
        if model is None:
            model = fresh_model(charset, seed)
        self.codec = list(model.codec)
        self.no = model.no
        self.lrate, self.momentum, self.lines_per_update = float(lrate), float(momentum), int(lines_per_update)
        self._device_arg = device
        self._host = (np.stack([np.stack([np.asarray(w[k], dtype=np.float64) for k in GATES]) for w in (model.fwd, model.rev)]),
                      np.stack([np.stack([np.asarray(w[k], dtype=np.float64) for k in PEEPS]) for w in (model.fwd, model.rev)]),
                      np.array(model.W2, dtype=np.float64))
        self.W = None

    # ---- device state ---------------------------------------------------------------------------------------------
    def _ensure_device(self):
        if self.W is not None:
            return
        if not torch.cuda.is_available():
            raise RuntimeError("text_alignment_amd needs an AMD GPU (MI355X); there is no CPU fallback")
        self.device = torch.device(self._device_arg)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.W, self.peep, self.W2 = (torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in self._host)
        self.ds = [torch.zeros_like(a) for a in (self.W, self.peep, self.W2)]

    def model(self):
        """the current weights as a LineModel (what LineRecognizer and model_io.save_pyrnn take)"""
        W, peep, W2 = self._host if self.W is None else (a.cpu().numpy() for a in (self.W, self.peep, self.W2))
        nets = []
        for d in range(2):
            w = {k: W[d, g].copy() for g, k in enumerate(GATES)}
            w.update({k: peep[d, q].copy() for q, k in enumerate(PEEPS)})
            nets.append(w)
        return LineModel(nets[0], nets[1], W2.copy(), self.codec)

    # ---- one batch against the current weights --------------------------------------------------------------------
    def _rows(self, lines, first_counter=None):
        """(x float64 (rows, 48) on the device, T per line): prepared rows as they are, raw uint8 strips through the
        device normaliser (lineest_gpu), as LineRecognizer.prepare accepts them -- distorted before it when train()
        passes the batch's first noise counter"""
        raw = [_is_raw_strip(ln) for ln in lines]
        if all(raw) and lines:
            from . import lineest_gpu
            if first_counter is not None:
                from . import augment
                lines = augment.distort_strips(list(lines), self.distort, self.dsigma, seed=self.seed % 2 ** 64,
                                               first_counter=first_counter, device=self.device)
            x, T, _ = lineest_gpu.normalize_strips(list(lines), device=self.device)
            return x.to(torch.float64), [int(t) for t in T]
        if any(raw):
            raise ValueError("a batch is either all prepared lines or all raw uint8 strips")
        for ln in lines:
            if ln.ndim != 2 or ln.shape[1] != NI:
                raise ValueError("a prepared line must have shape (T, 48)")
        T = [int(ln.shape[0]) for ln in lines]
        x = np.concatenate([np.asarray(ln, dtype=np.float64) for ln in lines], axis=0)
        return torch.from_numpy(np.ascontiguousarray(x)).to(self.device), T

    def _check(self, lines, texts, distorting=False):
        """everything that can be refused before the device is touched"""
        if len(lines) != len(texts):
            raise ValueError("%d lines but %d texts" % (len(lines), len(texts)))
        if distorting and not all(_is_raw_strip(ln) for ln in lines):
            raise ValueError("distort is set: train() takes raw uint8 strips, not prepared (T, 48) lines")
        labels = [encode_text(self.codec, t) for t in texts]
        for ln, l in zip(lines, labels):
            if not _is_raw_strip(ln) and getattr(ln, "ndim", 0) == 2:
                check_target(int(ln.shape[0]), len(l))
        return labels

    def _pass(self, lines, labels, backward=True, first_counter=None):
        """forward, alignment and (backward) BPTT of a batch against the current weights; everything stays on the
        device.  Returns a dict of the batch's tensors."""
        self._ensure_device()
        lib = _native.lib
        dev = self.device
        with torch.cuda.device(dev):
            x, T = self._rows(lines, first_counter)
            meta = _batch_meta(T, labels, self.no, dev)
            rows, n = meta["rows"], meta["n"]
            stream = torch.cuda.current_stream(dev).cuda_stream
            x1 = torch.cat([torch.ones((rows, 1), dtype=torch.float64, device=dev), x], dim=1)
            gx = x1 @ self.W[:, :, :, :1 + NI].reshape(8 * NS, 1 + NI).t()             # [rows][dir][gate][unit]
            states = torch.empty((rows, 2, STATE_FIELDS, NS), dtype=torch.float64, device=dev)
            hout = torch.empty((rows, 2 * NS), dtype=torch.float64, device=dev)
            probs = torch.empty((rows, self.no), dtype=torch.float64, device=dev)
            max_T = int(meta["T"].max())
            _native.check(lib.ta_lstm_train_forward(
                gx.data_ptr(), meta["d_row_off"].data_ptr(), meta["d_T"].data_ptr(), n, max_T, rows, self.W.data_ptr(),
                self.peep.data_ptr(), self.W2.data_ptr(), self.no, states.data_ptr(), hout.data_ptr(), probs.data_ptr(),
                stream), "ta_lstm_train_forward")
            aligned, deltas, err = _ctc(probs, meta, self.no)
            out = {"meta": meta, "probs": probs, "aligned": aligned, "deltas": deltas, "err": err}
            if not backward:
                return out
            dy = deltas @ self.W2[:, 1:]
            gate_err = torch.empty((rows, 2, 4 * NS), dtype=torch.float64, device=dev)
            dpeep = torch.empty((n, 2, 3, NS), dtype=torch.float64, device=dev)
            _native.check(lib.ta_lstm_train_backward(
                dy.data_ptr(), states.data_ptr(), meta["d_row_off"].data_ptr(), meta["d_T"].data_ptr(), n, max_T, rows,
                self.W.data_ptr(), self.peep.data_ptr(), gate_err.data_ptr(), dpeep.data_ptr(), stream),
                "ta_lstm_train_backward")
            out.update(x1=x1, states=states, hout=hout, gate_err=gate_err, dpeep=dpeep)
            return out

    @staticmethod
    def _sums(p, r0, r1, b0, b1):
        """(DW, Dpeep, DW2) of rows r0 .. r1 = lines b0 .. b1 of a pass: the time-summed outer products"""
        ge, x1 = p["gate_err"][r0:r1], p["x1"][r0:r1]
        DW = torch.stack([ge[:, d].t() @ torch.cat([x1, p["states"][r0:r1, d, 5]], dim=1) for d in range(2)])
        ones = x1[:, :1]
        DW2 = p["deltas"][r0:r1].t() @ torch.cat([ones, p["hout"][r0:r1]], dim=1)
        return DW.reshape(2, 4, NS, NA), p["dpeep"][b0:b1].sum(dim=0), DW2

    def _finish(self, p):
        """host side of a pass: per line the error and the decoded text of the outputs"""
        meta = p["meta"]
        probs, err = p["probs"].cpu().numpy(), p["err"].cpu().numpy()
        if np.isnan(err).any():
            raise RuntimeError("ta_ctc_align refused a line on the device (sizes out of bounds)")
        res = []
        for b in range(meta["n"]):
            r0 = int(meta["row_off"][b])
            dec = translate_back(probs[r0:r0 + int(meta["T"][b])])
            res.append({"error": float(err[b]), "decoded": "".join(self.codec[c] for c in dec)})
        return res

    # ---- public ---------------------------------------------------------------------------------------------------
    def train(self, lines, texts):
        """One update per `lines_per_update` lines, in order.  Returns per line {"error": sum of deltas^2, "decoded":
        translate_back of the outputs BEFORE the line's update}."""
        labels = self._check(lines, texts, distorting=self.distort is not None)
        res, B = [], self.lines_per_update
        for a in range(0, len(lines), B):
            p = self._pass(lines[a:a + B], labels[a:a + B],
                           first_counter=None if self.distort is None else self.lines_seen)
            self.lines_seen += len(lines[a:a + B])
            meta = p["meta"]
            grads = self._sums(p, 0, meta["rows"], 0, meta["n"])
            for w, ds, g in zip((self.W, self.peep, self.W2), self.ds, grads):
                ds.mul_(self.momentum).add_(g, alpha=self.lrate)
                w.add_(ds)
            res.extend(self._finish(p))
        return res

    def gradients(self, lines, texts):
        """Per line the derivative of -CE with respect to every weight array (no update): a list of dicts with "fwd"
        and "rev" (WGI .. WCI (100, 149), WIP WFP WOP (100,)), "W2" (No, 201), "error" and "decoded"."""
        labels = self._check(lines, texts)
        if not lines:
            return []
        p = self._pass(lines, labels)
        meta = p["meta"]
        res = self._finish(p)
        for b in range(meta["n"]):
            r0 = int(meta["row_off"][b])
            DW, Dp, DW2 = (g.cpu().numpy() for g in self._sums(p, r0, r0 + int(meta["T"][b]), b, b + 1))
            for d, name in enumerate(("fwd", "rev")):
                res[b][name] = {k: DW[d, g] for g, k in enumerate(GATES)}
                res[b][name].update({k: Dp[d, q] for q, k in enumerate(PEEPS)})
            res[b]["W2"] = DW2
        return res

    def evaluate(self, lines, texts, kind="exact"):
        """Held-out score of the CURRENT weights (errs.evaluate on self.model(): recognise, decode and edit distance on
        the device): {"errors", "chars", "lines", "cer", "per_line", "confusions"}.  Never
        distorts, never updates."""
        from . import errs
        return errs.evaluate(self.model(), lines, texts, kind=kind, device=self._device_arg)

    def train_from_pages(self, pages, transcripts, seq_align_params=None, min_agreement=0.9):
        """Train on page images and page transcripts, with no line-level ground truth: the pages' lines are recognised
        with the CURRENT weights (never distorted), every page's OCR is aligned with its transcript, the alignment is
        cut into per-line texts on the device (harvest.harvest_pages) and train() runs on the
        accepted lines, in line order.  Returns the HarvestResult (every line with its reason and counts); its
        `trained` holds what train() returned.  Arguments as harvest_pages takes them."""
        from . import harvest, ocr
        harvest.agreement_ratio(min_agreement)
        rec = ocr.LineRecognizer(self.model(), device=self._device_arg)
        res = harvest.harvest_pages(pages, transcripts, rec, seq_align_params, min_agreement)
        pairs = list(res.accepted())
        res.trained = self.train([s for s, _ in pairs], [t for _, t in pairs])
        return res

    def align(self, lines, texts, want_probs=False):
        """Per line the aligned targets (T, No) of the current weights' outputs; want_probs: (aligned, probs) pairs."""
        labels = self._check(lines, texts)
        if not lines:
            return []
        p = self._pass(lines, labels, backward=False)
        meta = p["meta"]
        al, pr = p["aligned"].cpu().numpy(), p["probs"].cpu().numpy()
        if np.isnan(p["err"].cpu().numpy()).any():
            raise RuntimeError("ta_ctc_align refused a line on the device (sizes out of bounds)")
        sl = [slice(int(meta["row_off"][b]), int(meta["row_off"][b]) + int(meta["T"][b])) for b in range(meta["n"])]
        return [(al[s], pr[s]) if want_probs else al[s] for s in sl]
