"""Held-out evaluation of line models on MI355X -- what `ocropus-errs` (character error rate) and `ocropus-econf`
(confusions) report, the numbers a user picks a checkpoint by.

The chain is recognise -> decode -> edit distance against the ground truth -> error counts and confusion matrix, all on
the device: the scorer (csrc/ta_errs.hip, `ta_edit_distance`) reads the decoded class codes where the recogniser's
decoder left them, lengths included, so nothing is downloaded between recognition and scoring; one small download at the
end brings six integers per line.  The arithmetic is DESIGN.md section 14.5 (unit-cost Levenshtein, one alignment with a
fixed tie order); PARITY UNPINNED like the rest of section 14 -- ocropy is not available to compare with, the checker of
record is tests/errs_ref.py.
"""
import unicodedata

import numpy as np
import torch

from . import _native
from .ocr import DEFAULT_PRECISION, MAX_CLASSES, MAX_T, LineModel, LineRecognizer, _is_raw_strip

KINDS = {"exact": _native.TA_ERRS_KIND_EXACT, "nospace": _native.TA_ERRS_KIND_NOSPACE}
MAX_TARGET = _native.TA_ERRS_MAX_TARGET
MAX_DECODED = _native.TA_ERRS_MAX_DECODED       # (MAX_T + 1) // 2: two decoded characters are a timestep apart
FIELDS = _native.TA_ERRS_FIELDS                 # errors, n, m, substitutions, insertions, deletions


def _kind(kind):
    if kind not in KINDS:
        raise ValueError("unknown text kind %r: one of %s" % (kind, ", ".join(sorted(KINDS))))
    return KINDS[kind]


def normalise_text(s, kind="exact"):
    """NFC, then the kind's whitespace rule (the two of `ocropus-errs -k` that matter here): "exact" collapses
    whitespace runs to one space and strips both ends, "nospace" removes all whitespace"""
    _kind(kind)
    s = unicodedata.normalize("NFC", s)
    return " ".join(s.split()) if kind == "exact" else "".join(s.split())


def encode_target(codec, s, kind="exact"):
    """class codes of the normalised ground truth; a character outside the codec becomes the one extra code
    len(codec), which no decoded code equals"""
    index = {ch: k for k, ch in enumerate(codec) if k > 0 and ch != ""}
    unknown = len(codec)
    return [index.get(ch, unknown) for ch in normalise_text(s, kind)]


class ErrsResult(object):
    """per_line: (lines, 6) int32 on the host -- errors, n, m, substitutions, insertions, deletions; conf: the
    (No + 1, No + 1) int64 confusion counts on the device (confusions() downloads them); errors, chars, lines, cer:
    the totals as `ocropus-errs` prints them (cer = errors / chars, nan without characters)."""

    def __init__(self, per_line, conf, extra=None):
        self.per_line, self.conf, self.extra = per_line, conf, extra
        self.errors = int(per_line[:, 0].sum(dtype=np.int64)) if len(per_line) else 0
        self.chars = int(per_line[:, 2].sum(dtype=np.int64)) if len(per_line) else 0
        self.lines = int(per_line.shape[0])
        self.cer = self.errors / self.chars if self.chars else float("nan")

    def confusions(self):
        return self.conf.cpu().numpy()

    def confusion_list(self, codec):
        """off-diagonal (count, decoded char, truth char), count descending, then by the two codes; "_" stands for
        nothing and "?" for a character outside the codec, as in `ocropus-econf`"""
        conf = self.confusions()
        no = len(codec)
        xs, ys = np.nonzero(conf)
        rows = sorted((-int(conf[x, y]), int(x), int(y)) for x, y in zip(xs, ys) if x != y)

        def name(c):
            return "_" if c == 0 else ("?" if c == no else codec[c])
        return [(-c, name(x), name(y)) for c, x, y in rows]


class RefusedLineError(RuntimeError):
    """the scoring kernel found a line's device numbers outside the bounds its workspace was sized for and left it
    alone; `per_line` holds every line's tuple (errors = -1 for the refused ones)"""

    def __init__(self, msg, per_line):
        RuntimeError.__init__(self, msg)
        self.per_line = per_line


def _check_targets(T, targets, no):
    """everything score_decoded refuses before the device is touched"""
    if len(T) != len(targets):
        raise ValueError("%d lines but %d targets" % (len(T), len(targets)))
    if not 1 <= no <= MAX_CLASSES:
        raise ValueError("1 .. %d classes" % MAX_CLASSES)
    for t, g in zip(T, targets):
        if t < 0 or t > MAX_T:
            raise ValueError("a line of %d timesteps is outside the 0 .. %d the scorer is sized for" % (t, MAX_T))
        if len(g) > MAX_TARGET:
            raise ValueError("a ground truth of %d characters exceeds the scorer's %d" % (len(g), MAX_TARGET))
        if len(g) and (min(g) < 1 or max(g) > no):
            raise ValueError("target class codes must lie in 1 .. %d" % no)


def score_decoded(dec_c, dec_off, dec_n, T, targets, no, kind="exact", conf=None, check=True, extra=None):
    """Score decoded lines against encoded targets on the device.

    dec_c (int32), dec_off (int64), dec_n (int32): device tensors exactly as ta_decode / ta_decode_summary leave them
    -- line b's codes are dec_c[dec_off[b] : dec_off[b] + dec_n[b]]; dec_n may carry further words behind the lines'.
    T: timesteps per line on the HOST; the workspace is sized from the bound dec_n[b] <= (T[b] + 1) // 2 (two decoded
    characters are at least a timestep apart), the lengths themselves stay on the device.  targets: per line the codes
    of encode_target; no = len(codec).  conf: a (no + 1, no + 1) int64 device tensor to ADD into (several batches, one
    matrix), or None for a fresh one.  extra: an int32 device tensor that rides along in the one download (evaluate():
    the recogniser's status word) and comes back as result.extra.
    One packed upload, one launch, one download.  A line the kernel refused (errors = -1) raises RefusedLineError
    unless check is False."""
    k = _kind(kind)
    T = [int(t) for t in T]
    _check_targets(T, targets, no)
    for name, t, dt in (("dec_c", dec_c, torch.int32), ("dec_off", dec_off, torch.int64), ("dec_n", dec_n, torch.int32)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s device tensor" % (name, dt))
    n = len(T)
    if dec_off.numel() < n or dec_n.numel() < n:
        raise ValueError("dec_off / dec_n hold fewer than %d lines" % n)
    dev = dec_c.device
    nc = no + 1
    if conf is None:
        conf = torch.zeros((nc, nc), dtype=torch.int64, device=dev)
    elif conf.shape != (nc, nc) or conf.dtype != torch.int64 or conf.device != dev or not conf.is_contiguous():
        raise ValueError("conf must be a contiguous (%d, %d) int64 tensor on %s" % (nc, nc, dev))
    if n == 0:
        host = extra.cpu().numpy() if extra is not None else None
        return ErrsResult(np.zeros((0, FIELDS), dtype=np.int32), conf, host)
    lib = _native.lib
    nb = np.asarray([(t + 1) // 2 for t in T], dtype=np.int32)
    m = np.asarray([len(g) for g in targets], dtype=np.int32)
    ws = np.asarray([lib.ta_errs_workspace_bytes(int(a), int(b)) for a, b in zip(nb, m)], dtype=np.int64)
    ws_off = np.zeros(n, dtype=np.int64)
    ws_off[1:] = np.cumsum(ws)[:-1]
    tgt_off = np.zeros(n, dtype=np.int64)
    tgt_off[1:] = np.cumsum(m.astype(np.int64))[:-1]
    flat = np.asarray([c for g in targets for c in g] or [1], dtype=np.int32)
    with torch.cuda.device(dev):
        d_flat, d_toff, d_m, d_nb, d_wsoff = _native.upload_packed([flat, tgt_off, m, nb, ws_off], dev)
        ws_bytes = int(ws.sum())
        work = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        out = torch.empty(n * FIELDS + (extra.numel() if extra is not None else 0), dtype=torch.int32, device=dev)
        _native.check(lib.ta_edit_distance(
            dec_c.data_ptr(), dec_off.data_ptr(), dec_n.data_ptr(), dec_c.numel(), d_flat.data_ptr(), d_toff.data_ptr(),
            d_m.data_ptr(), int(m.sum()), d_nb.data_ptr(), d_wsoff.data_ptr(), n, nc, k, nb.ctypes.data, m.ctypes.data,
            work.data_ptr(), work.numel(), out.data_ptr(), conf.data_ptr(),
            torch.cuda.current_stream(dev).cuda_stream), "ta_edit_distance")
        if extra is not None:
            out[n * FIELDS:] = extra.reshape(-1)
        host = out.cpu().numpy()
    per_line = host[:n * FIELDS].reshape(n, FIELDS)
    if check and (per_line[:, 0] < 0).any():
        bad = np.nonzero(per_line[:, 0] < 0)[0]
        raise RefusedLineError("ta_edit_distance refused line(s) %s on the device (lengths or codes out of bounds)"
                               % ", ".join(str(int(b)) for b in bad[:8]), per_line)
    return ErrsResult(per_line, conf, host[n * FIELDS:] if extra is not None else None)


def _as_recognizer(model, precision, device):
    if isinstance(model, LineRecognizer):
        return model
    if isinstance(model, str):
        from . import model_io
        model = model_io.load_pyrnn(model)
    if not isinstance(model, LineModel):
        raise ValueError("model must be a LineModel, a LineRecognizer or the path of a .pyrnn.gz")
    return LineRecognizer(model, device=device, precision=precision)


def _codec_of(model):
    if isinstance(model, LineRecognizer):
        return model.model.codec
    return model.codec


def _check_call(lines, texts, kind):
    _kind(kind)
    if len(lines) != len(texts):
        raise ValueError("%d lines but %d texts" % (len(lines), len(texts)))


def _encode_all(codec, texts, kind):
    targets = [encode_target(codec, t, kind) for t in texts]
    for g in targets:
        if len(g) > MAX_TARGET:
            raise ValueError("a ground truth of %d characters exceeds the scorer's %d" % (len(g), MAX_TARGET))
    return targets


def _evaluate(rec, lines, targets, kind):
    codec = rec.model.codec
    no = len(codec)
    with torch.cuda.device(rec.device):
        st = rec.prepare(lines)
        rec.run(st)
        if st["n"] == 0:
            res = ErrsResult(np.zeros((0, FIELDS), dtype=np.int32),
                             torch.zeros((no + 1, no + 1), dtype=torch.int64, device=rec.device))
        else:
            res = score_decoded(st["dec_c"], st["row_off"], st["dec_n"], st["T_host"], targets, no, kind,
                                extra=st["dec_n"][-1:])
            rec.check_status(res.extra)
    return {"errors": res.errors, "chars": res.chars, "lines": res.lines, "cer": res.cer, "per_line": res.per_line,
            "confusions": res.confusion_list(codec)}


def evaluate(model, lines, texts, kind="exact", precision=DEFAULT_PRECISION, device="cuda"):
    """Score a model on held-out lines.  model: a LineModel, a LineRecognizer or the path of a .pyrnn.gz; lines:
    prepared (T, 48) rows or raw uint8 strips, as LineRecognizer.prepare takes them; texts: their ground truth.
    Returns {"errors", "chars", "lines", "cer", "per_line", "confusions"}: the totals, the (lines, 6) int32 tuples
    (errors, n, m, substitutions, insertions, deletions) and the off-diagonal confusions as (count, decoded char, truth
    char), most frequent first ("_" = nothing, "?" = not in the codec).  ValueError -- a length mismatch, an unknown
    kind, a ground truth over the limit -- before the device is touched."""
    _check_call(lines, texts, kind)
    if isinstance(model, str):
        from . import model_io
        model = model_io.load_pyrnn(model)
    targets = _encode_all(_codec_of(model), texts, kind)
    return _evaluate(_as_recognizer(model, precision, device), lines, targets, kind)


def evaluate_models(models, lines, texts, kind="exact", precision=DEFAULT_PRECISION, device="cuda"):
    """evaluate() for several models on the same lines: a list of its dicts.  Raw strips are normalised ONCE on the
    device and the prepared rows handed to every model's recogniser."""
    _check_call(lines, texts, kind)
    loaded = []
    for mdl in models:
        if isinstance(mdl, str):
            from . import model_io
            mdl = model_io.load_pyrnn(mdl)
        loaded.append((mdl, _encode_all(_codec_of(mdl), texts, kind)))
    if not loaded:
        return []
    recs = [_as_recognizer(mdl, precision, device) for mdl, _ in loaded]
    lines = list(lines)
    if lines and all(_is_raw_strip(ln) for ln in lines) and len(recs) > 1:
        from . import lineest_gpu
        dev = recs[0].device
        with torch.cuda.device(dev):
            x, T, _ = lineest_gpu.normalize_strips(lines, device=dev)
            lines = _device_rows(x, T)
    return [_evaluate(rec, lines, targets, kind) for rec, (_, targets) in zip(recs, loaded)]


def _device_rows(x, T):
    """the normaliser's rows (sum T, 48) on the device as the per-line spans LineRecognizer.prepare reads in place"""
    from .page import RowBlock
    block = RowBlock(x.shape[0], "device", x.device)
    block.tensor[:x.shape[0]] = x
    spans, r = [], 0
    for t in T:
        spans.append(block.span(r, r + int(t)))
        r += int(t)
    return spans
