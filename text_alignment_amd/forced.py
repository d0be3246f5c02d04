"""Forced alignment: where every character of a line's KNOWN text sits in the recogniser's output.

The page path places a syllable only where the greedy decoder emitted characters for it.  The recogniser knows better
than its decode: it holds a probability for every class at every timestep, and since harvesting (harvest.py) the package
knows which piece of the page's transcript belongs to which text line.  `forced_alignment` finds, per line, the best CTC
path through exactly that text (csrc/ta_forced.hip: `ta_forced_align`; integers only, the rule is DESIGN.md section 14.7
and the checker of record tests/forced_ref.py) and reads off per character the timesteps it occupies and its peak.
`align_lines` does it for line images with known texts (`ocropus-rpred --llocs` for a known text: tools/rforced.py);
`refine_pages` runs recognise -> align -> harvest -> forced alignment for a batch of pages and gives every transcript
character of an accepted line a box of its own, so every syllable on such a line gets one -- also those the decoder lost.
`Refining` is the same refinement inside the page pipeline (alignToOCR.process_batch(..., refine=True)): harvest,
`ta_forced_align_lines` and `ta_refine_columns` (csrc/ta_refine.hip; checker tests/refine_ref.py) behind a chunk's aligner
launch, one download, no look at the harvest table from the host.
How many lines of real manuscript pages get refined has NOT been measured.
"""
import numpy as np
import torch

from . import _native

FIELDS = 3                      # TA_FORCED_FIELDS: t_first, t_last, t_peak
MAX_TARGET = 1023               # TA_FORCED_MAX_TARGET
OK, BOUNDS, LABEL = 0, 1, 2
STATUS = {0: "ok", 1: "the line's own numbers are out of bounds", 2: "a label outside 1 .. no - 1"}


def _host_ints(x, dtype, name):
    a = np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=dtype).reshape(-1)
    if a.size and a.min() < 0:
        raise ValueError("%s must not be negative" % name)
    return a


def forced_alignment(probs, row_off, T, labels, lab_off, L, host=False, _fill=None):
    """The device-level call, on torch's current stream; nothing is waited for.

    probs: contiguous float32 device tensor (rows, no), what the recogniser's output layer wrote; line b owns the rows
    row_off[b] .. + T[b] and the labels labels[lab_off[b] .. + L[b]] (class codes 1 .. no - 1).  row_off, T, lab_off, L:
    host integers per line; labels: host integers or an int32 device tensor.  Returns (frames (labels, 3) int32 =
    t_first, t_last, t_peak per label, score (lines,) int64, status (lines,) int32) as device tensors, or with host=True
    a dict of numpy arrays.  ValueError for sizes that do not fit each other or the kernel (L < 1, 2 L + 1 > T,
    L > 1023, T > 5000, classes outside 2 .. 128).  (_fill: a byte value every output and the workspace are filled with
    before the launch -- for tests.)"""
    if not (isinstance(probs, torch.Tensor) and probs.is_cuda and probs.dtype == torch.float32 and probs.dim() == 2 and
            probs.is_contiguous()):
        raise ValueError("probs must be a contiguous float32 device tensor (rows, classes)")
    rows, no = int(probs.shape[0]), int(probs.shape[1])
    if not 2 <= no <= 128:
        raise ValueError("2 .. 128 classes")
    row_off, lab_off = _host_ints(row_off, np.int64, "row_off"), _host_ints(lab_off, np.int64, "lab_off")
    T32, L32 = _host_ints(T, np.int32, "T"), _host_ints(L, np.int32, "L")
    n = len(T32)
    if not (len(row_off) == len(lab_off) == len(L32) == n):
        raise ValueError("row_off, T, lab_off and L need one entry per line")
    dev = probs.device
    lib = _native.lib
    if isinstance(labels, torch.Tensor) and labels.is_cuda:
        if labels.dtype != torch.int32 or not labels.is_contiguous():
            raise ValueError("labels on the device must be a contiguous int32 tensor")
        d_labels, nlabels = labels, int(labels.numel())
    else:
        d_labels, nlabels = None, None
        labels = _host_ints(labels, np.int32, "labels")
        nlabels = len(labels)
    ws = np.asarray([lib.ta_forced_workspace_bytes(int(t), int(l)) for t, l in zip(T32, L32)], dtype=np.int64)
    if (ws < 0).any():
        b = int(np.nonzero(ws < 0)[0][0])
        raise ValueError("line %d: a text of %d characters and %d timesteps is outside what ta_forced_align takes "
                         "(1 <= L <= %d, 2 L + 1 <= T <= 5000)" % (b, int(L32[b]), int(T32[b]), MAX_TARGET))
    if n and ((row_off + T32 > rows).any() or (lab_off + L32 > nlabels).any()):
        raise ValueError("a line's rows or labels lie outside probs / labels")
    ws_off = np.zeros(n, dtype=np.int64)
    ws_off[1:] = np.cumsum(ws)[:-1]
    ws_bytes = int(ws.sum())
    with torch.cuda.device(dev):
        frames = torch.empty((max(nlabels, 1), FIELDS), dtype=torch.int32, device=dev)
        score = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        if n:
            up = [row_off, T32, lab_off, L32, ws_off] + ([labels if nlabels else np.zeros(1, np.int32)] if d_labels is None else [])
            d = _native.upload_packed(up, dev)
            if d_labels is None:
                d_labels = d[5]
            work = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
            if _fill is not None:
                for t in (frames, score, status, work):
                    t.view(torch.uint8).fill_(_fill)
            _native.check(lib.ta_forced_align(
                probs.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d_labels.data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                d[4].data_ptr(), n, no, rows, nlabels, T32.ctypes.data, L32.ctypes.data, work.data_ptr(), ws_bytes,
                frames.data_ptr(), score.data_ptr(), status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                "ta_forced_align")
            work.record_stream(torch.cuda.current_stream(dev))
        frames, score, status = frames[:nlabels], score[:n], status[:n]
        if host:
            return {"frames": frames.cpu().numpy(), "score": score.cpu().numpy(), "status": status.cpu().numpy()}
        return frames, score, status


def _recognizer(model_or_recogniser):
    from . import alignToOCR as atocr
    return atocr._recognizer_for(model_or_recogniser)


def align_lines(model_or_recogniser, lines, texts, want_run=False):
    """Recognise the lines (prepared (T, 48) rows or raw uint8 strips, as LineRecognizer.prepare takes them), keep the
    probabilities and align each with its text.  Returns per line ([(char, t_first, t_last, t_peak, x)], score): x is the
    .llocs position of t_peak, (t_peak - pad) raw_width / (T - 2 pad) in raw strip pixels.  ValueError for a character
    outside the model's codec or a text whose 2 L + 1 states exceed its line's timesteps.  want_run: also return what the
    alignment ran on, {"probs" (the device tensor), "row_off", "T"} -- for checking it."""
    from . import ocr, train
    rec = _recognizer(model_or_recogniser)
    lines, texts = list(lines), list(texts)
    if len(lines) != len(texts):
        raise ValueError("%d lines but %d texts" % (len(lines), len(texts)))
    codec = rec.model.codec
    labels = [train.encode_text(codec, tx) for tx in texts]
    if not lines:
        return ([], None) if want_run else []
    with torch.cuda.device(rec.device):
        st = rec.prepare(lines)
        T = np.asarray(st["T_host"], dtype=np.int64)[:len(lines)]
        for b, (t, l) in enumerate(zip(T, labels)):
            if len(l) < 1:
                raise ValueError("line %d has no text" % b)
            if 2 * len(l) + 1 > t:
                raise ValueError("line %d: a text of %d characters (%d CTC states) does not fit a line of %d timesteps"
                                 % (b, len(l), 2 * len(l) + 1, t))
        rec.run(st, want_probs=True, decode=False)
        L = np.asarray([len(l) for l in labels], dtype=np.int64)
        lab_off = np.concatenate([[0], np.cumsum(L)[:-1]])
        got = forced_alignment(st["probs"], st["row_start_host"][:len(lines)], T, np.concatenate(labels), lab_off, L, host=True)
    bad = np.nonzero(got["status"])[0]
    if bad.size:
        raise RuntimeError("ta_forced_align refused line %d on the device: %s" % (int(bad[0]), STATUS.get(int(got["status"][bad[0]]), "?")))
    widths = [int(ln.shape[1]) if ocr._is_raw_strip(ln) else None for ln in lines]     # a raw strip's own width
    out = []
    for b in range(len(lines)):
        fr = got["frames"][lab_off[b]:lab_off[b] + L[b]]
        raw_w = float(widths[b]) if widths[b] is not None else float(T[b] - 2 * ocr.PAD)
        scale = raw_w / (T[b] - 2 * ocr.PAD)
        out.append(([(ch, int(f[0]), int(f[1]), int(f[2]), (int(f[2]) - ocr.PAD) * scale) for ch, f in zip(texts[b], fr)],
                    int(got["score"][b])))
    if want_run:
        return out, {"probs": st["probs"], "row_off": np.asarray(st["row_start_host"][:len(lines)]), "T": T}
    return out


# ---- boxes under refinement (the per-character rule of record is tests/forced_ref.py) --------

def refine_columns(ops, idx, o_line, lines):
    """One page's alignment columns with every refined line's run replaced.  ops: the columns (0 pair, 1 transcript
    character alone, 2 OCR character alone); idx: per OCR character of the columns its row of the box array; o_line: per
    OCR character its text line; lines: [(line, t_first, L, first new box row)] of the page's refined lines, ascending.
    A refined line owns the columns from its first to its last OCR-carrying column: they become op-1 columns for the
    transcript characters in front of the kept range t_first .. + L, L pair columns with the new box rows, and op-1
    columns for the rest.  Returns (ops, idx)."""
    ops, idx, o_line = np.asarray(ops, dtype=np.uint8), np.asarray(idx, dtype=np.int64), np.asarray(o_line)
    if not lines:
        return ops, idx
    has_t = ops != 2
    col_of_o = np.flatnonzero(ops != 1)
    t_before = np.cumsum(has_t) - has_t                  # transcript characters in front of each column
    new_ops, new_idx, c_done, j_done = [], [], 0, 0
    for line, t_first, L, row in lines:
        js = np.flatnonzero(o_line == line)
        jlo, jhi = int(js[0]), int(js[-1])
        c0, c1 = int(col_of_o[jlo]), int(col_of_o[jhi])
        ta, tb = int(t_before[c0]), int(t_before[c1]) + int(has_t[c1])
        if not (jhi - jlo + 1 == len(js) and c0 >= c_done and ta <= t_first and t_first + L <= tb):
            raise ValueError("line %d: its kept characters are not inside the columns of its OCR characters" % line)
        new_ops += [ops[c_done:c0], np.ones(t_first - ta, np.uint8), np.zeros(L, np.uint8), np.ones(tb - t_first - L, np.uint8)]
        new_idx += [idx[j_done:jlo], np.arange(row, row + L, dtype=np.int64)]
        c_done, j_done = c1 + 1, jhi + 1
    new_ops.append(ops[c_done:])
    new_idx.append(idx[j_done:])
    return np.concatenate(new_ops), np.concatenate(new_idx)


def peak_boxes(t_peak, L, T, raw_w, x_min, y_min, y_max, pad):
    """the boxes the page path's character-box construction yields for the entries (t_peak[i], .) of each line: x =
    (t - pad) raw_w / (T - 2 pad), one decimal, round half to even, previous position -> own position, the strip's
    y_min .. y_max.  t_peak: the lines' peaks one after the other; the rest per line.  Returns [sum L, 4]."""
    from . import page_batch as pb
    L = np.asarray(L, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(L)[:-1]]) if len(L) else np.zeros(0, np.int64)
    t_peak = np.ascontiguousarray(t_peak, dtype=np.int32)
    _, _, boxes = pb.chars_of_batch(t_peak, np.zeros(len(t_peak), np.int32), L, off, T, raw_w, x_min, y_min, y_max,
                                    np.zeros(1, np.int64), pad)       # one class that is kept: nothing is dropped
    return boxes


# ---- the refinement inside the page pipeline: device-resident from the aligner's launch to ONE download -------------------

REFINE_STATUS = {0: "ok", 1: "the harvest refused the page", 2: "the page's own numbers are out of bounds",
                 3: "line indices decrease or leave the page, or the columns disagree with the page's sizes",
                 4: "a line's kept characters are not inside the columns of its OCR characters"}


def refine_checks(seq_align_params, recognisers, min_agreement):
    """what refine_pages refuses, before any GPU work: ValueError for a scoring callable or non-integral numbers, a codec
    with multi-character entries or without the space as class 1, a min_agreement agreement_ratio rejects.  Returns the
    ratio (num, den)."""
    from . import harvest, page_batch as pb, textSeqCompare as tsc
    ratio = harvest.agreement_ratio(min_agreement)
    if tsc.integer_scoring(seq_align_params) is None:
        raise ValueError("refine=True needs the integer aligner: no scoring callable, integral scoring numbers")
    for rec in recognisers:
        if pb.codec_code_points(rec.model.codec) is None:
            raise ValueError("refine=True needs a recogniser codec of single characters")
        harvest.transcript_classes(rec.model.codec, "")
    return ratio


def line_caps(T, line_first, transcripts):
    """per chunk line the longest text it can receive: min((T - 1) / 2, MAX_TARGET, its page's transcript characters)"""
    T = np.asarray(T, dtype=np.int64)
    per_page = np.asarray([len(tr) for tr in transcripts], dtype=np.int64)
    page_len = np.repeat(per_page, np.diff(np.asarray(line_first, dtype=np.int64)))
    return np.maximum(np.minimum(np.minimum((T - 1) // 2, MAX_TARGET), page_len), 0).astype(np.int32)


def workspace_pieces(T, caps):
    """(ws_off int64 per line, total bytes): line q's piece holds the moves of any text of at most caps[q] characters
    (ta_forced_workspace_bytes never decreases with L); a line with cap 0 has none"""
    f = _native.lib.ta_forced_workspace_bytes
    size = np.asarray([f(int(t), int(c)) if c > 0 else 0 for t, c in zip(T, caps)], dtype=np.int64)
    if (size < 0).any():
        q = int(np.flatnonzero(size < 0)[0])
        raise ValueError("line %d: %d timesteps are outside what ta_forced_align_lines takes" % (q, int(T[q])))
    off = np.zeros(len(size), dtype=np.int64)
    if len(size):
        off[1:] = np.cumsum(size)[:-1]
    return off, int(size.sum())


class Refining(object):
    """A chunk's refinement on its way (alignToOCR.PageChunk.align with refine): ta_harvest_lines, ta_harvest_pack,
    ta_forced_align_lines (one launch per variant) and ta_refine_columns enqueued behind the aligner's launch on the
    stream it went to, and ONE pinned download started behind them.  complete() waits for that download alone.  The
    workspace and every other device buffer of the refinement are given back when the download has been started (the
    stream's own order keeps them until the kernels are through), the probabilities with the chunk.
    keep: the device buffers stay (self.d) and forced() / columns() can be launched again -- tools/refine_time.py."""
    last_bytes = None                # (workspace, probabilities) of the most recent chunk: tools/refine_time.py

    def __init__(self, chunk, batch, ratio, keep=False):
        from . import harvest, page_batch as pb
        rec, st = chunk.rec, chunk.st
        dev = batch.device
        o_line, line_first, T = chunk.line_table()
        nprob, nlines = int(batch.nprob), len(T)
        self.nprob, self.nlines, self.ops_off = nprob, nlines, batch.ops_off_host
        probs = st["probs"]
        cat = lambda arrs, dt: np.concatenate(arrs).astype(dt) if arrs else np.zeros(0, dt)        # noqa: E731
        classes = cat([harvest.transcript_classes(rec.model.codec, tr) for tr in chunk.transcripts], np.int32)
        o_cat, idx_cat = cat(o_line, np.int32), cat([np.asarray(i) for i in chunk.idxs], np.int32)
        self.T = np.ascontiguousarray(T, dtype=np.int32)
        self.caps = line_caps(self.T, line_first, chunk.transcripts)
        ws_off, ws_bytes = workspace_pieces(self.T, self.caps)
        plain = np.asarray([pb.plain_page(tr, sy) for tr, sy in zip(chunk.transcripts, chunk.syls_all)], dtype=np.uint8)
        self.box_base = int(np.asarray(chunk.boxes).reshape(-1, 4).shape[0])
        Refining.last_bytes = (ws_bytes, int(probs.numel()) * 4)
        self.stream = torch.cuda.current_stream(dev)
        probs.record_stream(self.stream)                 # written on the recogniser's stream, read here
        pad1 = lambda a: a if a.size else np.zeros(1, a.dtype)                                      # noqa: E731
        d = dict(zip(("o_line", "idx", "row", "T", "ws_off", "cap", "plain", "line_first"), _native.upload_packed(
            [pad1(o_cat), pad1(idx_cat), np.ascontiguousarray(st["row_start_host"][:nlines], dtype=np.int64), self.T, ws_off,
             self.caps, plain, np.ascontiguousarray(line_first, dtype=np.int64)], dev)))
        tb = harvest.harvest_alignment(batch, d["o_line"] if len(o_cat) else o_cat, line_first, classes, d["T"], ratio)
        i32 = dict(dtype=torch.int32, device=dev)
        nbytes = int(batch.ops.numel())
        d.update(probs=probs, batch=batch, tb=tb, t_len=len(classes), o_len=len(o_cat), ws_bytes=ws_bytes,
                 frames=torch.empty((int(tb.labels.numel()), FIELDS), **i32),
                 score=torch.empty(nlines, dtype=torch.int64, device=dev), f_status=torch.empty(nlines, **i32),
                 work=torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev),
                 ops_new=torch.empty(nbytes, dtype=torch.uint8, device=dev), idx_new=torch.empty(nbytes, **i32),
                 ops_new_len=torch.empty(nprob, **i32), idx_new_len=torch.empty(nprob, **i32), r_status=torch.empty(nprob, **i32),
                 refined=torch.empty(nlines, **i32), slot=torch.empty(nlines, **i32))
        self.d = d
        self.forced()
        self.columns()
        self.download = _native.download_begin([d["ops_new"], d["ops_new_len"], d["idx_new"], d["idx_new_len"], d["refined"],
                                                d["frames"], tb.acc_line, tb.L, tb.lab_off, tb.count, tb.status[:nprob],
                                                d["f_status"], d["r_status"]])
        if not keep:
            self.d = None
        self.refined = None

    def forced(self):
        """ta_forced_align_lines on the harvest's packed slots, where they lie"""
        d, tb, p = self.d, self.d["tb"], lambda t: t.data_ptr()                                     # noqa: E731
        probs = d["probs"]
        _native.check(_native.lib.ta_forced_align_lines(
            p(probs), p(d["row"]), p(d["T"]), p(d["ws_off"]), p(d["cap"]), p(tb.acc_line), p(tb.L), p(tb.lab_off), p(tb.labels),
            p(tb.count), self.nlines, self.nlines, int(probs.shape[1]), int(probs.shape[0]), int(tb.labels.numel()),
            self.T.ctypes.data, self.caps.ctypes.data, p(d["work"]), d["ws_bytes"], p(d["frames"]), p(d["score"]),
            p(d["f_status"]), self.stream.cuda_stream), "ta_forced_align_lines")

    def columns(self):
        """ta_refine_columns on the aligner's columns, the harvest's tables and the forced alignment's status"""
        d, tb, p = self.d, self.d["tb"], lambda t: t.data_ptr()                                     # noqa: E731
        batch = d["batch"]
        _native.check(_native.lib.ta_refine_columns(
            p(batch.ops), p(batch.ops_off), p(batch.ops_len), int(batch.ops.numel()), p(batch.t_off), p(batch.o_off), d["t_len"],
            d["o_len"], self.nprob, p(d["o_line"]), p(d["line_first"]), p(d["idx"]), p(tb.table), p(tb.status), self.nlines,
            p(tb.acc_line), p(tb.L), p(tb.lab_off), p(tb.count), self.nlines, int(tb.labels.numel()), p(d["f_status"]),
            p(d["plain"]), self.box_base, p(d["ops_new"]), p(d["ops_new_len"]), p(d["idx_new"]), p(d["idx_new_len"]),
            p(d["refined"]), p(d["slot"]), p(d["r_status"]), self.stream.cuda_stream), "ta_refine_columns")

    def complete(self, chunk, waiter=None):
        """wait for the download, refuse what the kernels refused (RuntimeError, the page named), build the new box rows on
        the host (peak_boxes: the one-decimal rule stays there) and hand columns, rows and boxes to replace_columns()"""
        from . import harvest, ocr
        (ops_new, ops_len, idx_new, idx_len, refined, frames, acc, L, lab_off, count, h_status, f_status,
         r_status), self.download = self.download.wait(waiter), None
        self.d = None
        page = lambda p: chunk.page_ids[p] if chunk.page_ids is not None else p                      # noqa: E731
        bad = np.flatnonzero(h_status)
        if bad.size:
            raise RuntimeError("ta_harvest_lines refused page %d on the device: %s"
                               % (page(int(bad[0])), harvest.STATUS.get(int(h_status[bad[0]]), "?")))
        if (count < 0).any():
            raise RuntimeError("ta_harvest_pack found a row of the table out of bounds on the device")
        bad = np.flatnonzero(r_status)
        if bad.size:
            raise RuntimeError("ta_refine_columns refused page %d on the device: %s"
                               % (page(int(bad[0])), REFINE_STATUS.get(int(r_status[bad[0]]), "?")))
        k, nl = int(count[0]), int(count[1])
        acc, L, lab_off = acc[:k].astype(np.int64), L[:k].astype(np.int64), lab_off[:k]
        old = np.asarray(chunk.boxes, dtype=np.int64).reshape(-1, 4)
        if k:
            # a row per label of every packed slot, at box_base + lab_off[k]; the rows of a slot that was not aligned hold
            # whatever its frames held and are never referenced
            done = np.repeat((f_status[:k] == OK) & (L <= MAX_TARGET), L)
            t_peak = np.where(done, frames[:nl, 2], 0)
            x_min, y_min, y_max = chunk.strip_geometry(acc)
            new = peak_boxes(t_peak, L, self.T[acc].astype(np.int64), np.asarray(chunk.widths, dtype=np.int64)[acc],
                             x_min, y_min, y_max, ocr.PAD)
            boxes = np.concatenate([old, new])
        else:
            boxes = old
        ops_r, idx_r = [], []
        for p in range(self.nprob):
            a = int(self.ops_off[p])
            ops_r.append(ops_new[a:a + int(ops_len[p])].copy())
            idx_r.append(idx_new[a:a + int(idx_len[p])].astype(np.int64))
        self.refined = refined.astype(bool)
        chunk.replace_columns(ops_r, idx_r, boxes)


class RefineResult(object):
    """refine_pages' result: results (per page (syl_boxes, image, lines_peak_locs, all_chars), as process_batch returns
    them), indices / arrays (as its indices_out / arrays_out), refined (bool per text line, page after page), frames
    (per line an (L, 3) array of t_first, t_last, t_peak, None for a line that was not aligned), score (per line, None
    likewise), harvest (the HarvestResult), spans (locate: (a, b) per page, else None), object_pages (pages whose
    syllable search took the object path: returned unrefined)."""

    def __init__(self, results, indices, arrays, refined, frames, score, harvest, object_pages):
        self.results, self.indices, self.arrays, self.refined = results, indices, arrays, refined
        self.frames, self.score, self.harvest, self.spans = frames, score, harvest, harvest.spans
        self.object_pages = object_pages

    def __len__(self):
        return len(self.results)


def refine_pages(pages, transcripts, ocropus_model, seq_align_params=None, min_agreement=0.9, locate=False):
    """process_batch (one chunk) with the boxes of every ACCEPTED line refined by forced alignment: a RefineResult.

    The flow is harvest.harvest_pages' -- recognise, align, harvest -- with the recogniser's probabilities kept; one
    ta_forced_align then covers the accepted lines, and a line is refined if the harvest rule accepted it (reason 0:
    min_agreement and the other bits, harvest.py) and the kernel aligned it.  Every kept transcript character of a
    refined line gets the box the page path's construction yields for its peak; everything else keeps what it has.
    A page none of whose lines is refined comes out exactly as from process_batch.  ValueErrors as harvest_pages."""
    from . import harvest, ocr, page_batch as pb
    hres, chunk = harvest._harvest_flow(pages, transcripts, ocropus_model, seq_align_params, min_agreement, locate,
                                        want_probs=True)
    rec, st = chunk.rec, chunk.st
    nlines = len(hres)
    packed = hres.packed
    take = np.flatnonzero(packed["L"] <= MAX_TARGET)
    acc = packed["acc_line"][take].astype(np.int64)
    L, lab_off = packed["L"][take].astype(np.int64), packed["lab_off"][take]
    refined = np.zeros(nlines, dtype=bool)
    frames, score = [None] * nlines, [None] * nlines
    T_all = np.asarray(st["T_host"], dtype=np.int64)[:nlines]
    if len(acc):
        with torch.cuda.device(rec.device):
            got = forced_alignment(st["probs"], np.asarray(st["row_start_host"])[acc], T_all[acc], packed["labels"], lab_off, L,
                                   host=True)
        for k, q in enumerate(acc):
            if got["status"][k] == OK:
                refined[q] = True
                frames[q] = got["frames"][lab_off[k]:lab_off[k] + L[k]]
                score[q] = int(got["score"][k])
    transcripts_, syls_all = chunk.transcripts, chunk.syls_all
    object_pages = [p for p in range(len(transcripts_)) if not pb.plain_page(transcripts_[p], syls_all[p])]
    for p in object_pages:
        refined[int(hres.line_first[p]):int(hres.line_first[p + 1])] = False
    # ---- the refined lines' boxes, then every page's columns with their runs replaced ------------------------------------
    qs = np.flatnonzero(refined)
    x_min, y_min, y_max = chunk.strip_geometry(qs)
    Lq = np.array([len(frames[q]) for q in qs], dtype=np.int64)
    old = np.asarray(chunk.boxes, dtype=np.int64).reshape(-1, 4)
    if len(qs):
        new = peak_boxes(np.concatenate([frames[q][:, 2] for q in qs]), Lq, T_all[qs],
                         np.asarray(chunk.widths, dtype=np.int64)[qs], x_min, y_min, y_max, ocr.PAD)
    else:
        new = np.zeros((0, 4), np.int64)
    row_of = dict(zip(qs.tolist(), (len(old) + np.concatenate([[0], np.cumsum(Lq)[:-1]])).tolist() if len(qs) else []))
    ops_r, idx_r = [], []
    for p in range(len(transcripts_)):
        mine = [(q, int(hres.table[q][1]), int(hres.table[q][2]), int(row_of[q]))
                for q in range(int(hres.line_first[p]), int(hres.line_first[p + 1])) if refined[q]]
        o, i = refine_columns(hres.ops[p], chunk.idxs[p], hres.o_line[p], mine)
        ops_r.append(o)
        idx_r.append(i)
    chunk.replace_columns(ops_r, idx_r, np.concatenate([old, new]))
    indices, arrays = [], []
    results = chunk.finish(indices, arrays)
    out = RefineResult(results, indices, arrays, refined, frames, score, hres, object_pages)
    out.columns = (ops_r, idx_r, chunk.syl_boxes)       # what the boxes were formed from, for checking the rule
    out.probs, out.row_off, out.T = st["probs"], np.asarray(st["row_start_host"])[:nlines], T_all
    return out
