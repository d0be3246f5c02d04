"""Harvesting: line-level training texts from aligned pages, on the device where the alignment columns lie.

The page side of the package aligns a page's OCR with the page's transcript; the training side (train.LineTrainer)
wants one ground-truth text per TEXT LINE.  Every OCR character knows its line and the alignment is monotone, so each
line owns one contiguous piece of the transcript: `harvest_alignment` cuts it out per line, with counts that say how far
to trust it and an accept / reject decision, and packs the accepted lines in the layout the CTC kernel reads
(csrc/ta_harvest.hip: `ta_harvest_lines`, `ta_harvest_pack`).  `harvest_pages` drives recognise -> align -> harvest for a
batch of pages; `LineTrainer.train_from_pages` trains on what it accepts.  The rule is DESIGN.md section 14.6; the
checker of record is tests/harvest_ref.py.  How many lines of real manuscript pages the rule accepts has NOT been
measured.
"""
import fractions

import numpy as np
import torch

from . import _native

FIELDS = _native.TA_HARVEST_FIELDS              # reason, t_first, L, equal, unequal, interior op-1, op-2, seam
EMPTY, LOW, SEAM, UNANCHORED = (_native.TA_HARVEST_EMPTY, _native.TA_HARVEST_LOW, _native.TA_HARVEST_SEAM,
                                _native.TA_HARVEST_UNANCHORED)
CODEC, TOO_LONG, PAGE = _native.TA_HARVEST_CODEC, _native.TA_HARVEST_TOO_LONG, _native.TA_HARVEST_PAGE
REASONS = (("EMPTY", EMPTY), ("LOW", LOW), ("SEAM", SEAM), ("UNANCHORED", UNANCHORED), ("CODEC", CODEC),
           ("TOO_LONG", TOO_LONG), ("PAGE", PAGE))
STATUS = {_native.TA_HARVEST_OK: "ok", _native.TA_HARVEST_UNFINISHED: "unfinished traceback",
          _native.TA_HARVEST_MISMATCH: "columns disagree with the page's sizes",
          _native.TA_HARVEST_LINES: "line indices decrease or leave the page"}
MAX_DEN = _native.TA_HARVEST_MAX_DEN
COUNT_NAMES = ("equal", "unequal", "interior", "op2", "seam")


def agreement_ratio(min_agreement):
    """the minimum agreement as a ratio (num, den) of two positive integers: a number goes through
    fractions.Fraction(str(x)) (0.9 is 9/10, not the binary fraction next to it), a (num, den) pair is taken as it is.
    ValueError for a value outside (0, 1] or a denominator over 10^6."""
    if isinstance(min_agreement, (tuple, list)):
        if len(min_agreement) != 2 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool)
                                               for v in min_agreement):
            raise ValueError("min_agreement as a pair is (num, den), two integers")
        num, den = int(min_agreement[0]), int(min_agreement[1])
    else:
        try:
            fr = fractions.Fraction(str(min_agreement))
        except (ValueError, ZeroDivisionError):
            raise ValueError("min_agreement %r is no number" % (min_agreement,))
        num, den = fr.numerator, fr.denominator
    if den <= 0 or num <= 0 or num > den:
        raise ValueError("min_agreement must lie in (0, 1], got %s/%s" % (num, den))
    if den > MAX_DEN:
        raise ValueError("min_agreement needs a denominator of at most %d, got %d" % (MAX_DEN, den))
    return num, den


def reason_names(reason):
    """the names of the bits set in a line's reason ([] = accepted)"""
    return [name for name, bit in REASONS if reason & bit]


def transcript_classes(codec, text):
    """the recogniser's class of every character of a transcript, as train.encode_text numbers them; 0 for a character
    that is not in the codec.  The rule trims spaces by their class 1, so a codec whose space is another class is a
    ValueError."""
    index = {ch: k for k, ch in enumerate(codec) if k > 0 and ch != ""}
    if index.get(" ") != 1:
        raise ValueError("harvesting needs a codec whose class 1 is the space")
    return np.fromiter((index.get(ch, 0) for ch in text), dtype=np.int32, count=len(text))


class HarvestTables(object):
    """What the two kernels wrote, on the device: table (lines, 8) int32, status (pages,) int32, and the packed accepted
    lines acc_line / L (int32), lab_off (int64), labels (int32; the first count[1] are written), count (2,) int64 =
    accepted lines, labels.  host() downloads everything once: a dict of numpy arrays with the packed ones cut to their
    counts."""

    def __init__(self, nprob, nlines, table, status, acc_line, L, lab_off, labels, count):
        self.nprob, self.nlines = nprob, nlines
        self.table, self.status = table, status
        self.acc_line, self.L, self.lab_off, self.labels, self.count = acc_line, L, lab_off, labels, count
        self._host = None

    def host(self):
        if self._host is None:
            count = self.count.cpu().numpy()
            if (count < 0).any():
                raise RuntimeError("ta_harvest_pack found a row of the table out of bounds on the device")
            k, nl = int(count[0]), int(count[1])
            self._host = {"table": self.table[:self.nlines].cpu().numpy(), "status": self.status[:self.nprob].cpu().numpy(),
                          "acc_line": self.acc_line[:k].cpu().numpy(), "L": self.L[:k].cpu().numpy(),
                          "lab_off": self.lab_off[:k].cpu().numpy(), "labels": self.labels[:nl].cpu().numpy(),
                          "count": count}
        return self._host


def _int32_input(x, name, need, uploads):
    """a device int32 tensor as it is (at least `need` elements), anything else as a host array queued for the upload"""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        if x.dtype != torch.int32 or not x.is_contiguous() or x.numel() < need:
            raise ValueError("%s must be a contiguous int32 tensor of at least %d elements" % (name, need))
        return x
    arr = np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.int32).reshape(-1)
    if arr.size != need:
        raise ValueError("%s has %d entries, the batch needs %d" % (name, arr.size, need))
    uploads.append((name, arr if arr.size else np.zeros(1, np.int32)))
    return None


def harvest_alignment(batch, o_line, line_first, t_class, T, min_agreement=0.9, host=False, _fill=None):
    """The device-level call, on a textSeqCompare.NWBatch whose run() has been enqueued (one page per problem).

    o_line: per character of the batch's OCR strings (as the batch holds them: abbreviations expanded, an inserted
    character carrying its donor's line) the batch-wide index of its text line; line_first: pages + 1 host integers,
    page p owns the lines line_first[p] .. line_first[p + 1]; t_class: per transcript character its class
    (transcript_classes); T: per line its timesteps.  o_line, t_class and T are host arrays or int32 device tensors.
    Two launches on torch's current stream, which must be the stream the batch ran on or one that waits for it;
    nothing is waited for.  Returns a HarvestTables (host=True: its host() dict instead).
    ValueError for sizes that do not fit the batch and for a min_agreement agreement_ratio refuses.  (_fill: a byte
    value every output and the workspace are filled with before the launches -- for tests.)"""
    num, den = agreement_ratio(min_agreement)
    nprob = int(batch.nprob)
    lf = np.ascontiguousarray(line_first, dtype=np.int64).reshape(-1)
    if lf.size != nprob + 1:
        raise ValueError("line_first needs one entry per page and one more")
    nlines = int(lf[-1])
    if lf[0] != 0 or (np.diff(lf) < 0).any():
        raise ValueError("line_first must run from 0 upwards without decreasing")
    t_off = np.zeros(nprob + 1, dtype=np.int64)
    o_off = np.zeros(nprob + 1, dtype=np.int64)
    np.cumsum(batch.n, out=t_off[1:])
    np.cumsum(batch.m, out=o_off[1:])
    t_len, o_len = int(t_off[-1]), int(o_off[-1])
    dev = batch.device
    lib = _native.lib
    ws_bytes = int(lib.ta_harvest_workspace_bytes(nlines, t_len, o_len))
    if ws_bytes < 0:
        raise ValueError("the batch is larger than the harvest kernels take")
    uploads = [("line_first", lf)]
    given = {"o_line": _int32_input(o_line, "o_line", o_len, uploads),
             "t_class": _int32_input(t_class, "t_class", t_len, uploads),
             "T": _int32_input(T, "T", nlines, uploads)}
    with torch.cuda.device(dev):
        for (name, _), t in zip(uploads, _native.upload_packed([a for _, a in uploads], dev)):
            given[name] = t
        i32 = dict(dtype=torch.int32, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = HarvestTables(nprob, nlines, torch.empty((max(nlines, 1), FIELDS), **i32), torch.empty(max(nprob, 1), **i32),
                            torch.empty(max(nlines, 1), **i32), torch.empty(max(nlines, 1), **i32),
                            torch.empty(max(nlines, 1), dtype=torch.int64, device=dev), torch.empty(max(t_len, 1), **i32),
                            torch.empty(2, dtype=torch.int64, device=dev))
        if _fill is not None:
            ws.fill_(_fill)
            for t in (out.table, out.status, out.acc_line, out.L, out.lab_off, out.labels, out.count):
                t.view(torch.uint8).fill_(_fill)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _native.check(lib.ta_harvest_lines(
            batch.ops.data_ptr(), batch.ops_off.data_ptr(), batch.ops_len.data_ptr(), batch.ops.numel(),
            batch.t_codes.data_ptr(), batch.t_off.data_ptr(), batch.o_codes.data_ptr(), batch.o_off.data_ptr(), nprob,
            given["o_line"].data_ptr(), given["line_first"].data_ptr(), given["t_class"].data_ptr(), given["T"].data_ptr(),
            nlines, num, den, t_off.ctypes.data, o_off.ctypes.data, lf.ctypes.data, ws.data_ptr(), ws_bytes,
            out.table.data_ptr(), out.status.data_ptr(), stream), "ta_harvest_lines")
        _native.check(lib.ta_harvest_pack(
            out.table.data_ptr(), ws.data_ptr(), ws_bytes, given["t_class"].data_ptr(), t_len, nlines, max(t_len, 1),
            out.acc_line.data_ptr(), out.L.data_ptr(), out.lab_off.data_ptr(), out.labels.data_ptr(),
            out.count.data_ptr(), stream), "ta_harvest_pack")
        return out.host() if host else out


class HarvestLine(object):
    """one text line of a harvested batch: page, line (in the page), strip (what the recogniser was given for it: the
    prepared (T, 48) rows or the raw uint8 strip, i.e. what LineTrainer.train takes), source (the page.Strip it was cut
    as: position on the page, `.pixels`), text (the kept piece of the page's transcript; None for a line with none),
    reason (0 = accepted) and counts {equal, unequal, interior, op2, seam}"""
    __slots__ = ("page", "line", "strip", "source", "text", "reason", "counts")

    def __init__(self, page, line, strip, source, text, reason, counts):
        self.page, self.line, self.strip, self.source = page, line, strip, source
        self.text, self.reason, self.counts = text, reason, counts

    def reasons(self):
        return reason_names(self.reason)


class HarvestResult(object):
    """harvest_pages' result: lines (a HarvestLine per text line, page after page), table (lines, 8) and status
    (pages,) as the kernel wrote them, packed (the accepted lines as the CTC kernel reads them: acc_line, L, lab_off,
    labels), and what the rule was applied to, for checking it: ops (per page the alignment columns), o_line (per page
    the line of every expanded OCR character), ocr (per page the expanded OCR string), line_first, T.  trained: what
    LineTrainer.train returned for the accepted lines (train_from_pages only)."""

    def __init__(self, lines, host, ops, o_line, ocr, line_first, T, ratio):
        self.lines, self.table, self.status = lines, host["table"], host["status"]
        self.packed = {k: host[k] for k in ("acc_line", "L", "lab_off", "labels")}
        self.ops, self.o_line, self.ocr, self.line_first, self.T, self.min_agreement = ops, o_line, ocr, line_first, T, ratio
        self.trained = None

    def accepted(self):
        """(strip, text) of every accepted line, in line order"""
        for ln in self.lines:
            if ln.reason == 0:
                yield ln.strip, ln.text

    def __len__(self):
        return len(self.lines)


def harvest_pages(pages, transcripts, ocropus_model, seq_align_params=None, min_agreement=0.9, locate=False):
    """Recognise the pages' lines, align every page's OCR with its transcript and harvest: a HarvestResult.

    pages, transcripts, ocropus_model (ONE model: a path, a LineModel or a LineRecognizer) and seq_align_params as
    alignToOCR.process_batch takes them; the first stages of process_batch run through their own helpers, as one chunk.
    min_agreement: agreement_ratio.  ValueError for a scoring system the integer aligner refuses (a scoring callable,
    non-integral numbers, a codec with multi-character entries, a page too large), as evaluate_text_alignment.sweep
    refuses them -- the harvest reads the integer aligner's columns on the device.
    locate: as in alignToOCR.process_batch -- the transcripts may be longer than the pages; each page's span (a, b) is
    found first (`spans` of the result, one per page) and the harvested texts are slices of transcript[a:b]."""
    return _harvest_flow(pages, transcripts, ocropus_model, seq_align_params, min_agreement, locate)[0]


def _harvest_flow(pages, transcripts, ocropus_model, seq_align_params, min_agreement, locate, want_probs=False):
    """harvest_pages' body: (the HarvestResult, the alignToOCR.PageChunk after its align(), its columns taken).
    want_probs: the recogniser also keeps its probabilities (forced.refine_pages goes on from here)."""
    from . import alignToOCR as atocr
    ratio = agreement_ratio(min_agreement)
    pages, transcripts = list(pages), list(transcripts)
    if len(pages) != len(transcripts):
        raise ValueError("%d pages but %d transcripts" % (len(pages), len(transcripts)))
    if isinstance(ocropus_model, (list, tuple)):
        raise ValueError("harvest_pages takes one model for all pages")
    rec = atocr._recognizer_for(ocropus_model)
    chunk = atocr.PageChunk(rec, pages, transcripts, seq_align_params, atocr.parallel, locate)
    chunk.launch(want_probs=bool(want_probs))
    chunk.host_ahead()
    chunk.align()
    transcripts = chunk.transcripts                  # locate: the pages' own spans of what was passed
    classes = [transcript_classes(rec.model.codec, tr) for tr in transcripts]
    batch = chunk.nw
    if batch is None:
        raise ValueError("harvesting needs the integer aligner: no scoring callable, integral scoring numbers, a codec "
                         "of single characters and pages within its size limits")
    o_line, line_first, T = chunk.line_table()
    cat = lambda arrs: np.concatenate(arrs) if arrs else np.zeros(0, np.int32)                 # noqa: E731
    with torch.cuda.stream(atocr._nw_stream(rec.device)):                # the stream the aligner's launch went to
        host = harvest_alignment(batch, cat(o_line), line_first, cat(classes), T, ratio, host=True)
    ops = chunk.columns()
    bad = np.nonzero(host["status"])[0]
    if bad.size:
        raise RuntimeError("ta_harvest_lines refused page %d on the device: %s"
                           % (int(bad[0]), STATUS.get(int(host["status"][bad[0]]), "?")))
    lines, table = [], host["table"]
    for p in range(len(pages)):
        for q in range(int(line_first[p]), int(line_first[p + 1])):
            r = table[q]
            text = transcripts[p][int(r[1]):int(r[1]) + int(r[2])] if r[2] > 0 else None
            lines.append(HarvestLine(p, q - int(line_first[p]), chunk.lines[q], chunk.all_strips[q], text, int(r[0]),
                                     dict(zip(COUNT_NAMES, (int(v) for v in r[3:])))))
    result = HarvestResult(lines, host, ops, o_line, chunk.texts, line_first, T, ratio)
    result.spans = chunk.spans                       # locate: (a, b) per page into the transcript as passed; else None
    return result, chunk
