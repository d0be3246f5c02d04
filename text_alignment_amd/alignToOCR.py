# -*- coding: utf-8 -*-
"""Page driver -- drop-in for the reference module of the same name (reference
alignToOCR.py:24-351): same `process` / `perform_ocr_with_ocropus` / `to_JSON_dict` /
`CharBox` / `rotate_bbox` / `read_file` surface, same `syl_boxes` JSON.

What changed underneath (and nothing else): the OCR seam no longer writes PNG strips and shells
out to `ocropus-rpred` (alignToOCR.py:131-147) -- text-line strips go through the HIP line
recogniser in-process (text_alignment_amd.ocr) -- and the transcript/OCR alignment runs in the
HIP Needleman-Wunsch kernels (text_alignment_amd.textSeqCompare).  The glue between the two
kernels (abbreviation expansion, gap insertion, syllable grouping, rotation, JSON) is host-side
string/box work restated from the reference.

Gamera (the reference's image toolkit, alignToOCR.py:3-5) is not needed: a page arrives either
as a `text_alignment_amd.page.PreparedPage` carrying its text-line strips, or as a raw text-layer
image (numpy array), which `preproc` (text_alignment_amd.textAlignPreprocessing over the HIP kernels
of csrc/ta_preproc.hip) binarises, deskews and cuts into lines -- the two calls `process` makes at alignToOCR.py:216-218.
"""
import io
import json  # noqa: F401  (callers json.dump the result of to_JSON_dict, alignToOCR.py:434)
import os
import pickle
import re
import time

import numpy as np
import torch

from . import _native
from . import latinSyllabification as latsyl
from . import ocr
from . import textSeqCompare as tsc
from . import page as page_mod
from . import page_batch as pb
from . import textAlignPreprocessing as preproc

parallel = 2                # kept for signature compatibility (alignToOCR.py:24): one GPU batch
median_line_mult = 2        # alignToOCR.py:25


class CharBox(object):
    __slots__ = ['char', 'ul', 'lr', 'ulx', 'lrx', 'uly', 'lry', 'width', 'height']

    def __init__(self, char, ul=None, lr=None):
        self.char = char
        if (ul is None) or (lr is None):        # a gap marker: no geometry (alignToOCR.py:41-44)
            self.ul = None
            self.lr = None
            return
        self.ul, self.lr = tuple(ul), tuple(lr)
        self.ulx, self.uly = ul[0], ul[1]
        self.lrx, self.lry = lr[0], lr[1]
        self.width = lr[0] - ul[0]
        self.height = lr[1] - ul[1]

    def __repr__(self):
        if self.ul and self.lr:
            return '{}: {}, {}'.format(self.char, self.ul, self.lr)
        return '{}: empty'.format(self.char)

    # __slots__ classes pickle by slot; unset geometry of gap markers is skipped
    def __getstate__(self):
        return {k: getattr(self, k) for k in self.__slots__ if hasattr(self, k)}

    def __setstate__(self, state):
        # a pickle the reference wrote (alignToOCR.py:435-436: its CharBox has no __getstate__) carries the
        # default state of a __slots__ class, the pair (None, {slot: value})
        if isinstance(state, tuple) and len(state) == 2:
            state = dict(state[0] or {}, **(state[1] or {}))
        for k, v in state.items():
            if k not in self.__slots__:
                raise pickle.UnpicklingError("CharBox has no slot %r" % (k,))
            setattr(self, k, v)


class _BoxUnpickler(pickle.Unpickler):
    """Loader of the OCR cache files of alignToOCR.py:225-233 (written at :435-436 and by
    evaluate_text_alignment.py:170-171 with protocol 2): a list of CharBox and nothing else.  The class may be
    named after the reference's module (`alignToOCR`, or `__main__` when the reference ran as a script) or
    after this one; coordinates may be numpy scalars (rotate_bbox's int16).  No other global resolves, so a
    cache file cannot run code -- the same rule as the model loader's (model_io.RestrictedUnpickler)."""
    _BOX_MODULES = ('alignToOCR', '__main__', 'text_alignment_amd.alignToOCR')

    def find_class(self, module, name):
        if name == 'CharBox' and module in self._BOX_MODULES:
            return CharBox
        if module in ('numpy.core.multiarray', 'numpy._core.multiarray') and name == 'scalar':
            import numpy.core.multiarray as ma
            return ma.scalar
        if module == 'numpy' and name == 'dtype':
            return np.dtype
        if (module, name) in (('copy_reg', '_reconstructor'), ('copyreg', '_reconstructor')):
            import copyreg
            return copyreg._reconstructor
        if (module, name) in (('__builtin__', 'object'), ('builtins', 'object')):
            return object
        if (module, name) == ('_codecs', 'encode'):       # how Python 3 writes bytes at protocol 2
            import _codecs
            return _codecs.encode
        raise pickle.UnpicklingError('global %s.%s is not allowed in an OCR cache file' % (module, name))


def load_ocr_pickle(path):
    """list[CharBox] from a cache file this package or the reference (Python 2, latin-1 strings) wrote"""
    with open(path, 'rb') as f:
        chars = _BoxUnpickler(f, encoding='latin1').load()
    if not isinstance(chars, list) or not all(isinstance(c, CharBox) for c in chars):
        raise pickle.UnpicklingError('an OCR cache file holds a list of CharBox')
    return chars


def clean_special_chars(inp):
    '''drops the reject class '~' from OCR output (alignToOCR.py:61-72)'''
    return inp.replace('~', '')


def read_file(fname):
    '''plaintext transcript of a page -> one string (alignToOCR.py:75-87)'''
    with open(fname, 'r') as f:
        rows = f.readlines()
    text = ' '.join(r for r in rows if not r[0] == '#')
    for junk in ('\n', '\r', '| '):
        text = text.replace(junk, '')
    return text


def rotate_bbox(cbox, angle, orig_dim, target_dim, radians=False):
    '''rotate a box about the centre of `orig_dim` and shift by half the size difference to
    `target_dim` (alignToOCR.py:90-125).  The reference runs on Python 2, where the three
    divisions at alignToOCR.py:91,95-96 are integer floor divisions.'''
    px, py = orig_dim.ncols // 2, orig_dim.nrows // 2
    dx = (orig_dim.ncols - target_dim.ncols) // 2
    dy = (orig_dim.nrows - target_dim.nrows) // 2
    if not radians:
        angle = angle * np.pi / 180
    s, c = np.sin(angle), np.cos(angle)

    def turn(x, y):
        x, y = x - px, y - py
        return (x * c) - (y * s) + (px - dx), (x * s) + (y * c) + (py - dy)

    ulx, uly = turn(cbox.ulx, cbox.uly)
    lrx, lry = turn(cbox.lrx, cbox.lry)
    new_ul = np.round([ulx, uly]).astype('int16')
    new_lr = np.round([lrx, lry]).astype('int16')
    return CharBox(cbox.char, new_ul, new_lr)


def rotate_bboxes(boxes, angle, orig_dim, target_dim, radians=False):
    """rotate_bbox over a whole page's boxes at once: the same float64 arithmetic element by
    element (one numpy pass instead of four np.round calls per box)."""
    if not boxes:
        return []
    px, py = orig_dim.ncols // 2, orig_dim.nrows // 2
    dx = (orig_dim.ncols - target_dim.ncols) // 2
    dy = (orig_dim.nrows - target_dim.nrows) // 2
    if not radians:
        angle = angle * np.pi / 180
    s, c = np.sin(angle), np.cos(angle)
    pts = np.array([[b.ulx, b.uly, b.lrx, b.lry] for b in boxes])
    x = pts[:, 0::2] - px
    y = pts[:, 1::2] - py
    nx = (x * c) - (y * s) + (px - dx)
    ny = (x * s) + (y * c) + (py - dy)
    rx = np.round(nx).astype('int16')
    ry = np.round(ny).astype('int16')
    return [CharBox(b.char, np.array([rx[k, 0], ry[k, 0]]), np.array([rx[k, 1], ry[k, 1]]))
            for k, b in enumerate(boxes)]


# --------------------------------------------------------------------------- OCR seam
_recognizers = {}


def _recognizer_for(ocropus_model):
    """`ocropus_model` as the reference passes it is a model file path (alignToOCR.py:390-405);
    a LineModel or a ready LineRecognizer is accepted as well."""
    if isinstance(ocropus_model, ocr.LineRecognizer):
        return ocropus_model
    key = id(ocropus_model) if not isinstance(ocropus_model, str) else os.path.abspath(ocropus_model)
    if key not in _recognizers:
        if isinstance(ocropus_model, str):
            from . import model_io
            model = model_io.load_pyrnn(ocropus_model)
        else:
            model = ocropus_model
        _recognizers[key] = (ocropus_model, ocr.LineRecognizer(model))
    return _recognizers[key][1]


def parse_llocs_text(text):
    """The `.llocs` wire format ocropus-rpred writes and the reference reads back
    (alignToOCR.py:157-170): one "char<TAB>x" line per decoded character, x with one decimal ->
    [(char, x)] as chars_from_llocs takes it."""
    out = []
    for line in text.split('\n'):
        if line == '':
            continue
        lsp = line.split('\t')
        out.append((lsp[0], float(lsp[1])))
    return out


def chars_from_llocs(llocs, x_min, y_min, y_max, all_chars):
    """One strip's (char, x) list -> CharBoxes appended to all_chars (alignToOCR.py:160-182).
    ocropus reports the RIGHT edge of each character, so a character's box runs from the
    previous character's position to its own; '~' and '' still advance the position."""
    if not llocs:
        return
    prev_xpos = x_min
    for (ch, _), cur_xpos in zip(llocs, pb.edge_positions([x for _, x in llocs], x_min).tolist()):
        if not (ch == '~' or ch == ''):
            all_chars.append(CharBox(clean_special_chars(ch), (prev_xpos, y_min), (cur_xpos, y_max)))
        prev_xpos = cur_xpos


def perform_ocr_with_ocropus(cc_strips, ocropus_model, wkdir_name=None, parallel=parallel):
    """Recognise every text-line strip of a page and return its characters in reading order
    (strip order, then x), as reference alignToOCR.py:128-184 does through `ocropus-rpred`.

    cc_strips: objects with offset_x, offset_y, height and either `prepared` (a (T, 48) array,
    ink = 1, already normalised and padded) or `pixels` (raw 2-D uint8 strip, white background:
    normalised on the device, csrc/ta_lineest.hip).  wkdir_name and `parallel` (the reference's
    temp directory and number of ocropus worker processes) are accepted and unused: all strips of
    the page go to the GPU in one batch and no host-side image work is left to spread.
    """
    rec = _recognizer_for(ocropus_model)
    prepared = page_mod.prepared_lines(list(cc_strips), workers=parallel)
    lines = [xs for xs, _ in prepared]
    widths = [w for _, w in prepared]
    decoded = rec.recognise(lines)
    all_chars = []
    for k, (strip, raw_w, dec) in enumerate(zip(cc_strips, widths, decoded)):
        llocs = rec.llocs(dec, int(rec.last_T[k]), raw_w)
        chars_from_llocs(llocs, strip.offset_x, strip.offset_y, strip.offset_y + strip.height, all_chars)
    return all_chars


# --------------------------------------------------------------------------- alignment glue
def expand_abbreviations(all_chars):
    """Replace every occurrence of an abbreviation in the OCR character list by its expansion;
    character k of the abbreviation lends its box to all letters of segment k
    (alignToOCR.py:251-264).  String positions index the character list, as in the reference."""
    ocr_str = ''.join(str(x.char) for x in all_chars)
    for abb, segments in latsyl.abbreviations.items():
        idx = ocr_str.find(abb)
        while idx != -1:
            ins = []
            for k, segment in enumerate(segments):
                donor = all_chars[k + idx]
                ins += [CharBox(ch, donor.ul, donor.lr) for ch in segment]
            all_chars = all_chars[:idx] + ins + all_chars[idx + len(abb):]
            ocr_str = ''.join(str(x.char) for x in all_chars)        # only after a replacement
            idx = ocr_str.find(abb)
    return all_chars


def syllable_boxes(syls, tra_align, all_chars, indices=None):
    """For each syllable of the transcript, the union of the OCR character boxes it is aligned
    to (alignToOCR.py:297-324).  `indices`, if given, receives for every emitted box the index of
    its syllable among the non-empty syllables of the transcript."""
    out = []
    offset = 0
    which = -1
    for syl in syls:
        if len(syl) < 1:
            continue
        which += 1
        if len(syl) == 1:
            pattern = syl
        else:
            pattern = syl[0] + syl[1:-1].replace('', '_*') + syl[-1]
        hit = re.search(pattern, tra_align[offset:])
        start, end = hit.start() + offset, hit.end() + offset
        offset = end
        boxes = [b for b in all_chars[start:end] if b.lr is not None]
        if not boxes:
            continue                          # aligned to nothing in the OCR
        if len(set(b.uly for b in boxes)) > 1:
            lowest = max(b.uly for b in boxes)       # spans two text lines: keep the lower one
            boxes = [b for b in boxes if b.uly == lowest]
        ul = (min(b.ulx for b in boxes), min(b.uly for b in boxes))
        lr = (max(b.lrx for b in boxes), max(b.lry for b in boxes))
        out.append(CharBox(syl, ul, lr))
        if indices is not None:
            indices.append(which)
    return out


def snap_to_words(tr, i0, i1):
    """The span (i0, i1) the span search found in the transcript string `tr` (textSeqCompare.locate_span), widened
    OUTWARD to whole words: spaces at its ends go first; a span of nothing but spaces is empty (nothing of the
    transcript lies on the page); otherwise a word cut by the page's edge stays whole -- its off-page letters align to
    gaps, as they do without the search.  Returns (a, b), indices into `tr`."""
    while i0 < i1 and tr[i0] == ' ':
        i0 += 1
    while i1 > i0 and tr[i1 - 1] == ' ':
        i1 -= 1
    if i0 == i1:
        return i0, i0
    a = tr.rfind(' ', 0, i0) + 1
    b = tr.find(' ', i1)
    return a, (len(tr) if b < 0 else b)


def align_page(transcript, all_chars, angle, image_dim, raw_dim, seq_align_params=None,
               alignment=None, indices=None, expanded=False, locate=False, spans_out=None):
    """Everything `process` does after OCR (alignToOCR.py:247-328), on plain data.  `alignment`
    may carry a precomputed (tra_align, ocr_align) of the transcript against the expanded OCR
    string (the batched driver aligns all pages in one launch).  locate: `transcript` is longer than the page (the
    neighbouring chants, the whole book); the page's own span is found first (textSeqCompare.locate_span, snapped to
    words), appended to spans_out as (a, b), and everything below runs on transcript[a:b]."""
    all_chars = list(all_chars) if expanded else expand_abbreviations(list(all_chars))
    ocr = ''.join(x.char for x in all_chars)
    all_chars_copy = list(all_chars)
    if locate:
        if alignment is not None:
            raise ValueError("locate=True finds the span itself: no precomputed alignment")
        i0, i1, _ = tsc.locate_span(list(transcript), list(ocr), seq_align_params)
        a, b = snap_to_words(transcript, i0, i1)
        transcript = transcript[a:b]
        if spans_out is not None:
            spans_out.append((a, b))
        if a == b:                            # nothing of the transcript on this page: no boxes, no aligner call
            return [], all_chars_copy

    if alignment is None:
        alignment = tsc.perform_alignment(list(transcript), list(ocr),
                                          scoring_system=seq_align_params, verbose=False)
    tra_align, ocr_align = alignment
    tra_align = ''.join(tra_align)
    ocr_align = ''.join(ocr_align)
    syls = latsyl.syllabify_text(transcript)

    # gaps of the OCR side get placeholder boxes (alignToOCR.py:285-292; a literal '_' in the OCR
    # text counts as a gap there too and trips the same assertion)
    ngaps = ocr_align.count('_')
    assert len(all_chars) + ngaps == len(tra_align), 'all_chars not same length as alignment: ' \
        '{} vs {}'.format(len(all_chars) + ngaps, len(tra_align))
    boxes = iter(all_chars)
    all_chars = [CharBox('_') if ch == '_' else next(boxes) for ch in ocr_align]

    syl_boxes = syllable_boxes(syls, tra_align, all_chars, indices)
    syl_boxes = rotate_bboxes(syl_boxes, -1 * angle, image_dim, raw_dim)
    return syl_boxes, all_chars_copy


def find_lines_all(pages, workers=1):
    """preprocessing + text-line finding of every page: (image_bin, image_eroded, angle, strips,
    peak locations) per page.  Page images (greyscale, colour or onebit, any numeric type: reduced to
    uint8 greyscale by preproc.to_grey_u8) go through the device kernels (preproc_gpu,
    csrc/ta_preproc.hip), several pages per batch so that the pipeline's data-dependent host decisions
    share their waits for the device; PreparedPages pass through.  `workers` -- the reference's
    `parallel` -- is accepted and unused: there is no host-side image work left to spread."""
    return preproc.find_lines_many(list(pages))


def _raw_dim(pg):
    """`raw_image.dim` of the reference (alignToOCR.py:328) for whatever stands for the raw page
    here: an object with .dim (PreparedPage, a Gamera-like image), or a bare pixel array /
    an object with .pixels, whose size is its shape."""
    dim = getattr(pg, "dim", None)
    if dim is not None and hasattr(dim, "ncols"):
        return dim
    px = getattr(pg, "pixels", pg)
    if not hasattr(px, "shape") or type(px).__module__.split(".")[0] != "torch":   # (a tensor -- possibly on the device -- has its shape)
        px = np.asarray(px)
    if len(px.shape) < 2:
        raise TypeError("a page is a PreparedPage, an image object with .dim, or a 2-D / 3-D pixel array")
    return page_mod.Dim(int(px.shape[1]), int(px.shape[0]))


# process_batch runs batches larger than this as a pipeline over chunks of PIPELINE_CHUNK_PAGES pages (three stages per chunk,
# see the loop): while the recogniser kernels of chunk k run, the copy pool stages the rows of chunk k + 1 and this thread
# does the later stages of chunks k - 2 and k - 3 (characters and the aligner launch; syllable boxes).  One host thread
# besides the copy pool; results are those of the unchunked call.
# (Plain module attributes: this module reads no environment variables; tools/switches.py sets them for timing experiments.)
PIPELINE_CHUNK_PAGES = 16
PIPELINE_CHUNK_PAGES_RAW = 16        # raw strips: the device normaliser in front (32 while every chunk's first stage WAITED for
                                     # its measuring pass; round 6 enqueues it and waits a stage later: 16 is faster, 970 against 885)
PIPELINE_CHUNK_PAGES_IMAGES = 16     # page images: preprocessing in front, itself in batches of pages on page threads of its own (64 until
                                     # round 6: no faster -- 447-564 against 542-557 pages/s -- and its 1 920-line recogniser batch took a
                                     # 17.7 GB scratch buffer from the caching allocator and gave it back on every call).  Measured twice and
                                     # not kept: the line finding of the NEXT chunk started ahead on a thread of its own -- 551-575
                                     # pages/s against 625-636 without while the page threads launched from Python, 750-787 against
                                     # 802-807 with a stage per library call and four page threads (same box each; bound to the GPU's
                                     # NUMA node as bench.py binds a rank: 731-789 against 801-854, three runs each, alternating): the
                                     # stages of the chunks in flight are Python, and more threads of it contend for one interpreter lock
_side_streams = {}
WAIT_SECONDS = [0.0]                 # wall seconds the calling thread has spent WAITING for the device inside process_batch (a
                                     # running total: callers take differences): a pass's wall time minus this is its host work
TWO_STREAMS = True                   # consecutive chunks' recogniser kernels on two compute streams


def _ocr_streams(device):
    """two compute streams for the recogniser kernels of consecutive chunks: on ONE stream the projection of chunk k + 1
    cannot start before the last workgroup of chunk k's recurrence has finished, and a chunk's recurrence is one round of
    workgroups whose CUs free up one by one as the shorter lines end (mean / longest line = 0.71)"""
    key = ("ocr", device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _side_streams:
        _side_streams[key] = [torch.cuda.Stream(device=device), torch.cuda.Stream(device=device)]
    return _side_streams[key]


def _nw_stream(device):
    """the aligner's launches of a chunk go to a side stream: on the recogniser's stream they would queue behind the
    next chunk's recurrence and the host would wait for it"""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=device)
    return _side_streams[key]


# The call's FIRST chunk is half a chunk: nothing can be finished on the host before the first chunk's characters are back,
# so its latency stands in front of the whole pipeline (a 16-page chunk: ~12 ms until decoded, an 8-page one ~6).  Measured
# on 64 pages of page-locked rows: chunks 8, 16, 16, 16, 8 give 2 125-2 140 pages/s against 1 937 for 4 x 16 (device rows
# 2 223-2 239 against 2 095-2 111; pageable rows the same within their noise); a first chunk of 4 pages is too small to
# fill the chip (1 790), halving the last chunk as well gains nothing (profiles/r06_lead_chunk.txt).
LEAD_CHUNK_DIVISOR = 2


def plan_chunks(groups, C, lead=()):
    """[(recogniser, page indices)] in pipeline order: every group of pages (one recogniser each, in order of first
    appearance) cut into runs of C pages; a last run shorter than C / 2 joins the run before it (no sliver of a chunk
    whose kernels would not cover the next chunk's host stage).  lead: sizes of the call's FIRST chunks (taken from the
    first group while more than C pages of it remain)"""
    chunks = []
    lead = list(lead)
    for rec, ks in groups:
        a = 0
        while lead and len(ks) - a > C + lead[0]:
            chunks.append((rec, ks[a:a + lead[0]]))
            a += lead.pop(0)
        lead = []
        while True:
            b = len(ks) if len(ks) - (a + C) < C // 2 else min(a + C, len(ks))
            chunks.append((rec, ks[a:b]))
            a = b
            if a >= len(ks):
                break
    return chunks


def process_batch(pages, transcripts, ocropus_model, seq_align_params=None, indices_out=None,
                  parallel=parallel, arrays_out=None, locate=False, spans_out=None, refine=False, min_agreement=0.9,
                  refined_out=None, refine_scope="line", confidence=False, confidence_out=None, posterior=False,
                  posterior_out=None, page_margin=None, page_scope_out=None, line_omit=None, omitted_out=None,
                  page_scope_omit=None):
    """`process` for many pages at once: the strips of ALL pages go through the line recogniser
    in one batch (large batches: in chunks of PIPELINE_CHUNK_PAGES pages, host and device overlapped), the
    transcript/OCR alignments of a chunk's pages run in one NW launch, and the glue in
    between runs on arrays (text_alignment_amd.page_batch) -- the shape in which a GPU is worth
    using.  Per page the result equals process(page, transcript, model, seq_align_params).  `ocropus_model` is one model
    for all pages or a list with one per page.
    Returns a list of (syl_boxes, image, lines_peak_locs, all_chars); the two box lists are
    sequences that build their CharBox objects on access.  indices_out, if given, receives per page
    the index of each box's syllable among the transcript's non-empty syllables; arrays_out the
    boxes themselves as an int array [k, 4] (ulx, uly, lrx, lry).
    locate: a page's transcript may be longer than the page -- the neighbouring chants, or ONE string for the whole book
    passed for every page (it is uploaded once per chunk).  Once a chunk's OCR text exists, one span search
    (textSeqCompare.SpanBatch) finds each page's own span, which is snapped to words (snap_to_words) and handed to
    spans_out as (a, b) per page; everything after that runs on transcript[a:b] exactly as without the switch.  Costs
    one more host wait per chunk.  ValueError up front for what the integer span search does not take: a scoring
    callable, non-integral numbers, a codec with multi-character entries.
    refine: the lines whose piece of the transcript the harvest rule accepts at min_agreement (harvest.agreement_ratio)
    get a box per transcript character from forced alignment, as forced.refine_pages gives them -- here inside the
    pipeline: each chunk's harvest, forced alignment and column replacement are enqueued behind its aligner launch and
    come back in the one download its last stage waits for anyway.  Per page the result equals
    refine_pages on that page; refined_out receives per page a bool per text line.  ValueError up front for what
    refine_pages refuses (a scoring callable, non-integral numbers, a codec with multi-character entries, a
    min_agreement outside (0, 1]); a page whose alignment the integer kernels do not take is a ValueError for the call.
    With refine=False nothing of this runs.
    refine_scope="page" with page_margin=M (an integer >= 0, characters; DESIGN.md sections 14.8 and 14.14): ONE best path
    through all lines of a page gives EVERY transcript character of an eligible page a box, as
    forced.refine_pages(scope="page", margin=M) does -- here inside the pipeline: behind each chunk's aligner launch the
    harvest, ta_page_windows (windows and eligibility on the device) and ta_forced_align_pages_gated (one launch per
    variant) are enqueued, and ONE download brings back what the chunk's last stage needs; the host forms no window and
    looks at no harvest table.  Per page every output equals refine_pages(scope="page", margin=M) on that page alone;
    refined_out receives a bool per text line (all True on a refined page), page_scope_out per page, in page order, a
    forced.PageScope: reason (0 = refined, else a key of forced.PAGE_SCOPE), windows ((lo, hi), None unless the reason is
    0 or PAGE_NO_PATH), frames ((n, 4), None for a page that was not refined) and score.  page_margin has no default here
    -- forced.DEFAULT_MARGIN is an unmeasured guess -- and refine_scope="page" without it is the ValueError it was before
    the pipeline had page scope: call forced.refine_pages(..., scope="page").  page_margin with refine=False, with
    refine_scope="line", with confidence or posterior, or anything but an integer >= 0 is a ValueError, before any GPU
    work.  page_confidence and page_posterior are not part of the pipeline: forced.refine_pages has them.  With
    refine_scope="line" or refine=False nothing of this is allocated, uploaded, launched or downloaded.
    page_scope_omit (with refine_scope="page" and page_margin): None, or the price in bits (0 ..
    1024, forced.omit_units) at which the page's ONE path may leave a transcript character out -- forced.refine_pages'
    `page_omit`, here inside the pipeline: the chunk calls ta_page_windows_omit and ta_forced_align_pages_omit_gated in
    place of the strict pair, its workspace sized by ta_forced_page_omit_gated_workspace_bytes, and downloads the same
    arrays.  Per page every output equals forced.refine_pages([page], [transcript], ..., scope="page", margin=M,
    page_omit=BITS) on that page alone; PageScope.omitted is the number of characters a refined page's path left out; a
    page whose path holds no character is PAGE_ALL_OMITTED and stays unrefined; a page with more characters than frames is
    eligible.  (The keyword is not `page_omit`: process_batch(page_omit=...) stays the TypeError it was.)  ValueError,
    before any GPU work and before a recogniser is built: without refine, without refine_scope="page" or page_margin, with
    line_omit, confidence or posterior, a bool, a non-number or a value outside 0 .. 1024.  No value of the price has been
    validated on real pages.  With page_scope_omit=None nothing of this is allocated, uploaded, launched or downloaded.
    confidence (with refine; ValueError without): every aligned line's per-character confidence from max-marginals
     is computed inside the same refinement -- two more launches per chunk behind the aligner's,
    their results in the chunk's one download -- and confidence_out receives per page, in page order, a
    forced.PageConfidence: char_confidence, syllable_confidence (aligned with the page's syllable boxes), confidence and
    rival per text line, each equal to what forced.refine_pages(confidence=True) returns for that page alone.  With
    confidence=False nothing of this runs and confidence_out is left alone.
    posterior (with refine; ValueError without): every aligned line's sum-product posteriors and its text's likelihood
     are computed inside the same refinement -- ta_forced_posterior_lines behind the aligner's
    launches, ta_posterior_pages behind the columns', their results in the chunk's one download -- and posterior_out
    receives per page, in page order, a forced.PagePosterior: char_posterior, syllable_posterior (aligned with the page's
    syllable boxes), and per text line posterior, rival_posterior, posterior_rival and loglik_bits, each equal bit for bit
    to what forced.refine_pages(posterior=True) returns for that page alone.  confidence and posterior together give both
    outputs.  With posterior=False nothing of this runs and posterior_out is left alone.
    line_omit (with refine at line scope): None, or the price in bits (0 .. 1024, forced.omit_units)
    of a transcript character the forced alignment of a line may leave out -- forced.refine_pages' `omit`, here inside the
    pipeline: the chunk's slots go through ta_forced_align_omit_lines and ta_refine_columns_omit instead of the strict
    pair, one more array comes back in the chunk's one download, and the box rows are formed from the present characters
    alone.  Per page every output equals forced.refine_pages([page], [transcript], ..., omit=line_omit) on that page alone;
    a line whose path holds no character is not refined.  omitted_out receives per page, in page order, an int32 array
    with one entry per text line: the characters of the line's text the path left out, -1 for a line that was not aligned
    (RefineResult.omitted with None as -1).  (The keyword is not `omit`: process_batch(omit=...) stays the TypeError it
    was; `line_omit` stands beside page_margin as the scope-prefixed name.)  ValueError, before any GPU work and before a
    recogniser is built: line_omit with refine=False, with refine_scope="page" or page_margin, with confidence or posterior
    (strict lattice only), a bool, a non-number or a value outside 0 .. 1024.  No value of the price has been validated on
    real pages.  With line_omit=None nothing of this is allocated, uploaded, launched or downloaded, and omitted_out is
    left alone."""
    page_omit_q = None
    if page_scope_omit is not None:                      # first of all: no recogniser, no GPU
        from . import forced
        page_omit_q = forced.omit_units(page_scope_omit)     # ValueError for a bool, a non-number, a value outside 0 .. 1024
        if not refine:
            raise ValueError("page_scope_omit belongs to refine=True")
        if refine_scope != "page" or page_margin is None:
            raise ValueError("page_scope_omit is the price at page scope: it goes with refine_scope='page' and page_margin")
        if line_omit is not None:
            raise ValueError("page_scope_omit is the price at page scope: not with line_omit")
        if confidence or posterior:
            raise ValueError("confidence and posteriors are defined on the strict lattice only: not with page_scope_omit")
    line_omit_q = None
    if line_omit is not None:                            # first of all: no recogniser, no GPU
        from . import forced
        line_omit_q = forced.omit_units(line_omit)       # ValueError for a bool, a non-number, a value outside 0 .. 1024
        if not refine:
            raise ValueError("line_omit belongs to refine=True")
        if refine_scope != "line" or page_margin is not None:
            raise ValueError("line_omit is the price at line scope: not with refine_scope='page' or page_margin")
        if confidence or posterior:
            raise ValueError("confidence and posteriors are defined on the strict lattice only: not with line_omit")
    if confidence and not refine:
        raise ValueError("confidence belongs to refine=True")
    if posterior and not refine:
        raise ValueError("posterior belongs to refine=True")
    if refine_scope not in ("line", "page"):
        raise ValueError("refine_scope is 'line' or 'page'")
    if page_margin is not None:
        if isinstance(page_margin, (bool, np.bool_)) or not isinstance(page_margin, (int, np.integer)) or page_margin < 0:
            raise ValueError("page_margin is a number of characters: an integer, 0 or more")
        if not refine:
            raise ValueError("page_margin belongs to refine=True")
        if refine_scope != "page":
            raise ValueError("page_margin goes with refine_scope='page'")
        if confidence or posterior:
            raise ValueError("confidence and posteriors are defined on the strict lattice of one line: not at page scope")
        page_margin = int(page_margin)
    elif refine_scope == "page":
        raise ValueError("process_batch refines at page scope only with page_margin=...: pass it, or call "
                         "forced.refine_pages(..., scope=\"page\")")
    pages, transcripts = list(pages), list(transcripts)
    n = len(pages)
    if locate and tsc.integer_scoring(seq_align_params) is None:
        raise ValueError("locate=True takes integer match/mismatch scoring systems only")
    # one model for all pages, or one per page (the reference's two manuscripts have a model each, alignToOCR.py:390-405):
    # pages are grouped by recogniser, every chunk has one, and the pipeline runs on across the groups
    if isinstance(ocropus_model, (list, tuple)):
        if len(ocropus_model) != n:
            raise ValueError("a list of models needs one entry per page")
        recs = [_recognizer_for(m) for m in ocropus_model]
    else:
        recs = [_recognizer_for(ocropus_model)] * n
    if locate and any(pb.codec_code_points(r.model.codec) is None for r in recs):
        raise ValueError("locate=True needs a recogniser codec of single characters")
    ratio = None
    if refine:
        from . import forced
        ratio = forced.refine_checks(seq_align_params, list({id(r): r for r in recs}.values()), min_agreement)
    groups = {}
    for k, r in enumerate(recs):
        groups.setdefault(id(r), (r, []))[1].append(k)
    if not groups:
        groups[0] = (_recognizer_for(ocropus_model), [])
    # pages that still need the preprocessing kernels (page images) take larger chunks: their line finding waits for the
    # device several times per batch of pages, and those waits queue behind a previous chunk's recogniser
    # (measured at 64 pages, chunks of 8 / 16 / 32: normalised strips 1 410 / 1 515 / 1 515 pages/s, raw strips -- whose
    # normaliser returns its data-dependent widths with a device wait per chunk -- 670 / 866 / 1 005; page images ~450-500
    # whatever the chunk)
    images = any(not isinstance(pg, page_mod.PreparedPage) for pg in pages)
    raw = not images and any(st.prepared is None for pg in pages for st in getattr(pg, "strips", ()))
    C = PIPELINE_CHUNK_PAGES_IMAGES if images else (PIPELINE_CHUNK_PAGES_RAW if raw else PIPELINE_CHUNK_PAGES)
    lead = (C // LEAD_CHUNK_DIVISOR,) if LEAD_CHUNK_DIVISOR > 1 and not (images or raw) else ()   # (raw strips: measured, no gain)
    chunks = plan_chunks(list(groups.values()), C, lead)
    out_res, out_idx, out_arr, out_span, out_ref = [None] * n, [None] * n, [None] * n, [None] * n, [None] * n
    out_conf, out_post, out_scope = [None] * n, [None] * n, [None] * n
    out_omit = [None] * n if line_omit_q is not None else None
    def begin(job):
        rec, ks = job
        return PageChunk(rec, [pages[k] for k in ks], [transcripts[k] for k in ks], seq_align_params, parallel, locate, ks,
                         refine=ratio, confidence=confidence, posterior=posterior, page_margin=page_margin,
                         omit_q=line_omit_q, page_omit_q=page_omit_q)

    def collect(chunk):
        idx, arr = [], []
        res = chunk.finish(idx, arr)
        for j, k in enumerate(chunk.page_ids):
            out_res[k] = res[j]
            out_idx[k], out_arr[k] = idx[j], arr[j]
            if locate:
                out_span[k] = chunk.spans[j]
        if ratio is not None:
            first = chunk.first_line()
            for j, k in enumerate(chunk.page_ids):
                out_ref[k] = chunk.refined[int(first[j]):int(first[j + 1])]
            if line_omit_q is not None:
                for k, gone in zip(chunk.page_ids, chunk.omitted_pages()):
                    out_omit[k] = gone
        if page_margin is not None:
            for j, k in enumerate(chunk.page_ids):
                out_scope[k] = chunk.page_scope[j]
        if confidence:
            for k, c in zip(chunk.page_ids, forced.chunk_confidence(chunk, idx)):
                out_conf[k] = c
        if posterior:
            for k, c in zip(chunk.page_ids, forced.chunk_posterior(chunk, idx)):
                out_post[k] = c

    def deliver():
        # one entry per page, in page order, whichever path each chunk took (a chunk whose alignment does not fit the
        # integer kernels goes object by object on its own; callers zip these lists with the pages)
        if indices_out is not None:
            indices_out.extend(out_idx)
        if arrays_out is not None:
            arrays_out.extend(out_arr)
        if locate and spans_out is not None:
            spans_out.extend(out_span)
        if ratio is not None and refined_out is not None:
            refined_out.extend(out_ref)
        if line_omit_q is not None and omitted_out is not None:
            omitted_out.extend(out_omit)
        if confidence and confidence_out is not None:
            confidence_out.extend(out_conf)
        if posterior and posterior_out is not None:
            posterior_out.extend(out_post)
        if page_margin is not None and page_scope_out is not None:
            page_scope_out.extend(out_scope)
        return out_res
    if len(chunks) == 1:
        chunk = begin(chunks[0])
        chunk.launch()
        chunk.host_ahead()
        chunk.align()
        collect(chunk)
        return deliver()
    device = chunks[0][0].device
    streams = _ocr_streams(device)
    caller = torch.cuda.current_stream(device)
    for st_ in streams:
        st_.wait_stream(caller)                                  # whatever the caller enqueued before this call
    # Three stages per chunk: (1) begin + launch -- the recogniser's kernels enqueued; (2) align, once the chunk's
    # characters are back: abbreviations and the chunk's ONE aligner launch; (3) collect, once the alignment columns are
    # back: syllable boxes.  The device must never run dry, so a new chunk is launched BEFORE any second stage of the
    # iteration, and neither later stage may make the host wait: stage 2 is taken for the chunk launched two iterations
    # ago (its recogniser is over by the time the chunk before this one is running), stage 3 for the chunk whose aligner
    # launch was made one iteration ago (small kernels that slip onto CUs the recurrences leave free).
    # (Round 5's order -- stage 2 of the oldest chunk, THEN this chunk's launch, stage 3 behind it -- left the GPU idle for
    # ~2 ms per chunk while the host did stage 2: timeline in profiles/r06_pages_timeline_pinned.txt.)
    # The first stage's host half of chunk c + 1 (row layout, the pool's staging copies STARTED) is taken right behind
    # chunk c's launch: the copies then run under this iteration's later stages and the next launch finds them done.
    return _pb_pipeline(chunks, begin, collect, deliver, streams, caller)


def locate_book(pages, transcript, ocropus_model, seq_align_params=None):
    """[(a, b)] per page: where in `transcript` -- ONE string for the whole book -- each of `pages`, given IN READING
    ORDER, has its text.  locate=True searches every page on its own, and a passage the book repeats (a doxology, a
    refrain, the same antiphon on two feasts) goes to its first copy; here the pages are recognised in chunks, each
    page's text is the expanded OCR text locate=True searches with, and ONE chained search over all pages
    (textSeqCompare.SpanChainBatch) puts them in order: page p's span ends where page p + 1's
    begins, or before.  Every span then goes through snap_to_words, which widens OUTWARD to whole words: two
    neighbouring spans may therefore share the word that a page break splits.  `ocropus_model` is one model or a list
    with one per page.  ValueError up front, before any GPU work, for what the integer span search does not take: a
    scoring callable, non-integral numbers, a codec with multi-character entries."""
    pages = list(pages)
    n = len(pages)
    params = tsc.integer_scoring(seq_align_params)
    if params is None:
        raise ValueError("locate_book takes integer match/mismatch scoring systems only")
    if not isinstance(transcript, str):
        raise ValueError("locate_book takes the book's transcript as one string")
    if isinstance(ocropus_model, (list, tuple)):
        if len(ocropus_model) != n:
            raise ValueError("a list of models needs one entry per page")
        recs = [_recognizer_for(m) for m in ocropus_model]
    else:
        recs = [_recognizer_for(ocropus_model)] * n
    if any(pb.codec_code_points(r.model.codec) is None for r in recs):
        raise ValueError("locate_book needs a recogniser codec of single characters")
    if n == 0:
        return []
    groups = {}
    for k, r in enumerate(recs):
        groups.setdefault(id(r), (r, []))[1].append(k)
    o_cp = [None] * n
    for rec, ks in plan_chunks(list(groups.values()), PIPELINE_CHUNK_PAGES):
        chunk = PageChunk(rec, [pages[k] for k in ks], [transcript] * len(ks), seq_align_params, parallel, True, ks)
        chunk.launch()
        for k, cp in zip(ks, chunk.ocr_texts()[4]):
            o_cp[k] = cp
    t_cp = pb.code_points(transcript)
    alphabet = np.unique(np.concatenate([t_cp] + o_cp))
    device = recs[0].device
    with torch.cuda.stream(_nw_stream(device)):
        search = tsc.SpanChainBatch([np.searchsorted(alphabet, t_cp).astype(np.int32)],
                                    [[np.searchsorted(alphabet, a).astype(np.int32) for a in o_cp]], params, device=device)
        search.run()
        search.fetch_begin()
    found, _ = search.results(_timed_wait)
    return [snap_to_words(transcript, int(r[0]), int(r[1])) for r in found]


def process_book(pages, transcript, ocropus_model, seq_align_params=None, spans_out=None, **switches):
    """process_batch for the pages of a book, in reading order, against the book's ONE transcript string: locate_book
    finds every page's span (a, b), then process_batch(pages, [transcript[a:b] ...], ...) runs with `switches` (its
    keyword arguments: indices_out, arrays_out, refine, ...) passed through; spans_out receives the spans.  The result
    is that call's.  The pages are recognised TWICE -- once for the search, once inside process_batch; keeping the first
    pass's characters is a follow-up.  locate and spans_out are this function's own and not among the switches."""
    if "locate" in switches:
        raise ValueError("process_book locates the pages itself: no locate switch")
    pages = list(pages)
    spans = locate_book(pages, transcript, ocropus_model, seq_align_params)
    if spans_out is not None:
        spans_out.extend(spans)
    return process_batch(pages, [transcript[a:b] for a, b in spans], ocropus_model, seq_align_params, **switches)


def _pb_pipeline(chunks, begin, collect, deliver, streams, caller):
    """the loop of process_batch over its chunks (see the comment there); begin(job) returns a PageChunk, or whatever has
    its launch / host_ahead / align"""
    flight, aligned = [], []
    nxt = begin(chunks[0])
    for c, job in enumerate(chunks):
        chunk = nxt
        lane = streams[c % 2] if TWO_STREAMS else caller
        # begin() ran on the CALLER's stream: for raw strips and page images it enqueued device work there (the normaliser's
        # kernels write the rows, the metadata uploads, the zero-fill of the decoder's outputs) that this chunk's recogniser
        # reads -- the chunk's compute stream takes it all in before its first kernel.  (Host rows: nothing was enqueued
        # there and the wait is on an idle stream.)  Nothing else is ever put on the caller's stream inside this loop,
        # so this never orders a chunk behind another chunk's kernels.
        if lane is not caller:
            lane.wait_stream(caller)
        with torch.cuda.stream(lane):
            chunk.launch()
        nxt = begin(chunks[c + 1]) if c + 1 < len(chunks) else None
        chunk.host_ahead()
        flight.append(chunk)
        if aligned:
            collect(aligned.pop(0))
        if len(flight) > 2:
            oldest = flight.pop(0)
            oldest.align()
            aligned.append(oldest)
    for st_ in streams:
        caller.wait_stream(st_)
    for chunk in flight:                                          # the drain: every aligner launch as soon as its characters are
        chunk.align()                                             # back, the box assembly of a chunk under the next one's launch
        if aligned:
            collect(aligned.pop(0))
        aligned.append(chunk)
    for chunk in aligned:
        collect(chunk)
    return deliver()


def _timed_wait(event):
    t0 = time.perf_counter()
    event.synchronize()
    WAIT_SECONDS[0] += time.perf_counter() - t0


class PageChunk(object):
    """One chunk of process_batch: pages of one recogniser that go through the stages together.  The stages in order, and
    the fields each one fills (a field is None until then):

        PageChunk(...)   rec, pages, transcripts, params, locate, page_ids (the pages' places in the call); raw_dims, found
                         (find_lines_all per page), strips_per_page, all_strips, lines, widths, st (the recogniser's
                         state: rows laid out, staging copies STARTED), cps (the codec's code points; None: object path)
        launch()         decoded (the decoder's outputs on their way to the host)
        host_ahead()     syls_all, t_cp -- with locate t_cp_full alone: the spans are not known yet
        align()          line (the chunk-wide text line of every OCR character), boxes, texts, idxs, nw (the aligner's
                         batch, its columns on their way; None: the integer kernels do not take this chunk and finish()
                         goes object by object), syl_idxs and syl_boxes (idxs and boxes: what the syllables' boxes are
                         formed from); with locate also spans, and transcripts, syls_all, t_cp become those of the pages'
                         own spans; with refine also refining (forced.Refining: harvest, forced alignment and the refined
                         runs' columns enqueued behind the aligner, ONE download in place of the aligner's columns; with
                         page_margin a forced.PageRefining instead: harvest, windows and the page aligner)
        finish()         returns the pages' results; nw is given up (columns()); with refine the refinement's download is
                         taken in through replace_columns() and refined (a bool per line of the chunk) is filled, at
                         page scope also page_scope (a forced.PageScope per page), with omit_q also omitted (int32 per
                         line of the chunk: the characters its path left out, -1 for a line that was not aligned)

    Between align() and finish() a caller may change ONE thing, through replace_columns() (forced.refine_pages), which
    fills ops and puts other syl_idxs, syl_boxes.  Everything else is read, not written, outside the stages; line_table() and
    strip_geometry() derive what harvest and forced need from the fields."""
    __slots__ = ("rec", "pages", "transcripts", "params", "locate", "page_ids", "raw_dims", "found", "strips_per_page",
                 "all_strips", "lines", "widths", "st", "cps", "decoded", "syls_all", "t_cp", "t_cp_full", "line", "boxes",
                 "texts", "idxs", "nw", "spans", "ops", "syl_idxs", "syl_boxes", "refine", "refining", "refined", "confidence",
                 "conf", "posterior", "post", "page_margin", "page_scope", "omit_q", "omitted", "page_omit_q")

    def __init__(self, rec, pages, transcripts, seq_align_params, workers, locate=False, page_ids=None, refine=None,
                 confidence=False, posterior=False, page_margin=None, omit_q=None, page_omit_q=None):
        """first stage, host part: line finding, the layout of the chunk's rows, the staging copies STARTED (pool threads).
        refine: None, or the minimum agreement (num, den) -- the chunk's accepted lines get their boxes from forced
        alignment (forced.Refining: enqueued by align(), taken in by finish()); confidence (with refine): the refinement
        computes the per-character confidences as well, and finish() leaves them in conf (forced.chunk_confidence);
        posterior (with refine): likewise the sum-product posteriors, left in post (forced.chunk_posterior);
        page_margin (with refine): None, or the margin at which the chunk is refined at PAGE scope instead
        (forced.PageRefining; finish() leaves a forced.PageScope per page in page_scope);
        omit_q (with refine at line scope, strict lattice): None, or the price (forced.omit_units) of a character the
        forced alignment may leave out (forced.Refining(omit_q=...); finish() leaves the counts per line in omitted);
        page_omit_q (with page_margin): None, or the price of a character the PAGE's one path may leave out
        (forced.PageRefining(omit_q=...); the counts per refined page are PageScope.omitted)"""
        self.rec, self.pages, self.transcripts, self.params = rec, pages, transcripts, seq_align_params
        self.locate, self.page_ids = bool(locate), page_ids
        self.refine, self.refining, self.refined = refine, None, None
        self.confidence, self.conf = bool(confidence) and refine is not None, None
        self.posterior, self.post = bool(posterior) and refine is not None, None
        self.page_margin, self.page_scope = (page_margin if refine is not None else None), None
        self.omit_q, self.omitted = (omit_q if refine is not None else None), None
        self.page_omit_q = page_omit_q if self.page_margin is not None else None
        self.raw_dims = [_raw_dim(pg) for pg in pages]       # bad page types fail before any GPU work
        self.found = find_lines_all(list(pages), workers=workers)
        self.strips_per_page = [f[3] for f in self.found]
        self.all_strips = [st for strips in self.strips_per_page for st in strips]
        prepared = page_mod.prepared_lines(self.all_strips, workers=workers)
        self.lines = [xs for xs, _ in prepared]
        self.widths = [w for _, w in prepared]
        self.st = rec.prepare(self.lines, defer=True)
        self.cps = pb.codec_code_points(rec.model.codec)
        self.decoded = self.syls_all = self.t_cp = self.t_cp_full = self.line = self.boxes = self.texts = self.idxs = None
        self.nw = self.spans = self.ops = self.syl_idxs = self.syl_boxes = None

    def launch(self, want_probs=False):
        """first stage, device part: the rows' transfer, the recogniser kernels and the download of the decoded characters
        -- everything enqueued, nothing waited for but the staging copies.  want_probs: the recogniser keeps its
        probabilities (forced.refine_pages)"""
        st = self.st
        self.rec.complete(st)
        self.rec.run(st, want_probs=bool(want_probs) or self.refine is not None)
        # the decoder's outputs come back through pinned buffers behind an event of their own: a plain .cpu() issued later
        # would queue behind whatever the stream has been given since (the next chunk's kernels)
        self.decoded = _native.download_begin([st["dec_t"], st["dec_c"], st["dec_n"]])

    def host_ahead(self):
        """the host work of a chunk that needs no OCR result -- syllables and code points of the transcripts -- done AFTER the
        chunk's kernels have been enqueued: nothing the device is waiting for stands behind it"""
        if self.locate:                    # the transcripts are longer than the pages: only their code points, each distinct
            seen = {}                      # string OBJECT once; the syllables wait for the spans (_locate)
            for tr in self.transcripts:
                if id(tr) not in seen:
                    seen[id(tr)] = pb.code_points(tr)
            self.t_cp_full = [seen[id(tr)] for tr in self.transcripts]
        else:
            self._own_transcripts(self.transcripts)

    def _own_transcripts(self, transcripts):
        self.transcripts = transcripts
        self.syls_all = [latsyl.syllabify_text(tr) for tr in transcripts]
        self.t_cp = [pb.code_points(tr) for tr in transcripts]

    def first_line(self):
        """pages + 1 integers: page p owns the chunk's lines first_line[p] .. first_line[p + 1]"""
        out = np.zeros(len(self.pages) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in self.strips_per_page], out=out[1:])
        return out

    def omitted_pages(self):
        """after finish() of a chunk that refined with omit_q: per page the int32 counts of its text lines, cut from
        omitted as process_batch cuts refined"""
        first = self.first_line()
        return [np.asarray(self.omitted[int(a):int(b)], dtype=np.int32).copy() for a, b in zip(first[:-1], first[1:])]

    def strip_geometry(self, lines=None):
        """(x_min, y_min, y_max) of the chunk's strips, or of those at the indices `lines`: int64 arrays"""
        strips = self.all_strips if lines is None else [self.all_strips[q] for q in lines]
        x_min = np.array([s.offset_x for s in strips], dtype=np.int64)
        y_min = np.array([s.offset_y for s in strips], dtype=np.int64)
        return x_min, y_min, y_min + np.array([s.height for s in strips], dtype=np.int64)

    def line_table(self):
        """after align(), what harvest.harvest_alignment takes besides the batch: (o_line: per page the chunk-wide line of
        every expanded OCR character, int32; line_first; T: the timesteps of every line, int32)"""
        line = np.asarray(self.line, dtype=np.int64)
        o_line = [line[np.asarray(idx, dtype=np.int64)].astype(np.int32) for idx in self.idxs]
        return o_line, self.first_line(), np.asarray(self.st["T_host"], dtype=np.int32)[:len(self.all_strips)]

    def ocr_texts(self):
        """after launch(), integer path (cps is not None): the chunk's decoded characters taken in -- (texts: per page the
        expanded OCR text, idxs: per page the chunk-wide character each of its positions came from, boxes, line: the
        chunk-wide text line of every character, o_cp: the texts' code points)"""
        rec, st = self.rec, self.st
        # ---- every character of every line: code points + boxes (alignToOCR.py:160-182) ----
        nlines = len(self.all_strips)
        dec_t, dec_c, dec_n = self.decoded.wait(_timed_wait)
        rec.check_status(dec_n)                              # the device's status word travels behind the counts
        dec_n = dec_n[:nlines].astype(np.int64) if nlines else np.zeros(0, np.int64)
        x_min, y_min, y_max = self.strip_geometry()
        line, cp, boxes = pb.chars_of_batch(dec_t, dec_c, dec_n, st["row_start_host"], st["T_host"],
                                            np.asarray(self.widths, dtype=np.int64), x_min, y_min, y_max, self.cps, ocr.PAD)
        first_char = np.searchsorted(line, self.first_line())  # characters of page k: first_char[k] .. first_char[k+1]

        # ---- abbreviations, then one NW launch for all pages (alignToOCR.py:251-276) ----
        texts, idxs = [], []
        for k in range(len(self.pages)):
            a, b = int(first_char[k]), int(first_char[k + 1])
            text = cp[a:b].astype('<u4').tobytes().decode('utf-32-le')
            text, idx = pb.expand_abbreviations(text, np.arange(a, b), latsyl.abbreviations)
            texts.append(text)
            idxs.append(idx)
        return texts, idxs, boxes, line, [pb.code_points(tx) for tx in texts]

    def align(self):
        """second stage, first half: characters and boxes of every line, abbreviations, ONE NW launch for the chunk's pages
        and the download of its alignment columns STARTED"""
        rec, st = self.rec, self.st
        params = tsc.integer_scoring(self.params)
        if params is None or self.cps is None:
            if self.locate:
                raise ValueError("locate=True needs the integer span search: no scoring callable, integral scoring numbers, "
                                 "a codec of single characters")
            if self.refine is not None:
                raise ValueError("refine needs the integer aligner: no scoring callable, integral scoring numbers, a codec "
                                 "of single characters")
            return

        nlines = len(self.all_strips)
        texts, idxs, boxes, line, o_cp = self.ocr_texts()
        if self.locate:
            self._locate(o_cp, params)                       # from here on the chunk's transcripts are the pages' own spans
        t_cp = self.t_cp
        alphabet = np.unique(np.concatenate(t_cp + o_cp)) if (t_cp or o_cp) else np.zeros(0, np.int64)
        self.texts, self.idxs, self.boxes = texts, idxs, boxes
        self.syl_idxs, self.syl_boxes = idxs, boxes          # what the syllables' boxes are formed from (replace_columns)
        self.line = line                                     # the chunk-wide line of every character (harvest.harvest_pages)
        # (the aligner's inputs come from the host and its buffers are the side stream's own: nothing to wait for)
        with torch.cuda.stream(_nw_stream(rec.device)):
            try:
                batch = tsc.NWBatch([np.searchsorted(alphabet, a).astype(np.int32) for a in t_cp],
                                    [np.searchsorted(alphabet, a).astype(np.int32) for a in o_cp], params)
                batch.run()
                if self.refine is not None and batch.nprob and nlines:
                    # harvest, forced alignment and the refined runs' columns right behind the aligner, on its stream; ONE
                    # download carries what finish() needs, in place of the aligner's columns
                    from . import forced
                    if self.page_margin is not None:
                        self.refining = forced.PageRefining(self, batch, self.refine, self.page_margin, omit_q=self.page_omit_q)
                    elif self.omit_q is not None:
                        self.refining = forced.Refining(self, batch, self.refine, omit_q=self.omit_q)
                    else:
                        self.refining = forced.Refining(self, batch, self.refine, confidence=self.confidence,
                                                        posterior=self.posterior)
                else:
                    batch.fetch_begin()
                self.nw = batch
            except OverflowError:
                if self.refine is not None:
                    raise ValueError("refine: a page's alignment is too large for the integer aligner")

    def _locate(self, o_cp, params):
        """locate=True: ONE span search for the chunk -- every page's expanded OCR text against the code points of its
        (longer) transcript, a transcript shared by several pages uploaded once -- the spans downloaded (three ints per page:
        the one host wait this mode adds) and snapped to words; the chunk's transcripts become the spans, and only those
        are syllabified."""
        full, t_full = self.transcripts, self.t_cp_full
        distinct = {}
        for a in t_full:
            distinct.setdefault(id(a), a)
        alphabet = np.unique(np.concatenate(list(distinct.values()) + o_cp)) if (distinct or o_cp) else np.zeros(0, np.int64)
        ids = {key: np.searchsorted(alphabet, a).astype(np.int32) for key, a in distinct.items()}
        with torch.cuda.stream(_nw_stream(self.rec.device)):
            search = tsc.SpanBatch([ids[id(a)] for a in t_full], [np.searchsorted(alphabet, a).astype(np.int32) for a in o_cp],
                                   params)
            search.run()
            search.fetch_begin()
        found = search.results(_timed_wait)
        self.spans = [snap_to_words(tr, int(r[0]), int(r[1])) for tr, r in zip(full, found)]
        self._own_transcripts([tr[a:b] for tr, (a, b) in zip(full, self.spans)])

    def columns(self, waiter=None):
        """after align(): the alignment columns per page, waited for here; the aligner's batch is given up"""
        ops, self.nw = self.nw.results(waiter), None
        return ops

    def replace_columns(self, ops, idxs, boxes):
        """the ONE thing a caller may change between align() and finish(): per page the alignment columns to form the
        syllables' boxes from, per page the row of `boxes` of every OCR character of those columns, and the box array
        [k, 4] itself -- in place of the aligner's columns, idxs and boxes (forced.refine_pages: the refined lines' runs)"""
        self.ops, self.syl_idxs, self.syl_boxes = ops, idxs, boxes

    def _finish_objects(self, indices_out):
        """finish(), object by object (CharBox lists, alignToOCR.py:247-330 per page): the path for scoring callables /
        non-integral numbers and for codecs with multi-character entries."""
        rec, T = self.rec, self.st["T_host"]
        decoded = rec.decoded(self.st)
        chars_per_page, k = [], 0
        for strips in self.strips_per_page:
            all_chars = []
            for strip in strips:
                llocs = rec.llocs(decoded[k], int(T[k]), self.widths[k])
                chars_from_llocs(llocs, strip.offset_x, strip.offset_y, strip.offset_y + strip.height, all_chars)
                k += 1
            chars_per_page.append(expand_abbreviations(all_chars))
        pairs = [(list(tr), [c.char for c in chars]) for tr, chars in zip(self.transcripts, chars_per_page)]
        alignments = tsc.perform_alignment_batch(pairs, self.params)
        results = []
        for raw_dim, f, tr, chars, al in zip(self.raw_dims, self.found, self.transcripts, chars_per_page, alignments):
            image, angle, lp = f[0], f[2], f[4]
            idx = [] if indices_out is not None else None
            syl_boxes, all_chars_copy = align_page(tr, chars, angle, image.dim, raw_dim,
                                                   self.params, alignment=al, indices=idx, expanded=True)
            if indices_out is not None:
                indices_out.append(idx)
            results.append((syl_boxes, image, lp, all_chars_copy))
        return results

    def finish(self, indices_out, arrays_out):
        """second stage, second half: the alignment columns (waited for here), syllable boxes (alignToOCR.py:277-328)"""
        transcripts, raw_dims, found, syls_all = self.transcripts, self.raw_dims, self.found, self.syls_all
        if self.refining is not None:         # the refinement's one download in place of the aligner's columns
            refining, self.refining, self.nw = self.refining, None, None
            refining.complete(self, _timed_wait)
            self.refined, self.conf, self.post = refining.refined, refining.conf, refining.post
            self.page_scope = getattr(refining, "scope", None)
            if self.omit_q is not None:
                self.omitted = refining.omitted
        elif self.refine is not None:
            self.refined = np.zeros(len(self.all_strips), dtype=bool)
            if self.omit_q is not None:               # nothing was launched: no line was aligned
                self.omitted = np.full(len(self.all_strips), -1, dtype=np.int32)
            if self.page_margin is not None:          # no text line in the whole chunk: nothing was launched
                from . import forced
                self.page_scope = forced.page_scope_without_lines(self, omit=self.page_omit_q is not None)
        all_ops = self.ops                    # forced.refine_pages: the columns are here already, the refined lines' replaced
        if all_ops is None and self.nw is None:   # a scoring callable / non-integral numbers / a multi-character codec / too large
            res = self._finish_objects(indices_out)
            if arrays_out is not None:            # the same [k, 4] arrays as the array path hands over: one entry per page
                for r in res:
                    arrays_out.append(np.array([[b.ulx, b.uly, b.lrx, b.lry] for b in r[0]], dtype=np.int64).reshape(-1, 4))
            return res
        if all_ops is None:
            all_ops = self.columns(_timed_wait)
        texts, idxs, boxes = self.texts, self.idxs, self.boxes

        # ---- syllable boxes (alignToOCR.py:277-328): all plain pages in one set of array operations ----
        plain = [k for k in range(len(self.pages)) if pb.plain_page(transcripts[k], syls_all[k])]
        batched = dict(zip(plain, pb.syllable_boxes_batch(
            [transcripts[k] for k in plain], [syls_all[k] for k in plain], [all_ops[k] for k in plain],
            [self.syl_idxs[k] for k in plain], self.syl_boxes, [found[k][2] for k in plain], [found[k][0].dim for k in plain],
            [raw_dims[k] for k in plain])))
        results = []
        for k, (raw_dim, f, tr) in enumerate(zip(raw_dims, found, transcripts)):
            image, angle, lp = f[0], f[2], f[4]
            chars_seq = pb.BoxSeq(texts[k], boxes[idxs[k]], CharBox)          # (a str is a sequence of its characters)
            if k in batched:
                which, sb = batched[k]
                named = [s for s in syls_all[k] if len(s) >= 1]
                syl_seq = pb.BoxSeq([named[w] for w in which], sb, CharBox)
                which = which.tolist()
            else:                                             # characters `re` would interpret: object path
                which = []
                al = tsc.ops_to_alignment(all_ops[k], list(tr), list(texts[k]))
                syl_boxes, _ = align_page(tr, list(chars_seq), angle, image.dim, raw_dim, self.params,
                                          alignment=al, indices=which, expanded=True)
                sb = np.array([[b.ulx, b.uly, b.lrx, b.lry] for b in syl_boxes], dtype=np.int64).reshape(-1, 4)
                syl_seq = syl_boxes
            if indices_out is not None:
                indices_out.append(which)
            if arrays_out is not None:
                arrays_out.append(sb)
            results.append((syl_seq, image, lp, chars_seq))
        return results


def process(raw_image,
            transcript,
            ocropus_model,
            seq_align_params=None,
            wkdir_name='wkdir_ocropy',
            parallel=parallel,
            median_line_mult=median_line_mult,
            existing_ocr_pickle=None,
            existing_preproc_images=None,
            verbose=True,
            locate=False,
            spans_out=None,
            refine=False,
            min_agreement=0.9,
            refine_scope="line",
            margin=16,
            omit=None,
            confidence=False,
            confidence_out=None,
            posterior=False,
            posterior_out=None,
            page_omit=None,
            page_confidence=False,
            page_posterior=False,
            omit_confidence=False):
    '''
    given a text layer @raw_image and a string transcript @transcript, performs OCR on the text
    lines and aligns the results to the transcript text (reference alignToOCR.py:187-330).
    Returns (syl_boxes, image, lines_peak_locs, all_chars), or None when OCR fails.
    locate: @transcript may be longer than the page; the page's own span is found first and appended to spans_out as
    (a, b) (see align_page); the boxes are those of process(raw_image, transcript[a:b], ...).
    refine: the page goes through forced.refine_pages -- the lines whose piece of the transcript the harvest rule accepts
    at @min_agreement get a box per transcript character from forced alignment, the others stay as they are.
    refine_scope="page": forced.refine_pages(scope="page", margin=@margin) -- one best path through all lines of the page
    gives EVERY transcript character a box if the page is eligible for it, else the page comes
    back unrefined.
    omit (with refine, line scope): the price in bits of a transcript character the forced alignment may leave out
    (forced.refine_pages(omit=...)); None: every character of an accepted line must be there.
    confidence (with refine, line scope, no omit: forced.refine_pages' ValueError otherwise): the page's
    forced.PageConfidence is appended to confidence_out, as process_batch hands it over.
    posterior (with refine, line scope, no omit: forced.refine_pages' ValueError otherwise): the page's
    forced.PagePosterior (sum-product posteriors per character and syllable, the text's
    likelihood per line) is appended to posterior_out.  As with confidence, the switch alone decides what runs: with
    posterior_out=None the posteriors are computed and dropped.
    page_omit (with refine and refine_scope="page": forced.refine_pages' ValueError otherwise): the price in bits of a
    transcript character the page's one path may leave out (forced.refine_pages(page_omit=...));
    such a character gets no box, and a page with more transcript characters than frames is refined all the same.
    page_confidence (with refine and refine_scope="page", no page_omit: forced.refine_pages' ValueError otherwise): the
    page's forced.PageConfidence from the max-marginals of the page's one lattice is appended
    to confidence_out; its rival states are PAGE states, and a page that was not refined has no values.
    page_posterior (with refine and refine_scope="page", no page_omit: forced.refine_pages' ValueError otherwise): the
    page's forced.PagePosterior from the sum-product posteriors of the page's one lattice is
    appended to posterior_out, page_loglik_bits = log2 P(transcript | page) with it; its rival states are PAGE states,
    loglik_bits holds None per line, and a page that was not refined has no values.
    omit_confidence (with refine, line scope and omit: forced.refine_pages' ValueError otherwise): the page's
    forced.PageConfidence on the lattice with omission is appended to confidence_out: >= 0 for a
    present character, <= 0 for an omitted one, a syllable's value over its present characters.
    '''
    if omit_confidence and not refine:
        raise ValueError("omit_confidence belongs to refine=True")
    if omit is not None and not refine:
        raise ValueError("omit belongs to refine=True")
    if page_omit is not None and not refine:
        raise ValueError("page_omit belongs to refine=True")
    if confidence and not refine:
        raise ValueError("confidence belongs to refine=True")
    if posterior and not refine:
        raise ValueError("posterior belongs to refine=True")
    if page_confidence and not refine:
        raise ValueError("page_confidence belongs to refine=True")
    if page_posterior and not refine:
        raise ValueError("page_posterior belongs to refine=True")
    if refine:
        from . import forced
        res = forced.refine_pages([raw_image], [transcript], ocropus_model, seq_align_params, min_agreement, locate,
                                  scope=refine_scope, margin=margin, omit=omit, confidence=confidence, posterior=posterior,
                                  page_omit=page_omit, page_confidence=page_confidence, page_posterior=page_posterior,
                                  omit_confidence=omit_confidence)
        if (posterior or page_posterior) and posterior_out is not None:
            posterior_out.append(forced.PagePosterior(res, 0))
        if (confidence or page_confidence or omit_confidence) and confidence_out is not None:
            confidence_out.append(forced.result_confidence(res, 0))
        if locate and spans_out is not None:
            spans_out.append(res.spans[0])
        return res.results[0]
    if locate and tsc.integer_scoring(seq_align_params) is None:
        raise ValueError("locate=True takes integer match/mismatch scoring systems only")
    raw_dim = _raw_dim(raw_image)
    image, eroded, angle, cc_strips, lines_peak_locs = find_lines_all([raw_image], workers=1)[0]

    all_chars = []
    if existing_ocr_pickle:
        try:
            all_chars = load_ocr_pickle(existing_ocr_pickle)
            print('using pickled ocr results in {}...'.format(existing_ocr_pickle))
        except IOError:
            print('Pickle file {} not found - performing ocr instead'.format(existing_ocr_pickle))
        except AttributeError:
            print('Pickle error: re-performing ocr')

    if not all_chars:
        try:
            all_chars = perform_ocr_with_ocropus(cc_strips, ocropus_model, wkdir_name=wkdir_name,
                                                 parallel=parallel)
        except ocr.RecognitionError:
            print('OCRopus failed! Skipping current file.')
            return None

    syl_boxes, all_chars_copy = align_page(transcript, all_chars, angle, image.dim, raw_dim,
                                           seq_align_params, locate=locate, spans_out=spans_out)
    return syl_boxes, image, lines_peak_locs, all_chars_copy


def to_JSON_dict(syl_boxes, lines_peak_locs):
    '''
    output of process() -> the dict the MEI-encoding job consumes (alignToOCR.py:333-351).
    'median_line_spacing' is the 75th percentile of the line gaps, as in the reference.
    '''
    data = {'median_line_spacing': np.quantile(np.diff(lines_peak_locs), 0.75), 'syl_boxes': []}
    for s in syl_boxes:
        data['syl_boxes'].append({'syl': s.char,
                                  'ul': [int(s.ul[0]), int(s.ul[1])],
                                  'lr': [int(s.lr[0]), int(s.lr[1])]})
    return data
