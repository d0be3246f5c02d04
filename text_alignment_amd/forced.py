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
`refine_pages(scope="page")` lets the lattice decide which character lies on which line: ONE best path through the
frames of all lines of a page (csrc/ta_forced_page.hip: `ta_forced_align_pages`; DESIGN.md section 14.8, checker
tests/forced_page_ref.py), the harvest table supplying only a corridor of characters per line (`page_windows`), so every
transcript character of an eligible page gets a box whatever the decoder emitted.  `align_page_lines` does it for the
line images of one page and one text.
`page_omit` (forced_page_alignment(omit_q=...), align_page_lines(omit=...), refine_pages(scope="page", page_omit=...)): the
page's one path may leave transcript characters out at a price per character (csrc/ta_forced_page_omit.hip:
`ta_forced_align_pages_omit`; DESIGN.md section 14.12, checker tests/forced_page_omit_ref.py) -- page scope for the pages
whose transcript disagrees with the ink.  Every page with windows then has a path, more characters than frames or not.
NOT measured: the share of real pages this refines, the right page_omit, the right margin.
`omit` (forced_alignment(omit_q=...), align_lines, refine_pages at line scope): the lattice may leave characters of the
text out at a price per character (csrc/ta_forced_omit.hip: `ta_forced_align_omit`; DESIGN.md section 14.9, checker
tests/forced_omit_ref.py), so an abbreviation or a spelling variant costs a penalty instead of a box over its neighbours'
ink.  No value of `omit` has been validated on real pages.  Inside the pipeline
(alignToOCR.process_batch(..., refine=True, line_omit=BITS)) `Refining(omit_q=...)` runs it
device-resident: `ta_forced_align_omit_lines` on the harvest's slots, `ta_refine_columns_omit` (csrc/ta_refine.hip; checker
tests/refine_omit_ref.py) on its frames, the counts per line in the same download, the box rows of the present characters
formed by `present_box_rows`.
`confidence` (forced_confidence, align_lines, refine_pages at line scope without `omit`): per character of an aligned line
how far the best path that keeps it on its peak frame lies above the best path that puts anything else there, and which
state that rival is (csrc/ta_forced_conf.hip: `ta_forced_confidence`; DESIGN.md section 14.10, checker
tests/forced_conf_ref.py) -- max-marginals on one line's strict lattice, not a posterior; no threshold has been validated
on real pages.  Inside the pipeline (alignToOCR.process_batch(..., refine=True, confidence=True)) `Refining` computes it
device-resident: `ta_forced_confidence_lines` on the aligner's slots and peaks, `ta_confidence_pages`
(csrc/ta_refine_conf.hip; checker tests/refine_conf_ref.py) per transcript character and syllable, in the same download.
`omit_confidence` (forced_omit_confidence, omit_queries, align_lines, refine_pages at line scope WITH `omit`): the same
ranking on the lattice with omission, by a backward recursion of its own (csrc/ta_forced_omit_conf.hip:
`ta_forced_omit_confidence`; DESIGN.md section 14.18, checker tests/forced_omit_conf_ref.py) -- >= 0 for a present character
at its peak, <= 0 for an omitted one at the two frames around the place it was jumped at, minus it an UPPER bound of what
the best path would lose if the character had to appear.  Not at page scope, not inside process_batch; no threshold has
been validated on real pages.
`posterior` (forced_posterior, align_lines, refine_pages at line scope without `omit`): the sum-product counterpart -- per
character the probability, all CTC paths summed, that it holds its peak frame, the largest such probability of any other
state, and per line log2 P(text | line) (csrc/ta_forced_post.hip: `ta_forced_posterior`; DESIGN.md section 14.11, checker
tests/forced_post_ref.py, bit for bit).  Inside the pipeline (alignToOCR.process_batch(..., refine=True, posterior=True))
`Refining` computes it device-resident as it does the confidence: `ta_forced_posterior_lines` on the aligner's slots and
peaks, `ta_posterior_pages` (csrc/ta_refine_conf.hip; checker tests/refine_post_ref.py) per transcript character and
syllable, in the same download.  Nothing about real pages has been measured.
`page_confidence` (forced_page_confidence, align_page_lines(confidence=True), refine_pages(scope="page",
page_confidence=True)): the max-marginal confidence on the page's ONE lattice -- windows that move from line to line, no
character across a line break -- with a backward recursion of its own (csrc/ta_forced_page_conf.hip:
`ta_forced_page_confidence`; DESIGN.md section 14.13, checker tests/forced_page_conf_ref.py); a rival is a PAGE state.
`page_posterior` (forced_page_posterior, align_page_lines(posterior=True), refine_pages(scope="page",
page_posterior=True)): the sum-product posteriors on the page's ONE lattice and log2 P(transcript | page), the fit measure
that does not depend on how the harvest cut the transcript into lines (csrc/ta_forced_page_post.hip:
`ta_forced_page_posterior`; DESIGN.md section 14.15, checker tests/forced_page_post_ref.py, bit for bit).  Not inside
process_batch; no threshold on a posterior and nothing about real pages has been measured.
`PageRefining` is page scope inside the page pipeline (alignToOCR.process_batch(..., refine=True, refine_scope="page",
page_margin=M)): windows and eligibility formed on the device (csrc/ta_page_windows.hip:
`ta_page_windows`), the page aligner gated by them and sized by a cap per page instead of host windows
(csrc/ta_forced_page_gated.hip: `ta_forced_align_pages_gated`), ONE download; per page the result is refine_pages' at
page scope on that page alone.
How many lines of real manuscript pages get refined has NOT been measured, nor the corridor (`margin`) real pages need,
nor the share of real pages that are eligible for page scope.
"""
import numpy as np
import torch

from . import _native

FIELDS = _native.TA_FORCED_FIELDS               # t_first, t_last, t_peak
MAX_TARGET = _native.TA_FORCED_MAX_TARGET
MAX_T = _native.TA_TRAIN_MAX_T                  # timesteps of one line
OK, BOUNDS, LABEL = _native.TA_FORCED_OK, _native.TA_FORCED_BOUNDS, _native.TA_FORCED_LABEL
NOPATH = _native.TA_FORCED_NOPATH
CONF_QUERY = _native.TA_FORCED_QUERY            # a line's query frames leave 0 .. T - 1 or decrease
CONF_SKIPPED = _native.TA_FORCED_SKIPPED        # ta_forced_confidence_lines left a slot alone that the aligner had refused
STATUS = {OK: "ok", BOUNDS: "the line's own numbers are out of bounds", LABEL: "a label outside 1 .. no - 1",
          CONF_QUERY: "a query frame outside 0 .. T - 1, or query frames that decrease",
          CONF_SKIPPED: "the aligner did not align the slot"}
PAGE_FIELDS = _native.TA_FORCED_PAGE_FIELDS     # line, t_first, t_last, t_peak
PAGE_STATUS = {OK: "ok", BOUNDS: "the page's own numbers are out of bounds", LABEL: "a label outside 1 .. no - 1",
               NOPATH: "no path through the page's windows"}
PAGE_CONF_STATUS = dict(PAGE_STATUS)
PAGE_CONF_STATUS[CONF_QUERY] = "a query outside its page, line or window, or queries that decrease"
DEFAULT_MARGIN = 16             # characters a line's window reaches beyond its harvested piece: a guess, NOT measured
# RefineResult.page_scope, per page: 0 = refined at page scope, else why it came back unrefined
# (the numbers are the header's TA_PAGE_SCOPE_*: ta_page_windows writes them on the device)
(PAGE_REFINED, PAGE_NOT_PLAIN, PAGE_HARVEST, PAGE_CLASS0, PAGE_NO_TEXT, PAGE_WINDOWS, PAGE_FRAMES, PAGE_NO_PATH) = (
    _native.TA_PAGE_SCOPE_REFINED, _native.TA_PAGE_SCOPE_NOT_PLAIN, _native.TA_PAGE_SCOPE_HARVEST, _native.TA_PAGE_SCOPE_CLASS0,
    _native.TA_PAGE_SCOPE_NO_TEXT, _native.TA_PAGE_SCOPE_WINDOWS, _native.TA_PAGE_SCOPE_FRAMES, _native.TA_PAGE_SCOPE_NO_PATH)
PAGE_SCOPE = {0: "refined", 1: "the page's syllables take the object path", 2: "the harvest refused the page",
              3: "a transcript character outside the codec", 4: "no transcript characters",
              5: "no lines, or a window wider than %d characters" % MAX_TARGET, 6: "fewer frames than characters",
              7: "no path through the page's windows"}
# with page_omit the codes above keep their numbers -- PAGE_FRAMES and PAGE_NO_PATH do not occur,
# every page has a path -- and two follow
PAGE_TOO_LONG, PAGE_ALL_OMITTED = _native.TA_PAGE_SCOPE_TOO_LONG, _native.TA_PAGE_SCOPE_ALL_OMITTED
PAGE_MAX_CHARS, PAGE_MAX_FRAMES = 1 << 20, 1 << 25      # what ta_forced_align_pages_omit takes per page
PAGE_OMIT_SCOPE = dict(PAGE_SCOPE)
PAGE_OMIT_SCOPE.update({6: "not used with page_omit: a page may hold more characters than frames",
                        8: "more than 2^20 characters or 2^25 frames", 9: "the path holds no character at all"})


OMIT_MAX = _native.TA_FORCED_OMIT_MAX           # 1024 bits
OMITTED = _native.TA_FORCED_OMITTED             # all three fields of a character the path does not enter
NO_CONFIDENCE = _native.TA_NO_CONFIDENCE        # RefineResult.char_confidence of a character on no refined line
CONF_PAGES_STATUS = {_native.TA_CONF_PAGES_OK: "ok", _native.TA_CONF_PAGES_BOUNDS: "the page's own numbers are out of bounds",
                     _native.TA_CONF_PAGES_RANGE: "a syllable's range leaves the page's characters",
                     _native.TA_CONF_PAGES_TABLE: "a refined line's kept characters leave the page's",
                     _native.TA_CONF_PAGES_SLOT: "a refined line has no slot",
                     _native.TA_CONF_PAGES_STATUS: "a refined line's confidence status is not ok"}


def omit_units(bits):
    """the price of an omitted character, given in bits, in the integer units of the emission score (2^-16 bit):
    round(bits * 65536).  ValueError outside 0 .. 1024 bits or for something that is not a number."""
    if isinstance(bits, (bool, np.bool_)) or not isinstance(bits, (int, float, np.integer, np.floating)):
        raise ValueError("omit is a number of bits")
    if not 0 <= bits <= 1024:                            # NaN fails both comparisons
        raise ValueError("omit must lie in 0 .. 1024 bits")
    return int(round(float(bits) * 65536))


def _host_ints(x, dtype, name):
    a = np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=dtype).reshape(-1)
    if a.size and a.min() < 0:
        raise ValueError("%s must not be negative" % name)
    return a


def _line_arguments(probs, row_off, T, labels, lab_off, L):
    """the first checks of _line_list_call: (rows, no, row_off, lab_off, T32, L32, n, labels on the
    host or None, labels on the device or None, nlabels)"""
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
    if isinstance(labels, torch.Tensor) and labels.is_cuda:
        if labels.dtype != torch.int32 or not labels.is_contiguous():
            raise ValueError("labels on the device must be a contiguous int32 tensor")
        d_labels, nlabels = labels, int(labels.numel())
    else:
        d_labels, nlabels = None, None
        labels = _host_ints(labels, np.int32, "labels")
        nlabels = len(labels)
    return rows, no, row_off, lab_off, T32, L32, n, labels, d_labels, nlabels


def _omit_price(omit_q):
    """omit_q as the library takes it; ValueError for what is no integer in 0 .. OMIT_MAX"""
    if isinstance(omit_q, (bool, np.bool_)) or not isinstance(omit_q, (int, np.integer)) or not 0 <= omit_q <= OMIT_MAX:
        raise ValueError("omit_q is an integer in 0 .. %d (omit_units)" % OMIT_MAX)
    return int(omit_q)


def _query_ints(q, name):
    """a query array, host integers or an int32 device tensor: (the device tensor or None, the flat int32 host array or
    None, its length).  What lies outside a line or a page is the kernel's to refuse."""
    if isinstance(q, torch.Tensor) and q.is_cuda:
        if q.dtype != torch.int32 or not q.is_contiguous():
            raise ValueError("%s on the device must be a contiguous int32 tensor" % name)
        return q, None, int(q.numel())
    q = np.ascontiguousarray(q.cpu().numpy() if isinstance(q, torch.Tensor) else q, dtype=np.int32).reshape(-1)
    return None, q, len(q)


def _upload(fixed, optional, dev):
    """ONE packed upload of the host arrays `fixed` and of those of `optional` = [(device tensor or None, host array or
    None)] that are not on the device yet (an empty one as one zero): (the device tensors of `fixed`, those of `optional`)"""
    host = [np.zeros(1, np.int32) if not len(a) else a for d, a in optional if d is None]
    got = _native.upload_packed(list(fixed) + host, dev)
    rest = got[len(fixed):]
    return got[:len(fixed)], [d if d is not None else rest.pop(0) for d, _ in optional]


def _launch(entry, args, outs, ws_bytes, dev, _fill):
    """the call of the library function `entry` on torch's current stream: `args`, then the workspace and its bytes, the
    outputs `outs` = [(name, tensor, size)] and the stream; _fill goes over the workspace and the outputs first"""
    work = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    if _fill is not None:
        for t in [o for _, o, _ in outs] + [work]:
            t.view(torch.uint8).fill_(_fill)
    stream = torch.cuda.current_stream(dev)
    args = list(args) + [work.data_ptr(), ws_bytes] + [o.data_ptr() for _, o, _ in outs] + [stream.cuda_stream]
    _native.check(getattr(_native.lib, entry)(*args), entry)
    work.record_stream(stream)


def _pieces(ws):
    """workspace pieces of ws[i] bytes one behind the other: (their offsets, the bytes in all)"""
    ws_off = np.zeros(len(ws), dtype=np.int64)
    ws_off[1:] = np.cumsum(ws)[:-1]
    return ws_off, int(ws.sum())


_NO_QUERY = object()


def _line_list_call(entry, ws_bytes_of, takes, probs, row_off, T, labels, lab_off, L, _fill, per_label, per_line,
                    t_query=_NO_QUERY, omit_q=None, pairs=None, host=False):
    """what forced_alignment, forced_confidence, forced_posterior and forced_omit_confidence share: the checks, the
    workspace pieces sized by the library function `ws_bytes_of`, the packed upload, the outputs (per_label: [(name, torch
    dtype, trailing shape)], per_line: [(name, torch dtype)], then status per line) and the call of the library function
    named `entry` (`takes`: the name the refusal of a line's sizes gives).  t_query: the query array of the two entries that
    take one per label; omit_q: the price the entries with omission take; pairs: (q_char, q_frame, q_off, nq) of the entry
    whose queries are pairs -- its workspace function takes the line's nq as well and its per_label outputs have an entry per
    query.  Returns {name: device tensor}, with host=True {name: numpy array}."""
    rows, no, row_off, lab_off, T32, L32, n, labels, d_labels, nlabels = _line_arguments(probs, row_off, T, labels, lab_off, L)
    dev = probs.device
    lib = _native.lib
    queries, q_lines, nout = [], [], nlabels
    if pairs is not None:
        q_lines = [_host_ints(pairs[2], np.int64, "q_off"), _host_ints(pairs[3], np.int32, "nq")]
        if not len(q_lines[0]) == len(q_lines[1]) == n:
            raise ValueError("q_off and nq need one entry per line")
        queries = [_query_ints(pairs[0], "q_char"), _query_ints(pairs[1], "q_frame")]
        nout = queries[0][2]
        if queries[1][2] != nout:
            raise ValueError("q_char and q_frame need one entry per query: %d and %d" % (nout, queries[1][2]))
    elif t_query is not _NO_QUERY:
        queries = [_query_ints(t_query, "t_query")]
        if queries[0][2] != nlabels:
            raise ValueError("t_query needs an entry per label: %d for %d" % (queries[0][2], nlabels))
    ws = np.asarray([getattr(lib, ws_bytes_of)(*map(int, sizes)) for sizes in zip(T32, L32, *q_lines[1:])], dtype=np.int64)
    if (ws < 0).any():
        b = int(np.nonzero(ws < 0)[0][0])
        if pairs is not None:
            raise ValueError("line %d: a text of %d characters, %d timesteps and %d queries is outside what %s takes "
                             "(1 <= L <= %d, 2 L + 1 <= T <= %d, at most 2 L queries)"
                             % (b, int(L32[b]), int(T32[b]), int(q_lines[1][b]), takes, MAX_TARGET, MAX_T))
        raise ValueError("line %d: a text of %d characters and %d timesteps is outside what %s takes "
                         "(1 <= L <= %d, 2 L + 1 <= T <= %d)" % (b, int(L32[b]), int(T32[b]), takes, MAX_TARGET, MAX_T))
    outside = n and ((row_off + T32 > rows).any() or (lab_off + L32 > nlabels).any())
    if pairs is not None and n and (outside or (q_lines[0] + q_lines[1] > nout).any()):
        raise ValueError("a line's rows, labels or queries lie outside probs / labels / q_char")
    if outside:
        raise ValueError("a line's rows or labels lie outside probs / labels")
    ws_off, ws_bytes = _pieces(ws)
    with torch.cuda.device(dev):
        outs = [(name, torch.empty((max(nout, 1),) + shape, dtype=dt, device=dev), nout) for name, dt, shape in per_label]
        outs += [(name, torch.empty(max(n, 1), dtype=dt, device=dev), n) for name, dt in tuple(per_line) + (("status", torch.int32),)]
        if n:
            d, opt = _upload([row_off, T32, lab_off, L32, ws_off] + q_lines, [(d_labels, labels)] + [q[:2] for q in queries], dev)
            args = [probs.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), opt[0].data_ptr()]
            args += [t.data_ptr() for t in d[2:5] + opt[1:] + d[5:]] + [n, no, rows, nlabels] + ([] if pairs is None else [nout])
            args += [a.ctypes.data for a in [T32, L32] + q_lines[1:]] + ([] if omit_q is None else [omit_q])
            _launch(entry, args, outs, ws_bytes, dev, _fill)
        got = {name: o[:size] for name, o, size in outs}
    return {name: t.cpu().numpy() for name, t in got.items()} if host else got


def forced_alignment(probs, row_off, T, labels, lab_off, L, host=False, _fill=None, omit_q=None):
    """The device-level call, on torch's current stream; nothing is waited for.

    probs: contiguous float32 device tensor (rows, no), what the recogniser's output layer wrote; line b owns the rows
    row_off[b] .. + T[b] and the labels labels[lab_off[b] .. + L[b]] (class codes 1 .. no - 1).  row_off, T, lab_off, L:
    host integers per line; labels: host integers or an int32 device tensor.  Returns (frames (labels, 3) int32 =
    t_first, t_last, t_peak per label, score (lines,) int64, status (lines,) int32) as device tensors, or with host=True
    a dict of numpy arrays.  ValueError for sizes that do not fit each other or the kernel (L < 1, 2 L + 1 > T,
    L > 1023, T > 5000, classes outside 2 .. 128).  (_fill: a byte value every output and the workspace are filled with
    before the launch -- for tests.)
    omit_q: None, or the price (0 .. OMIT_MAX, the units of omit_units) at which the path may leave a character of the
    text out -- `ta_forced_align_omit` (csrc/ta_forced_omit.hip; DESIGN.md section 14.9, checker
    tests/forced_omit_ref.py) with its own workspace; such a character's three fields are OMITTED."""
    omit_q = None if omit_q is None else _omit_price(omit_q)
    omit = "" if omit_q is None else "_omit"
    got = _line_list_call("ta_forced_align" + omit, "ta_forced%s_workspace_bytes" % omit, "ta_forced_align", probs, row_off, T,
                          labels, lab_off, L, _fill, [("frames", torch.int32, (FIELDS,))], [("score", torch.int64)],
                          omit_q=omit_q, host=host)
    return got if host else (got["frames"], got["score"], got["status"])


def confidence_bits(c):
    """confidences in the integer units of the emission score (2^-16 bit) as float bits: c / 65536"""
    return np.asarray(c, dtype=np.float64) / 65536.0


def forced_confidence(probs, row_off, T, labels, lab_off, L, t_query, host=False, _fill=None):
    """Per-character confidence from max-marginals (csrc/ta_forced_conf.hip: `ta_forced_confidence`; DESIGN.md section
    14.10, checker tests/forced_conf_ref.py): the device-level call, on torch's current stream; nothing is waited for.

    probs, row_off, T, labels, lab_off, L: as forced_alignment takes them.  t_query: host integers or an int32 device
    tensor with an entry per label, entry lab_off[b] + i the frame queried for character i of line b (0 .. T[b] - 1, never
    decreasing along a line).  Returns (confidence (labels,) int64 in units of 2^-16 bit -- confidence_bits -- the total of
    the best path that spends the frame in the character's state minus that of the best path that spends it in any other
    state, rival (labels,) int32 that other state, status (lines,) int32: 0 ok, CONF_QUERY for a line whose queries the
    kernel refused) as device tensors, or with host=True a dict of numpy arrays.  ValueErrors as forced_alignment, and
    for a t_query without an entry per label.  (_fill: as forced_alignment's.)"""
    got = _line_list_call("ta_forced_confidence", "ta_forced_confidence_workspace_bytes", "ta_forced_confidence", probs,
                          row_off, T, labels, lab_off, L, _fill, [("confidence", torch.int64, ()), ("rival", torch.int32, ())],
                          [], t_query=t_query, host=host)
    return got if host else (got["confidence"], got["rival"], got["status"])


def omit_queries(frames, T):
    """The queries of ONE line aligned with `omit`, the host's rule of DESIGN.md section 14.18 (checker
    tests/forced_omit_conf_ref.py): frames (L, 3) as forced_alignment(omit_q=...) wrote them, T the line's timesteps.  A
    present character i asks (i, t_peak[i]); an omitted one asks (i, t_land - 1) and (i, t_land), t_land the t_first of the
    next present character or T - 1 if none follows, a frame below 0 dropped.  Returns (q_char, q_frame) int32, sorted by
    (frame, character): between 1 and 2 queries per character, what forced_omit_confidence takes for the line."""
    frames = np.asarray(frames, dtype=np.int64).reshape(-1, FIELDS)
    L, T = len(frames), int(T)
    if L == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    present = frames[:, 0] >= 0
    ahead = np.where(present, frames[:, 0], T - 1)       # t_first never decreases along the present characters
    land = np.full(L, T - 1, dtype=np.int64)             # per character the smallest of `ahead` behind it
    land[:-1] = np.minimum.accumulate(ahead[::-1])[::-1][1:]
    idx = np.arange(L, dtype=np.int64)
    absent = ~present
    q_char = np.concatenate([idx[present], idx[absent], idx[absent]])
    q_frame = np.concatenate([frames[present, 2], land[absent] - 1, land[absent]])
    keep = q_frame >= 0
    q_char, q_frame = q_char[keep], q_frame[keep]
    order = np.lexsort((q_char, q_frame))
    return q_char[order].astype(np.int32), q_frame[order].astype(np.int32)


def omit_values(L, q_char, confidence, rival):
    """per character of ONE line its (value, rival state) from the answers to omit_queries' queries, an (L, 2) int64 array:
    a present character's one answer; an omitted character's largest confidence and the rival state of the first query
    that attains it (the queries are in frame order)"""
    out = np.zeros((int(L), 2), dtype=np.int64)
    seen = np.zeros(int(L), dtype=bool)
    for i, c, r in zip(np.asarray(q_char).tolist(), np.asarray(confidence).tolist(), np.asarray(rival).tolist()):
        if not seen[i] or c > out[i, 0]:
            out[i] = (c, r)
            seen[i] = True
    if not seen.all():
        raise ValueError("a character without a query")
    return out


def forced_omit_confidence(probs, row_off, T, labels, lab_off, L, q_char, q_frame, q_off, nq, omit_q, host=False, _fill=None):
    """Per-character confidence on the lattice with omission (csrc/ta_forced_omit_conf.hip: `ta_forced_omit_confidence`;
    DESIGN.md section 14.18, checker tests/forced_omit_conf_ref.py): the device-level call, on torch's current stream;
    nothing is waited for.

    probs, row_off, T, labels, lab_off, L: as forced_alignment takes them; omit_q: the price, as forced_alignment's.  A query
    is a (character, frame) pair: line b has nq[b] of them, 0 .. 2 L[b], at q_off[b] .. + nq[b] of q_char / q_frame (host
    integers or int32 device tensors of one length) -- a character 0 .. L[b] - 1 and a frame 0 .. T[b] - 1, the frames never
    decreasing along the line (omit_queries makes such a list).  q_off, nq: host integers per line.  Returns (confidence
    (queries,) int64 in units of 2^-16 bit -- the total of the best path that spends the frame in the character's state minus
    that of the best path that spends it in any other state -- rival (queries,) int32 that other state, status (lines,) int32:
    0 ok, CONF_QUERY for a line whose queries the kernel refused) as device tensors, or with host=True a dict of numpy
    arrays.  ValueErrors as forced_alignment, and for queries that do not fit their arrays.  (_fill: as forced_alignment's.)"""
    got = _line_list_call("ta_forced_omit_confidence", "ta_forced_omit_confidence_workspace_bytes", "ta_forced_omit_confidence",
                          probs, row_off, T, labels, lab_off, L, _fill, [("confidence", torch.int64, ()), ("rival", torch.int32, ())],
                          [], omit_q=_omit_price(omit_q), pairs=(q_char, q_frame, q_off, nq), host=host)
    return got if host else (got["confidence"], got["rival"], got["status"])


POSTERIOR_OUTPUTS =("own_m", "own_x", "rival_m", "rival_x", "rival_state", "z_m", "z_x", "status")
# Refining's one download, by name: the new columns, the harvest's slots (slot_L: their lengths) and the three statuses;
# with confidence=True ta_forced_confidence_lines' outputs (c_status: per slot), then ta_confidence_pages' (p_status: per
# page); with posterior=True ta_forced_posterior_lines' (s_status: per slot), then ta_posterior_pages' (pp_status: per page)
DOWNLOAD = ("ops_new", "ops_new_len", "idx_new", "idx_new_len", "refined", "frames", "acc_line", "slot_L", "lab_off", "count",
            "h_status", "f_status", "r_status")
CONFIDENCE_DOWNLOAD = ("conf", "rival", "c_status", "char_conf", "syl_conf", "p_status")
OMIT_DOWNLOAD = ("omitted",)     # with omit_q: ta_refine_columns_omit's count per chunk line
POSTERIOR_DOWNLOAD = ("own_m", "own_x", "rival_m", "rival_x", "rival_state", "z_m", "z_x", "s_status", "char_post", "syl_post",
                      "pp_status")


def forced_posterior(probs, row_off, T, labels, lab_off, L, t_query, host=False, _fill=None):
    """Sum-product posteriors and the text's likelihood per line (csrc/ta_forced_post.hip: `ta_forced_posterior`; DESIGN.md
    section 14.11, checker tests/forced_post_ref.py, whose words the kernel's equal bit for bit): the device-level call, on
    torch's current stream; nothing is waited for.

    The arguments are forced_confidence's.  Returns a dict of device tensors, or with host=True of numpy arrays, each value
    a pair of a float64 significand in [0.5, 1) and an int32 exponent (zero: 0.0, 0): per label own_m / own_x -- the mass of
    all paths that spend the queried frame in the character's state -- rival_m / rival_x -- the largest such mass over the
    other states -- and rival_state int32, the smallest state that has it; per line z_m / z_x, the mass of all paths, and
    status (0 ok, CONF_QUERY for a line whose queries the kernel refused).  posterior_values and loglik_bits turn them
    into probabilities and bits on the host.  ValueErrors as forced_confidence."""
    f64, i32 = torch.float64, torch.int32
    return _line_list_call("ta_forced_posterior", "ta_forced_posterior_workspace_bytes", "ta_forced_posterior", probs, row_off,
                           T, labels, lab_off, L, _fill, [("own_m", f64, ()), ("own_x", i32, ()), ("rival_m", f64, ()),
                                                         ("rival_x", i32, ()), ("rival_state", i32, ())],
                           [("z_m", f64), ("z_x", i32)], t_query=t_query, host=host)


def posterior_values(m, x, z_m, z_x):
    """the posterior of a state's mass (m, x) under its line's (z_m, z_x) -- an entry per value, or one for all:
    ldexp(m / z_m, x - z_x), float64.  Host arithmetic in numpy; the pairs are what is compared with the checker."""
    return np.ldexp(np.asarray(m, dtype=np.float64) / np.asarray(z_m, dtype=np.float64),
                    np.asarray(x, dtype=np.int64) - np.asarray(z_x, dtype=np.int64))


def loglik_bits(z_m, z_x):
    """log2 P(text | line) of a line's (z_m, z_x): log2(z_m) + z_x, float64"""
    return np.log2(np.asarray(z_m, dtype=np.float64)) + np.asarray(z_x, dtype=np.float64)


class LinePosterior(object):
    """one line's posteriors at its own t_peak (align_lines(posterior=True)): posterior (L,)
    float64, the probability under the recogniser's outputs and the known text that character i holds its peak frame, all
    paths summed; rival_posterior (L,) float64, the largest posterior of any other state at that frame, and rival_state
    (L,) int32, that state (even: the blank 2 j, odd: character (s - 1) / 2); loglik_bits, log2 P(text | line)"""
    __slots__ = ("posterior", "rival_posterior", "rival_state", "loglik_bits")

    def __init__(self, got, a, b, line):
        """from forced_posterior's host dict: labels a .. b, line `line`"""
        z_m, z_x = got["z_m"][line], got["z_x"][line]
        self.posterior = posterior_values(got["own_m"][a:b], got["own_x"][a:b], z_m, z_x)
        self.rival_posterior = posterior_values(got["rival_m"][a:b], got["rival_x"][a:b], z_m, z_x)
        self.rival_state = got["rival_state"][a:b].copy()
        self.loglik_bits = float(loglik_bits(z_m, z_x))


# ---- page scope (the rule of record is tests/forced_page_ref.py) --------------------------------

def page_windows(table_rows, n, margin=DEFAULT_MARGIN):
    """the window of transcript characters [lo, hi) of every line of ONE page from its harvest rows (fields 0 - 2:
    reason, t_first, L) and the page's n transcript characters: (lo, hi) int32, or None if a window is wider than
    MAX_TARGET.  A line without EMPTY / PAGE has the core [t_first, t_first + L), any other the empty range at the
    previous line's core end (0 for a leading line); the core grows by `margin` on both sides inside 0 .. n, the first
    window starts at 0, the last ends at n, and a forward pass makes the windows move forwards without a gap:
    lo_k = max(lo_k, lo_{k-1}), hi_k = max(hi_k, hi_{k-1}), lo_k = min(lo_k, hi_{k-1})."""
    from . import harvest
    rows = np.asarray(table_rows, dtype=np.int64)
    rows = rows.reshape(len(rows), -1)
    nl = len(rows)
    if margin < 0 or nl < 1:
        raise ValueError("page_windows needs margin >= 0 and at least one line")
    text = (rows[:, 0] & (harvest.EMPTY | harvest.PAGE)) == 0
    end = np.where(text, rows[:, 1] + rows[:, 2], 0)
    last = np.maximum.accumulate(np.where(text, np.arange(nl), -1))          # the latest line with a core, itself included
    end = np.where(last >= 0, end[np.maximum(last, 0)], 0)
    start = np.where(text, rows[:, 1], end)
    lo, hi = np.maximum(start - margin, 0), np.minimum(end + margin, n)
    lo[0], hi[-1] = 0, n
    hi = np.maximum.accumulate(hi)
    for k in range(1, nl):
        lo[k] = min(max(lo[k], lo[k - 1]), hi[k - 1])
    if (hi - lo > MAX_TARGET).any():
        return None
    return lo.astype(np.int32), hi.astype(np.int32)


def _page_list_arguments(probs, row_off, T, line_first, lo, hi, labels, lab_off):
    """the first checks of _page_list_call: (rows, no, row_off, lab_off, line_first, T32,
    lo32, hi32, labels, npages, nlines, nlabels, the windows' widths)"""
    if not (isinstance(probs, torch.Tensor) and probs.is_cuda and probs.dtype == torch.float32 and probs.dim() == 2 and
            probs.is_contiguous()):
        raise ValueError("probs must be a contiguous float32 device tensor (rows, classes)")
    rows, no = int(probs.shape[0]), int(probs.shape[1])
    if not 2 <= no <= 128:
        raise ValueError("2 .. 128 classes")
    row_off, lab_off = _host_ints(row_off, np.int64, "row_off"), _host_ints(lab_off, np.int64, "lab_off")
    line_first = _host_ints(line_first, np.int64, "line_first")
    T32, lo32, hi32 = _host_ints(T, np.int32, "T"), _host_ints(lo, np.int32, "lo"), _host_ints(hi, np.int32, "hi")
    labels = _host_ints(labels, np.int32, "labels")
    npages, nlines, nlabels = len(line_first) - 1, len(T32), len(labels)
    if npages < 0 or len(lab_off) != npages + 1 or not (len(row_off) == len(lo32) == len(hi32) == nlines):
        raise ValueError("line_first and lab_off need one entry per page and one more; row_off, T, lo and hi one per line")
    width = hi32.astype(np.int64) - lo32
    if npages:
        if line_first[0] != 0 or line_first[-1] != nlines or (np.diff(line_first) < 1).any():
            raise ValueError("line_first must run from 0 to the number of lines and give every page a line")
        if lab_off[-1] > nlabels or (np.diff(lab_off) < 1).any():
            raise ValueError("lab_off must stay inside labels and give every page a character")
        if (row_off + T32 > rows).any():
            raise ValueError("a line's rows lie outside probs")
        if (width < 0).any() or (width > MAX_TARGET).any():
            raise ValueError("a window must hold 0 .. %d characters" % MAX_TARGET)
        if (T32 < 1).any() or (T32 > MAX_T).any():
            raise ValueError("a line needs 1 .. %d timesteps" % MAX_T)
    return rows, no, row_off, lab_off, line_first, T32, lo32, hi32, labels, npages, nlines, nlabels, width


def _page_list_call(entry, ws_bytes_of, probs, row_off, T, line_first, lo, hi, labels, lab_off, _fill, per_label, per_page, host,
                    caps=None, query=_NO_QUERY, omit_q=None):
    """what forced_page_alignment, forced_page_confidence and forced_page_posterior share: the checks, the optional `query`
    array with a row of PAGE_FIELDS per label, the per-page caps = (characters or None, frames, the refusal's text), the
    workspace pieces -- without a query a piece per line, formed here and held against the library function `ws_bytes_of`;
    with one a piece per page, which that function sizes -- the packed upload, the outputs (per_label: [(name, torch dtype,
    trailing shape)], per_page: [(name, torch dtype)], then status per page) and the call of the library function named
    `entry`.  omit_q: the price ta_forced_align_pages_omit takes.  Returns {name: device tensor}, with host=True {name:
    numpy array}."""
    (rows, no, row_off, lab_off, line_first, T32, lo32, hi32, labels, npages, nlines, nlabels,
     width) = _page_list_arguments(probs, row_off, T, line_first, lo, hi, labels, lab_off)
    queries = []
    if query is not _NO_QUERY:
        queries = [_query_ints(query, "query")]
        if queries[0][2] != PAGE_FIELDS * nlabels:
            raise ValueError("query needs a row of %d per label: %d words for %d labels" % (PAGE_FIELDS, queries[0][2], nlabels))
    dev = probs.device
    lib = _native.lib
    with torch.cuda.device(dev):
        outs = [(name, torch.empty((max(nlabels, 1),) + shape, dtype=dt, device=dev), nlabels) for name, dt, shape in per_label]
        outs += [(name, torch.empty(max(npages, 1), dtype=dt, device=dev), npages)
                 for name, dt in tuple(per_page) + (("status", torch.int32),)]
        if npages:
            t64 = T32.astype(np.int64)
            if caps is not None and ((caps[0] is not None and (np.diff(lab_off) > caps[0]).any()) or
                                     (np.add.reduceat(t64, line_first[:-1]) > caps[1]).any()):
                raise ValueError(caps[2])
            K = np.asarray([lib.ta_forced_page_variant(int(w)) for w in np.maximum.reduceat(width, line_first[:-1])],
                           dtype=np.int64)         # (every page has a line)
            if queries:
                ws = np.asarray([getattr(lib, ws_bytes_of)(int(n), int(k)) for n, k in zip(np.diff(lab_off), K)], dtype=np.int64)
                if (ws < 0).any():
                    raise ValueError("a page's text is too long")
            else:
                Kq = np.repeat(K, np.diff(line_first))
                ws = 256 * np.where(Kq == 32, 2 * t64, -(-t64 // np.maximum(16 // Kq, 1)))
                if omit_q is not None:
                    ws = ws + 256 * -(-t64 // (32 // Kq))    # the bit rows behind a line's move rows
                for p in range(npages):
                    a, b = int(line_first[p]), int(line_first[p + 1])
                    if int(ws[a:b].sum()) != getattr(lib, ws_bytes_of)(b - a, T32[a:b].ctypes.data, int(K[p])):
                        raise RuntimeError("the workspace pieces disagree with %s" % ws_bytes_of)
            ws_off, ws_bytes = _pieces(ws)
            d, opt = _upload([row_off, T32, line_first, lo32, hi32, labels, lab_off, ws_off], [q[:2] for q in queries], dev)
            args = [probs.data_ptr()] + [t.data_ptr() for t in d + opt] + [npages, nlines, no, rows, nlabels]
            args += [a.ctypes.data for a in (T32, line_first, lo32, hi32, lab_off)] + ([] if omit_q is None else [omit_q])
            _launch(entry, args, outs, ws_bytes, dev, _fill)
        got = {name: o[:size] for name, o, size in outs}
    return {name: t.cpu().numpy() for name, t in got.items()} if host else got


def forced_page_alignment(probs, row_off, T, line_first, lo, hi, labels, lab_off, host=False, _fill=None, omit_q=None):
    """The device-level call of page scope, on torch's current stream; nothing is waited for, one packed upload.

    probs: contiguous float32 device tensor (rows, no).  Page p owns the lines line_first[p] .. line_first[p + 1] (in
    reading order) and the labels labels[lab_off[p] .. lab_off[p + 1]) (class codes 1 .. no - 1); line q owns the rows
    row_off[q] .. + T[q] and the window of characters lo[q] .. hi[q] of its page's text.  All but probs: host integers.
    Returns (frames (labels, 4) int32 = line in the page, t_first, t_last, t_peak per label, score (pages,) int64,
    status (pages,) int32: 0 ok, 3 no path) as device tensors, or with host=True a dict of numpy arrays.  ValueError for
    what ta_forced_align_pages refuses: windows that do not start at 0, end at n and move forwards without a gap, a
    window wider than 1023, a page without lines or text, T outside 1 .. 5000.  (_fill: as forced_alignment's.)
    omit_q: None, or the price (0 .. OMIT_MAX, the units of omit_units) at which the path may leave a character of the
    text out -- `ta_forced_align_pages_omit` (csrc/ta_forced_page_omit.hip; DESIGN.md section 14.12, checker
    tests/forced_page_omit_ref.py) with its own workspace; such a character's four fields are OMITTED, every page has a
    path, and a page of more than 2^20 characters or 2^25 frames is a ValueError."""
    omit_q = None if omit_q is None else _omit_price(omit_q)
    omit = "" if omit_q is None else "_omit"
    got = _page_list_call("ta_forced_align_pages" + omit, "ta_forced_page%s_workspace_bytes" % omit, probs, row_off, T, line_first,
                          lo, hi, labels, lab_off, _fill, [("frames", torch.int32, (PAGE_FIELDS,))], [("score", torch.int64)], host,
                          caps=None if omit_q is None else (PAGE_MAX_CHARS, PAGE_MAX_FRAMES,
                                                            "a page with omission holds at most 2^20 characters and 2^25 frames"),
                          omit_q=omit_q)
    return got if host else (got["frames"], got["score"], got["status"])


def forced_page_confidence(probs, row_off, T, line_first, lo, hi, labels, lab_off, query, host=False, _fill=None):
    """Per-character confidence at page scope from max-marginals (csrc/ta_forced_page_conf.hip:
    `ta_forced_page_confidence`; DESIGN.md section 14.13, checker tests/forced_page_conf_ref.py): the device-level call, on
    torch's current stream; nothing is waited for, one packed upload.

    probs, row_off, T, line_first, lo, hi, labels, lab_off: as forced_page_alignment takes them.  query: (labels, 4)
    integers on the host or a contiguous int32 device tensor of that shape, row lab_off[p] + i = the query of character i
    of page p: field 0 the line (in the page), field 3 the frame (local to that line); fields 1 and 2 are not read, so the
    frames forced_page_alignment returned can be handed over as they are.  The character must lie in its query line's
    window, and the queries must not decrease in (line, frame) order along a page.  Returns (confidence (labels,) int64 in
    units of 2^-16 bit -- confidence_bits -- the total of the best path of the page that spends the frame in the
    character's state minus that of the best path that spends it in any other live state, rival (labels,) int32 that
    other PAGE state, status (pages,) int32: 0 ok, NOPATH, CONF_QUERY for a page whose queries the kernel refused) as
    device tensors, or with host=True a dict of numpy arrays.  ValueErrors as forced_page_alignment, for a page of more
    than 2^25 frames and for a query without a row per label.  (_fill: as forced_alignment's.)"""
    got = _page_list_call("ta_forced_page_confidence", "ta_forced_page_confidence_workspace_bytes", probs, row_off, T, line_first,
                          lo, hi, labels, lab_off, _fill, [("confidence", torch.int64, ()), ("rival", torch.int32, ())], [], host,
                          caps=(None, PAGE_MAX_FRAMES, "a page's confidence takes at most 2^25 frames"), query=query)
    return got if host else (got["confidence"], got["rival"], got["status"])


PAGE_POST_MAX_FRAMES = 1 << 24                  # what ta_forced_page_posterior takes per page
PAGE_POST_PER_LABEL = (("own_m", torch.float64), ("own_x", torch.int32), ("rival_m", torch.float64), ("rival_x", torch.int32),
                       ("rival_state", torch.int32))
PAGE_POST_PER_PAGE = (("z_m", torch.float64), ("z_x", torch.int32), ("status", torch.int32))


def forced_page_posterior(probs, row_off, T, line_first, lo, hi, labels, lab_off, query, host=False, _fill=None):
    """Sum-product posteriors at page scope and the page's likelihood (csrc/ta_forced_page_post.hip:
    `ta_forced_page_posterior`; DESIGN.md section 14.15, checker tests/forced_page_post_ref.py, whose words the kernel's
    equal bit for bit): the device-level call, on torch's current stream; nothing is waited for, one packed upload.

    The arguments are forced_page_confidence's: `query` (labels, 4) on the host or the contiguous int32 device tensor
    forced_page_alignment returned, field 0 the line and field 3 the frame.  Returns a dict of device tensors, or with
    host=True of numpy arrays, each value a pair of a float64 significand in [0.5, 1) and an int32 exponent (zero: 0.0, 0):
    per label own_m / own_x -- the mass of all legal paths of the page that spend the queried frame in the character's
    state -- rival_m / rival_x -- the largest such mass over the other live states of the query line's window -- and
    rival_state int32, the smallest PAGE state that has it; per page z_m / z_x, the mass of all legal paths, and status
    (0 ok, NOPATH -- z_m and z_x are left alone then --, CONF_QUERY for a page whose queries the kernel refused).
    posterior_values and loglik_bits turn them into probabilities and log2 P(text | page) on the host.  ValueErrors as
    forced_page_confidence, here for a page of more than 2^24 frames.  (_fill: as forced_alignment's.)"""
    return _page_list_call("ta_forced_page_posterior", "ta_forced_page_posterior_workspace_bytes", probs, row_off, T, line_first,
                           lo, hi, labels, lab_off, _fill, [(name, dt, ()) for name, dt in PAGE_POST_PER_LABEL],
                           PAGE_POST_PER_PAGE[:-1], host,
                           caps=(None, PAGE_POST_MAX_FRAMES, "a page's posteriors take at most 2^24 frames"), query=query)


def page_columns(frames, T, raw_w, x_min, y_min, y_max, pad, box_base):
    """a page refined at page scope: (ops, idx, boxes) -- n pair columns, the box row of each (box_base + i) and the n new
    boxes.  frames: (n, 4) line, t_first, t_last, t_peak of the page's characters; T, raw_w, x_min, y_min, y_max: per line
    of the page.  The characters the path put on a line, in order, get the boxes peak_boxes yields for one refined line.
    A character the path omitted (page_omit: a row of OMITTED) is a transcript character alone (op 1) in its place, as
    refine_columns(present=) makes one at line scope: no box row, and the box rows box_base .. go to the present ones in
    order.  Frames without such rows give exactly the columns above."""
    frames = np.asarray(frames, dtype=np.int64).reshape(-1, PAGE_FIELDS)
    here = frames[:, 0] != OMITTED
    n, shown = len(frames), frames[here]
    if (shown[:, 0] < 0).any():
        raise ValueError("the characters' lines must not decrease and must lie on the page")
    on = np.bincount(shown[:, 0], minlength=len(T)).astype(np.int64)
    if len(on) != len(T) or (np.diff(shown[:, 0]) < 0).any():
        raise ValueError("the characters' lines must not decrease and must lie on the page")
    used = np.flatnonzero(on)
    pick = lambda a: np.asarray(a, dtype=np.int64)[used]                                            # noqa: E731
    boxes = peak_boxes(shown[:, 3], on[used], pick(T), pick(raw_w), pick(x_min), pick(y_min), pick(y_max), pad)
    return (np.where(here, 0, 1).astype(np.uint8), np.arange(box_base, box_base + len(shown), dtype=np.int64),
            np.asarray(boxes, dtype=np.int64).reshape(-1, 4))


def align_page_lines(model_or_recogniser, lines, text, windows=None, want_run=False, omit=None, confidence=False,
                     posterior=False):
    """The line images of ONE page in reading order (as align_lines takes lines) against the page's text: one best path
    through all of them.  windows: (lo, hi) per line, by default the whole text on every line (refused if it has more
    than 1023 characters).  Returns (per line [(char, t_first, t_last, t_peak, x)] for the characters the path put on it,
    score); ValueError for a character outside the codec, an empty text, windows ta_forced_align_pages refuses, and a text
    that has no path through the lines (more characters than frames, for one).  want_run: also {"probs", "row_off", "T",
    "frames"}.
    omit: None, or the price in bits (omit_units) of a character the path may leave out.  Every
    text then has a path, more characters than frames or not; the per-line lists hold the characters that are present,
    and ONE MORE element is returned behind the others: the indices into `text` of the omitted characters -- an omitted
    character has no line, so it cannot sit in a line's list.
    confidence: return one more value behind the others -- an (n, 2) int64 array of (confidence, rival PAGE state) per
    character of `text` at its own line and t_peak (forced_page_confidence).  ValueError together
    with omit: the confidence is defined on the strict lattice only.
    posterior: return one more value behind those -- a LinePosterior of the PAGE (forced_page_posterior; DESIGN.md section
    14.15): per character of `text` at its own line and t_peak the posterior, all legal paths of the page summed, the
    largest posterior of any other live state and that PAGE state, and loglik_bits = log2 P(text | page).  ValueError
    together with omit."""
    if confidence and omit is not None:
        raise ValueError("confidence is defined on the strict lattice only: not together with omit")
    if posterior and omit is not None:
        raise ValueError("posterior is defined on the strict lattice only: not together with omit")
    omit_q = None if omit is None else omit_units(omit)
    from . import ocr, train
    rec = _recognizer(model_or_recogniser)
    lines = list(lines)
    labels = np.asarray(train.encode_text(rec.model.codec, text), dtype=np.int32)
    n, nl = len(labels), len(lines)
    if n < 1 or nl < 1:
        raise ValueError("align_page_lines needs at least one line and one character")
    if windows is None:
        if n > MAX_TARGET:
            raise ValueError("a text of %d characters needs windows: at most %d fit one" % (n, MAX_TARGET))
        lo, hi = np.zeros(nl, np.int32), np.full(nl, n, np.int32)
    else:
        lo, hi = (np.ascontiguousarray(w, dtype=np.int32) for w in windows)
    with torch.cuda.device(rec.device):
        st = rec.prepare(lines)
        T = np.asarray(st["T_host"], dtype=np.int64)[:nl]
        rec.run(st, want_probs=True, decode=False)
        row_off = np.asarray(st["row_start_host"][:nl], dtype=np.int64)
        got = forced_page_alignment(st["probs"], row_off, T, [0, nl], lo, hi, labels, [0, n], host=True, omit_q=omit_q)
        conf = None
        if confidence and got["status"][0] == OK:
            conf = forced_page_confidence(st["probs"], row_off, T, [0, nl], lo, hi, labels, [0, n], got["frames"], host=True)
        post = None
        if posterior and got["status"][0] == OK:
            post = forced_page_posterior(st["probs"], row_off, T, [0, nl], lo, hi, labels, [0, n], got["frames"], host=True)
    if got["status"][0] == NOPATH:
        raise ValueError("the text has no path through the lines' windows")
    if got["status"][0] != OK:
        raise RuntimeError("ta_forced_align_pages refused the page on the device: %s" % PAGE_STATUS.get(int(got["status"][0]), "?"))
    if conf is not None and conf["status"][0] != OK:
        raise RuntimeError("ta_forced_page_confidence refused the page on the device: %s"
                           % PAGE_CONF_STATUS.get(int(conf["status"][0]), "?"))
    if post is not None and post["status"][0] != OK:
        raise RuntimeError("ta_forced_page_posterior refused the page on the device: %s"
                           % PAGE_CONF_STATUS.get(int(post["status"][0]), "?"))
    widths = [int(ln.shape[1]) if ocr._is_raw_strip(ln) else None for ln in lines]
    out = [[] for _ in range(nl)]
    omitted = [i for i, f in enumerate(got["frames"]) if f[0] == OMITTED]
    for ch, f in zip(text, got["frames"]):
        k = int(f[0])
        if k == OMITTED:
            continue
        raw_w = float(widths[k]) if widths[k] is not None else float(T[k] - 2 * ocr.PAD)
        out[k].append((ch, int(f[1]), int(f[2]), int(f[3]), (int(f[3]) - ocr.PAD) * (raw_w / (T[k] - 2 * ocr.PAD))))
    ret = (out, int(got["score"][0]))
    if want_run:
        ret += ({"probs": st["probs"], "row_off": row_off, "T": T, "frames": got["frames"]},)
    if confidence:
        ret += (np.stack([conf["confidence"], conf["rival"].astype(np.int64)], axis=1),)
    if posterior:
        ret += (LinePosterior(post, 0, n, 0),)
    return ret if omit is None else ret + (omitted,)


def _recognizer(model_or_recogniser):
    from . import alignToOCR as atocr
    return atocr._recognizer_for(model_or_recogniser)


def align_lines(model_or_recogniser, lines, texts, want_run=False, omit=None, confidence=False, posterior=False,
                omit_confidence=False):
    """Recognise the lines (prepared (T, 48) rows or raw uint8 strips, as LineRecognizer.prepare takes them), keep the
    probabilities and align each with its text.  Returns per line ([(char, t_first, t_last, t_peak, x)], score): x is the
    .llocs position of t_peak, (t_peak - pad) raw_width / (T - 2 pad) in raw strip pixels.  ValueError for a character
    outside the model's codec or a text whose 2 L + 1 states exceed its line's timesteps.  want_run: also return what the
    alignment ran on, {"probs" (the device tensor), "row_off", "T"} -- for checking it.
    omit: None, or the price in bits (omit_units) of a character the path may leave out; the entry of such a character
    is (char, -1, -1, -1, None).
    confidence: return one more value behind the others -- per line an (L, 2) int64 array of (confidence, rival state) at
    the line's own t_peak (forced_confidence).  ValueError together with omit: the confidence is
    defined on the strict lattice only.
    posterior: return one more value behind the others (behind confidence's) -- per line a LinePosterior at the line's own
    t_peak (forced_posterior).  ValueError together with omit, as confidence.
    omit_confidence: with omit, return one more value behind the others -- per line an (L, 2) int64 array of (value, rival
    state) on the lattice with omission (omit_queries, forced_omit_confidence, omit_values): a
    present character's confidence at its own t_peak, >= 0; an omitted character's largest confidence over the two frames
    around the place the path jumped it at, <= 0 -- minus it bounds from ABOVE what the best path would lose if the
    character had to appear.  ValueError without omit."""
    from . import ocr, train
    for on, what in ((confidence, "confidence is"), (posterior, "posteriors are")):
        if on and omit is not None:
            raise ValueError("%s defined on the strict lattice only: not together with omit" % what)
    if omit_confidence and omit is None:
        raise ValueError("omit_confidence is the confidence on the lattice with omission: it needs omit")
    omit_q = None if omit is None else omit_units(omit)
    rec = _recognizer(model_or_recogniser)
    lines, texts = list(lines), list(texts)
    if len(lines) != len(texts):
        raise ValueError("%d lines but %d texts" % (len(lines), len(texts)))
    codec = rec.model.codec
    labels = [train.encode_text(codec, tx) for tx in texts]
    if not lines:
        empty = (([],) + ((None,) if want_run else ()) + (([],) if confidence else ()) + (([],) if posterior else ()) +
                 (([],) if omit_confidence else ()))
        return empty if len(empty) > 1 else []
    more = {}                                            # per switch that is on and ran: its call's host dict
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
        got = forced_alignment(st["probs"], st["row_start_host"][:len(lines)], T, np.concatenate(labels), lab_off, L, host=True,
                               omit_q=omit_q)
        for on, entry, call in ((confidence, "ta_forced_confidence", forced_confidence),
                                (posterior, "ta_forced_posterior", forced_posterior)):
            if on and not got["status"].any():
                more[entry] = call(st["probs"], st["row_start_host"][:len(lines)], T, np.concatenate(labels), lab_off, L,
                                   got["frames"][:, 2], host=True)
        if omit_confidence and not got["status"].any():
            qs = [omit_queries(got["frames"][lab_off[b]:lab_off[b] + L[b]], T[b]) for b in range(len(lines))]
            nq = np.asarray([len(qc) for qc, _ in qs], dtype=np.int64)
            q_off = np.concatenate([[0], np.cumsum(nq)[:-1]])
            more["ta_forced_omit_confidence"] = forced_omit_confidence(
                st["probs"], st["row_start_host"][:len(lines)], T, np.concatenate(labels), lab_off, L,
                np.concatenate([qc for qc, _ in qs]), np.concatenate([qf for _, qf in qs]), q_off, nq, omit_q, host=True)
    for entry, status in [("ta_forced_align", got["status"])] + [(entry, m["status"]) for entry, m in more.items()]:
        bad = np.nonzero(status)[0]
        if bad.size:
            raise RuntimeError("%s refused line %d on the device: %s" % (entry, int(bad[0]), STATUS.get(int(status[bad[0]]), "?")))
    widths = [int(ln.shape[1]) if ocr._is_raw_strip(ln) else None for ln in lines]     # a raw strip's own width
    out = []
    for b in range(len(lines)):
        fr = got["frames"][lab_off[b]:lab_off[b] + L[b]]
        raw_w = float(widths[b]) if widths[b] is not None else float(T[b] - 2 * ocr.PAD)
        scale = raw_w / (T[b] - 2 * ocr.PAD)
        out.append(([(ch, int(f[0]), int(f[1]), int(f[2]), (int(f[2]) - ocr.PAD) * scale if f[2] != OMITTED else None)
                     for ch, f in zip(texts[b], fr)], int(got["score"][b])))
    ret = (out,)
    if want_run:
        ret += ({"probs": st["probs"], "row_off": np.asarray(st["row_start_host"][:len(lines)]), "T": T},)
    if confidence:
        conf = more["ta_forced_confidence"]
        both = np.stack([conf["confidence"], conf["rival"].astype(np.int64)], axis=1)
        ret += ([both[lab_off[b]:lab_off[b] + L[b]] for b in range(len(lines))],)
    if posterior:
        post = more["ta_forced_posterior"]
        ret += ([LinePosterior(post, int(lab_off[b]), int(lab_off[b] + L[b]), b) for b in range(len(lines))],)
    if omit_confidence:
        oc = more["ta_forced_omit_confidence"]
        ret += ([omit_values(L[b], qs[b][0], oc["confidence"][q_off[b]:q_off[b] + nq[b]], oc["rival"][q_off[b]:q_off[b] + nq[b]])
                 for b in range(len(lines))],)
    return ret if len(ret) > 1 else out


# ---- boxes under refinement (the per-character rule of record is tests/forced_ref.py) --------

def refine_columns(ops, idx, o_line, lines, present=None):
    """One page's alignment columns with every refined line's run replaced.  ops: the columns (0 pair, 1 transcript
    character alone, 2 OCR character alone); idx: per OCR character of the columns its row of the box array; o_line: per
    OCR character its text line; lines: [(line, t_first, L, first new box row)] of the page's refined lines, ascending.
    A refined line owns the columns from its first to its last OCR-carrying column: they become op-1 columns for the
    transcript characters in front of the kept range t_first .. + L, L pair columns with the new box rows, and op-1
    columns for the rest.  Returns (ops, idx).
    present: None, or per entry of `lines` a bool per kept character -- one the forced alignment omitted (False) becomes
    an op-1 column in its place, and the line's new box rows, from its first on, go to the present ones in order."""
    ops, idx, o_line = np.asarray(ops, dtype=np.uint8), np.asarray(idx, dtype=np.int64), np.asarray(o_line)
    if present is not None:
        present = [np.asarray(m, dtype=bool).reshape(-1) for m in present]
        if len(present) != len(lines) or any(len(m) != ln[2] for m, ln in zip(present, lines)):
            raise ValueError("present needs a bool per kept character of every refined line")
    if not lines:
        return ops, idx
    has_t = ops != 2
    col_of_o = np.flatnonzero(ops != 1)
    t_before = np.cumsum(has_t) - has_t                  # transcript characters in front of each column
    new_ops, new_idx, c_done, j_done = [], [], 0, 0
    for n, (line, t_first, L, row) in enumerate(lines):
        kept = np.zeros(L, np.uint8) if present is None else np.where(present[n], 0, 1).astype(np.uint8)
        js = np.flatnonzero(o_line == line)
        jlo, jhi = int(js[0]), int(js[-1])
        c0, c1 = int(col_of_o[jlo]), int(col_of_o[jhi])
        ta, tb = int(t_before[c0]), int(t_before[c1]) + int(has_t[c1])
        if not (jhi - jlo + 1 == len(js) and c0 >= c_done and ta <= t_first and t_first + L <= tb):
            raise ValueError("line %d: its kept characters are not inside the columns of its OCR characters" % line)
        new_ops += [ops[c_done:c0], np.ones(t_first - ta, np.uint8), kept, np.ones(tb - t_first - L, np.uint8)]
        new_idx += [idx[j_done:jlo], np.arange(row, row + int((kept == 0).sum()), dtype=np.int64)]
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

REFINE_STATUS = {_native.TA_REFINE_OK: "ok", _native.TA_REFINE_HARVEST: "the harvest refused the page",
                 _native.TA_REFINE_BOUNDS: "the page's own numbers are out of bounds",
                 _native.TA_REFINE_COLUMNS: "line indices decrease or leave the page, or the columns disagree with the page's sizes",
                 _native.TA_REFINE_CONTAIN: "a line's kept characters are not inside the columns of its OCR characters"}


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


def present_box_rows(frames, L, lab_off, T, raw_w, x_min, y_min, y_max, pad, done=None):
    """The new box rows of packed slots whose forced alignment may have omitted characters.
    frames: (rows, 3) as ta_forced_align_omit_lines wrote them; L, lab_off and the geometry (peak_boxes') per slot; done: a
    bool per slot, False for one that was not aligned (its frames are not looked at).  A character is present iff its
    first field is not negative.  Per slot the rows are peak_boxes over the PRESENT characters' peaks alone -- a present
    character's previous position is the previous present character's, refine_pages' construction -- scattered to
    lab_off[k] + i of the present i.  Returns (len(frames), 4) int64; every other row holds zeros and is never referenced."""
    frames = np.asarray(frames).reshape(-1, FIELDS)
    L, lab_off = np.asarray(L, dtype=np.int64), np.asarray(lab_off, dtype=np.int64)
    rows = np.zeros((len(frames), 4), np.int64)
    slot_of = np.repeat(np.arange(len(L)), L)
    pos = np.repeat(lab_off, L) + (np.arange(len(slot_of)) - np.repeat(np.cumsum(L) - L, L))
    here = frames[pos, 0] >= 0
    if done is not None:
        here &= np.asarray(done, dtype=bool)[slot_of]
    Lp = np.bincount(slot_of[here], minlength=len(L))
    has = Lp > 0
    if has.any():
        pick = lambda a: np.asarray(a, dtype=np.int64)[has]                                         # noqa: E731
        rows[pos[here]] = peak_boxes(frames[pos[here], 2], Lp[has], pick(T), pick(raw_w), pick(x_min), pick(y_min),
                                     pick(y_max), pad)
    return rows


def workspace_pieces(T, caps, omit=False):
    """(ws_off int64 per line, total bytes): line q's piece holds the moves of any text of at most caps[q] characters
    (ta_forced_workspace_bytes never decreases with L); a line with cap 0 has none.  omit: the pieces of
    ta_forced_align_omit_lines (ta_forced_omit_workspace_bytes, which never decreases with L either)"""
    f = _native.lib.ta_forced_omit_workspace_bytes if omit else _native.lib.ta_forced_workspace_bytes
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
    keep: the device buffers stay (self.d) and forced() / columns() can be launched again -- tools/refine_time.py.
    confidence: the per-character confidence of the aligned lines as well: ta_forced_confidence_lines
    behind the aligner, on its slots and with its t_peak as queries where they lie, ta_confidence_pages behind the columns
    (per transcript character and per syllable; the syllables' character ranges are formed on the host before the launch),
    and six more arrays in the same download; complete() leaves them in self.conf.  Without it nothing of this is
    allocated, uploaded, launched or downloaded.
    posterior: the sum-product posteriors of the aligned lines as well ("Inside the pipeline"):
    ta_forced_posterior_lines behind the aligner (posterior_lines()), ta_posterior_pages behind the columns
    (posterior_pages(); the syllable spans are the confidence's, uploaded once) and eleven more arrays in the same
    download; complete() forms the per-line values with posterior_values / loglik_bits on the host and leaves everything
    in self.post.  Without it nothing of this is allocated, uploaded, launched or downloaded.
    omit_q: None, or the price (omit_units) of a character the forced alignment may leave out:
    the workspace pieces are ta_forced_omit_workspace_bytes', forced() calls ta_forced_align_omit_lines, columns()
    ta_refine_columns_omit, and one more array -- omitted, per chunk line -- joins the download; complete() builds the box rows
    from the present characters alone (present_box_rows) and leaves the counts in self.omitted.  Strict lattice only: not
    with confidence or posterior.  With None not one of these branches runs."""
    last_bytes = None                # (workspace, probabilities) of the most recent chunk: tools/refine_time.py
    last_conf_bytes = None           # the confidence workspace of the most recent chunk that had one: tools/refine_conf_time.py
    last_post_bytes = None           # the posterior workspace of the most recent chunk that had one: tools/refine_post_time.py

    def __init__(self, chunk, batch, ratio, keep=False, confidence=False, posterior=False, omit_q=None):
        from . import harvest, page_batch as pb
        if omit_q is not None and (confidence or posterior):
            raise ValueError("confidence and posteriors are defined on the strict lattice only: not with omit_q")
        self.omit_q, self.omitted = omit_q, None
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
        ws_off, ws_bytes = workspace_pieces(self.T, self.caps, omit=True) if omit_q is not None else \
            workspace_pieces(self.T, self.caps)
        plain = np.asarray([pb.plain_page(tr, sy) for tr, sy in zip(chunk.transcripts, chunk.syls_all)], dtype=np.uint8)
        self.box_base = int(np.asarray(chunk.boxes).reshape(-1, 4).shape[0])
        Refining.last_bytes = (ws_bytes, int(probs.numel()) * 4)
        self.stream = torch.cuda.current_stream(dev)
        probs.record_stream(self.stream)                 # written on the recogniser's stream, read here
        pad1 = lambda a: a if a.size else np.zeros(1, a.dtype)                                      # noqa: E731
        names = ("o_line", "idx", "row", "T", "ws_off", "cap", "plain", "line_first")
        up = [pad1(o_cat), pad1(idx_cat), np.ascontiguousarray(st["row_start_host"][:nlines], dtype=np.int64), self.T, ws_off,
              self.caps, plain, np.ascontiguousarray(line_first, dtype=np.int64)]
        self.confidence, self.conf = bool(confidence), None
        self.posterior, self.post = bool(posterior), None
        if confidence or posterior:
            # per page, for EVERY syllable of its transcript, the range of characters the glue forms its box over; none
            # for a page off the array path
            spans = [pb.syllable_spans(tr, sy) if ok else (np.zeros(0, np.int64),) * 2
                     for tr, sy, ok in zip(chunk.transcripts, chunk.syls_all, plain)]
            self.syl_off = np.concatenate([[0], np.cumsum([len(f) for f, _ in spans])]).astype(np.int64)
            self.t_off = np.concatenate([[0], np.cumsum([len(tr) for tr in chunk.transcripts])]).astype(np.int64)
            names += ("syl_first", "syl_last", "syl_off")
            up += [pad1(cat([f for f, _ in spans], np.int32)), pad1(cat([l for _, l in spans], np.int32)), self.syl_off]
        d = dict(zip(names, _native.upload_packed(up, dev)))
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
        if omit_q is not None:
            d.update(omitted=torch.empty(nlines, **i32))
        if confidence or posterior:
            label_cap, nsyl = int(tb.labels.numel()), int(self.syl_off[-1])
            d.update(nsyl=nsyl)
        if confidence:
            i64 = dict(dtype=torch.int64, device=dev)
            cws = int(_native.lib.ta_forced_confidence_lines_workspace_bytes(label_cap, int(self.caps.max())))
            if cws < 0:
                raise ValueError("the chunk's transcripts are longer than ta_forced_confidence_lines sizes a workspace for")
            Refining.last_conf_bytes = cws
            d.update(cws_bytes=cws, cwork=torch.empty(max(cws, 16), dtype=torch.uint8, device=dev),
                     conf=torch.empty(label_cap, **i64), rival=torch.empty(label_cap, **i32), c_status=torch.empty(nlines, **i32),
                     char_conf=torch.empty(max(d["t_len"], 1), **i64), syl_conf=torch.empty(max(nsyl, 1), **i64),
                     p_status=torch.empty(nprob, **i32))
        if posterior:
            f64 = dict(dtype=torch.float64, device=dev)
            pws = int(_native.lib.ta_forced_posterior_lines_workspace_bytes(label_cap, int(self.caps.max())))
            if pws < 0:
                raise ValueError("the chunk's transcripts are longer than ta_forced_posterior_lines sizes a workspace for")
            Refining.last_post_bytes = pws
            d.update(pws_bytes=pws, pwork=torch.empty(max(pws, 16), dtype=torch.uint8, device=dev),
                     own_m=torch.empty(label_cap, **f64), own_x=torch.empty(label_cap, **i32),
                     rival_m=torch.empty(label_cap, **f64), rival_x=torch.empty(label_cap, **i32),
                     rival_state=torch.empty(label_cap, **i32), z_m=torch.empty(nlines, **f64), z_x=torch.empty(nlines, **i32),
                     s_status=torch.empty(nlines, **i32), char_post=torch.empty(max(d["t_len"], 1), **f64),
                     syl_post=torch.empty(max(nsyl, 1), **f64), pp_status=torch.empty(nprob, **i32))
        self.d = d
        self.forced()
        if confidence:
            self.confidence_lines()
        if posterior:
            self.posterior_lines()
        self.columns()
        if confidence:
            self.confidence_pages()
        if posterior:
            self.posterior_pages()
        d.update(acc_line=tb.acc_line, slot_L=tb.L, lab_off=tb.lab_off, count=tb.count, h_status=tb.status[:nprob])
        self.names = DOWNLOAD + (CONFIDENCE_DOWNLOAD if confidence else ()) + (POSTERIOR_DOWNLOAD if posterior else ()) + \
            (OMIT_DOWNLOAD if omit_q is not None else ())
        self.download = _native.download_begin([d[name] for name in self.names])
        if not keep:
            self.d = None
        self.refined = None

    def forced(self):
        """ta_forced_align_lines on the harvest's packed slots, where they lie (with omit_q: ta_forced_align_omit_lines)"""
        d, tb, p = self.d, self.d["tb"], lambda t: t.data_ptr()                                     # noqa: E731
        probs = d["probs"]
        if self.omit_q is not None:
            _native.check(_native.lib.ta_forced_align_omit_lines(
                p(probs), p(d["row"]), p(d["T"]), p(d["ws_off"]), p(d["cap"]), p(tb.acc_line), p(tb.L), p(tb.lab_off),
                p(tb.labels), p(tb.count), self.nlines, self.nlines, int(probs.shape[1]), int(probs.shape[0]),
                int(tb.labels.numel()), self.T.ctypes.data, self.caps.ctypes.data, int(self.omit_q), p(d["work"]),
                d["ws_bytes"], p(d["frames"]), p(d["score"]), p(d["f_status"]), self.stream.cuda_stream),
                "ta_forced_align_omit_lines")
            return
        _native.check(_native.lib.ta_forced_align_lines(
            p(probs), p(d["row"]), p(d["T"]), p(d["ws_off"]), p(d["cap"]), p(tb.acc_line), p(tb.L), p(tb.lab_off), p(tb.labels),
            p(tb.count), self.nlines, self.nlines, int(probs.shape[1]), int(probs.shape[0]), int(tb.labels.numel()),
            self.T.ctypes.data, self.caps.ctypes.data, p(d["work"]), d["ws_bytes"], p(d["frames"]), p(d["score"]),
            p(d["f_status"]), self.stream.cuda_stream), "ta_forced_align_lines")

    def columns(self):
        """ta_refine_columns on the aligner's columns, the harvest's tables and the forced alignment's status (with omit_q:
        ta_refine_columns_omit, on its frames as well)"""
        d, tb, p = self.d, self.d["tb"], lambda t: t.data_ptr()                                     # noqa: E731
        batch = d["batch"]
        if self.omit_q is not None:
            _native.check(_native.lib.ta_refine_columns_omit(
                p(batch.ops), p(batch.ops_off), p(batch.ops_len), int(batch.ops.numel()), p(batch.t_off), p(batch.o_off),
                d["t_len"], d["o_len"], self.nprob, p(d["o_line"]), p(d["line_first"]), p(d["idx"]), p(tb.table), p(tb.status),
                self.nlines, p(tb.acc_line), p(tb.L), p(tb.lab_off), p(tb.count), self.nlines, int(tb.labels.numel()),
                p(d["f_status"]), p(d["frames"]), p(d["plain"]), self.box_base, p(d["ops_new"]), p(d["ops_new_len"]),
                p(d["idx_new"]), p(d["idx_new_len"]), p(d["refined"]), p(d["slot"]), p(d["omitted"]), p(d["r_status"]),
                self.stream.cuda_stream), "ta_refine_columns_omit")
            return
        _native.check(_native.lib.ta_refine_columns(
            p(batch.ops), p(batch.ops_off), p(batch.ops_len), int(batch.ops.numel()), p(batch.t_off), p(batch.o_off), d["t_len"],
            d["o_len"], self.nprob, p(d["o_line"]), p(d["line_first"]), p(d["idx"]), p(tb.table), p(tb.status), self.nlines,
            p(tb.acc_line), p(tb.L), p(tb.lab_off), p(tb.count), self.nlines, int(tb.labels.numel()), p(d["f_status"]),
            p(d["plain"]), self.box_base, p(d["ops_new"]), p(d["ops_new_len"]), p(d["idx_new"]), p(d["idx_new_len"]),
            p(d["refined"]), p(d["slot"]), p(d["r_status"]), self.stream.cuda_stream), "ta_refine_columns")

    def _slots_head(self):
        """the arguments ta_forced_confidence_lines and ta_forced_posterior_lines share, up to the workspace"""
        d, tb, p = self.d, self.d["tb"], lambda t: t.data_ptr()                                     # noqa: E731
        probs = d["probs"]
        return (p(probs), p(d["row"]), p(d["T"]), p(d["cap"]), p(tb.acc_line), p(tb.L), p(tb.lab_off), p(tb.labels),
                p(tb.count), p(d["f_status"]), p(d["frames"]), self.nlines, self.nlines, int(probs.shape[1]),
                int(probs.shape[0]), int(tb.labels.numel()), self.T.ctypes.data, self.caps.ctypes.data)

    def _pages_call(self, entry, values, status, outputs):
        """ta_confidence_pages or ta_posterior_pages: the slots' `values` and their `status`, the arguments the two share,
        `outputs`"""
        d, tb, p = self.d, self.d["tb"], lambda t: t.data_ptr()                                     # noqa: E731
        args = [p(d[name]) for name in values] + [
            p(tb.lab_off), p(tb.L), p(tb.count), p(d[status]), self.nlines, int(tb.labels.numel()), p(tb.table),
            p(d["line_first"]), p(d["refined"]), p(d["slot"]), self.nlines, p(d["batch"].t_off), d["t_len"], p(d["syl_first"]),
            p(d["syl_last"]), p(d["syl_off"]), d["nsyl"], self.nprob] + [p(d[name]) for name in outputs]
        _native.check(getattr(_native.lib, entry)(*(args + [self.stream.cuda_stream])), entry)

    def confidence_lines(self):
        """ta_forced_confidence_lines behind forced(): the same slots, the aligner's status and its t_peak where they lie"""
        d, p = self.d, lambda t: t.data_ptr()                                                       # noqa: E731
        _native.check(_native.lib.ta_forced_confidence_lines(
            *self._slots_head(), p(d["cwork"]), d["cws_bytes"], p(d["conf"]), p(d["rival"]), p(d["c_status"]),
            self.stream.cuda_stream), "ta_forced_confidence_lines")

    def confidence_pages(self):
        """ta_confidence_pages behind columns(): the slots' confidences per transcript character and per syllable"""
        self._pages_call("ta_confidence_pages", ("conf",), "c_status", ("char_conf", "syl_conf", "p_status"))

    def posterior_lines(self):
        """ta_forced_posterior_lines behind forced(): the same slots, the aligner's status and its t_peak where they lie"""
        d, p = self.d, lambda t: t.data_ptr()                                                       # noqa: E731
        _native.check(_native.lib.ta_forced_posterior_lines(
            *self._slots_head(), p(d["pwork"]), d["pws_bytes"], *[p(d[name]) for name in POSTERIOR_DOWNLOAD[:8]],
            self.stream.cuda_stream), "ta_forced_posterior_lines")

    def posterior_pages(self):
        """ta_posterior_pages behind columns(): the slots' posteriors per transcript character and per syllable"""
        self._pages_call("ta_posterior_pages", ("own_m", "own_x", "z_m", "z_x"), "s_status", POSTERIOR_DOWNLOAD[8:])

    def complete(self, chunk, waiter=None):
        """wait for the download, refuse what the kernels refused (RuntimeError, the page named), build the new box rows on
        the host (peak_boxes: the one-decimal rule stays there) and hand columns, rows and boxes to replace_columns()"""
        from . import harvest, ocr
        got, self.download = dict(zip(self.names, self.download.wait(waiter))), None
        self.d = None
        page = lambda p: chunk.page_ids[p] if chunk.page_ids is not None else p                      # noqa: E731

        def refused(entry, status, texts):               # a status per page: the first page an entry refused
            bad = np.flatnonzero(status)
            if bad.size:
                raise RuntimeError("%s refused page %d on the device: %s"
                                   % (entry, page(int(bad[0])), texts.get(int(status[bad[0]]), "?")))
        refused("ta_harvest_lines", got["h_status"], harvest.STATUS)
        count = got["count"]
        if (count < 0).any():
            raise RuntimeError("ta_harvest_pack found a row of the table out of bounds on the device")
        refused("ta_refine_columns" if self.omit_q is None else "ta_refine_columns_omit", got["r_status"], REFINE_STATUS)
        k, nl = int(count[0]), int(count[1])
        acc, L, lab_off = got["acc_line"][:k].astype(np.int64), got["slot_L"][:k].astype(np.int64), got["lab_off"][:k]

        def slots(lines_entry, s_status, pages_entry, p_status, per_slot, char, syl):
            """what the two kernels of a switch refused; then per chunk line per_slot(slot, first label, end) of its
            slot, None for a line without a value, and the per-character and per-syllable arrays cut into pages"""
            s_status = got[s_status][:k]
            bad = np.flatnonzero((s_status != OK) & (s_status != CONF_SKIPPED))
            if bad.size:
                raise RuntimeError("%s refused line %d of the chunk on the device: %s"
                                   % (lines_entry, int(acc[bad[0]]), STATUS.get(int(s_status[bad[0]]), "?")))
            refused(pages_entry, got[p_status], CONF_PAGES_STATUS)
            lines = [None] * self.nlines
            for s in np.flatnonzero(s_status == OK):
                lines[int(acc[s])] = per_slot(int(s), int(lab_off[s]), int(lab_off[s]) + int(L[s]))
            cut = lambda x, off: [x[int(a):int(b)].copy() for a, b in zip(off[:-1], off[1:])]      # noqa: E731
            of = lambda pick: [None if ln is None else pick(ln) for ln in lines]                    # noqa: E731
            return of, {"char": cut(got[char], self.t_off), "syllable": cut(got[syl], self.syl_off)}
        if self.posterior:                               # the host arithmetic of refine_pages' LinePosterior
            of, self.post = slots("ta_forced_posterior_lines", "s_status", "ta_posterior_pages", "pp_status",
                                  lambda s, a, b: LinePosterior(got, a, b, s), "char_post", "syl_post")
            self.post.update(posterior=of(lambda lp: lp.posterior), rival_posterior=of(lambda lp: lp.rival_posterior),
                             posterior_rival=of(lambda lp: lp.rival_state), loglik_bits=of(lambda lp: lp.loglik_bits))
        if self.confidence:
            of, self.conf = slots("ta_forced_confidence_lines", "c_status", "ta_confidence_pages", "p_status",
                                  lambda s, a, b: (got["conf"][a:b].copy(), got["rival"][a:b].copy()), "char_conf", "syl_conf")
            self.conf.update(confidence=of(lambda cr: cr[0]), rival=of(lambda cr: cr[1]))
        old = np.asarray(chunk.boxes, dtype=np.int64).reshape(-1, 4)
        if k:
            # a row per label of every packed slot, at box_base + lab_off[k]; the rows of a slot that was not aligned hold
            # whatever its frames held and are never referenced
            done = (got["f_status"][:k] == OK) & (L <= MAX_TARGET)
            x_min, y_min, y_max = chunk.strip_geometry(acc)
            T, raw_w = self.T[acc].astype(np.int64), np.asarray(chunk.widths, dtype=np.int64)[acc]
            if self.omit_q is not None:                  # rows for the present characters alone, where the columns point
                new = present_box_rows(got["frames"][:nl], L, lab_off, T, raw_w, x_min, y_min, y_max, ocr.PAD, done=done)
            else:
                t_peak = np.where(np.repeat(done, L), got["frames"][:nl, 2], 0)
                new = peak_boxes(t_peak, L, T, raw_w, x_min, y_min, y_max, ocr.PAD)
            boxes = np.concatenate([old, new])
        else:
            boxes = old
        ops_r, idx_r = [], []
        for p in range(self.nprob):
            a = int(self.ops_off[p])
            ops_r.append(got["ops_new"][a:a + int(got["ops_new_len"][p])].copy())
            idx_r.append(got["idx_new"][a:a + int(got["idx_new_len"][p])].astype(np.int64))
        self.refined = got["refined"].astype(bool)
        if self.omit_q is not None:
            self.omitted = got["omitted"].astype(np.int32)
        chunk.replace_columns(ops_r, idx_r, boxes)


class PageScope(object):
    """one page of process_batch(..., refine_scope="page", page_scope_out=...): reason (0 = refined at page scope, else a key
    of PAGE_SCOPE), windows ((lo, hi) int32 per line; None unless reason is 0 or PAGE_NO_PATH), frames ((n, 4) int32 line,
    t_first, t_last, t_peak per transcript character; None for a page that was not refined), score (None likewise) -- what
    refine_pages(scope="page") returns for that page in page_scope, windows, page_frames and page_score.  omitted (with
    page_scope_omit): the number of OMITTED rows of a refined page's frames -- page_omitted --, None
    for a page that was not refined and without the switch; the windows then also stay with PAGE_ALL_OMITTED"""
    __slots__ = ("reason", "windows", "frames", "score", "omitted")

    def __init__(self, reason, windows=None, frames=None, score=None, omitted=None):
        self.reason, self.windows, self.frames, self.score, self.omitted = int(reason), windows, frames, score, omitted


def replace_page_columns(chunk, line_first, T, ops_old, page_frames):
    """the host tail of page scope, refine_pages' and the pipeline's: every page with frames (page_frames[p]: (n, 4), None
    for a page that is not refined) has ALL its columns replaced by the n columns page_columns makes of them, boxed on the
    host (the one-decimal rule); every other page keeps ops_old[p] and its rows.  Hands the lot to chunk.replace_columns()
    and returns (refined: bool per chunk line, frames: per line the rows of the characters the path put on it or None,
    ops, idx)."""
    from . import ocr
    lf = np.asarray(line_first, dtype=np.int64)
    T = np.asarray(T, dtype=np.int64)
    nlines = int(lf[-1])
    refined = np.zeros(nlines, dtype=bool)
    frames = [None] * nlines
    x_min, y_min, y_max = chunk.strip_geometry()
    widths = np.asarray(chunk.widths, dtype=np.int64)
    boxes = [np.asarray(chunk.boxes, dtype=np.int64).reshape(-1, 4)]
    rows = len(boxes[0])
    ops_r, idx_r = [], []
    for p in range(len(lf) - 1):
        if page_frames[p] is None:
            ops_r.append(np.asarray(ops_old[p], dtype=np.uint8))
            idx_r.append(np.asarray(chunk.idxs[p], dtype=np.int64))
            continue
        a, b = int(lf[p]), int(lf[p + 1])
        fr = page_frames[p]
        o, i, new = page_columns(fr, T[a:b], widths[a:b], x_min[a:b], y_min[a:b], y_max[a:b], ocr.PAD, rows)
        ops_r.append(o)
        idx_r.append(i)
        boxes.append(new.reshape(-1, 4))
        rows += len(new)
        refined[a:b] = True
        for q in range(a, b):
            frames[q] = fr[fr[:, 0] == q - a][:, 1:]
    chunk.replace_columns(ops_r, idx_r, np.concatenate(boxes))
    return refined, frames, ops_r, idx_r


def page_caps(transcripts):
    """per page the widest window the host sizes ta_forced_align_pages_gated's workspace for: min(n, MAX_TARGET)"""
    return np.minimum(np.asarray([len(tr) for tr in transcripts], dtype=np.int64), MAX_TARGET).astype(np.int32)


def page_workspace_pieces(T, line_first, caps, omit=False):
    """(ws_off int64 per line, total bytes) of ta_forced_align_pages_gated: line q's piece holds the moves of the variant
    of its page's cap -- the footprint never decreases with the variant, so it holds whatever variant the device's windows
    call for.  ValueError for timesteps the entry does not take.  omit: the pieces of ta_forced_align_pages_omit_gated --
    the bit rows behind the moves (ta_forced_page_omit_gated_workspace_bytes, which never decreases with the cap either)"""
    lib = _native.lib
    ws_bytes_of = lib.ta_forced_page_omit_gated_workspace_bytes if omit else lib.ta_forced_page_gated_workspace_bytes
    lf = np.asarray(line_first, dtype=np.int64)
    t64 = np.asarray(T, dtype=np.int64)
    if len(t64) and (t64.min() < 1 or t64.max() > MAX_T):
        raise ValueError("a line's timesteps are outside 1 .. %d" % MAX_T)
    K = np.asarray([lib.ta_forced_page_variant(int(c)) for c in caps], dtype=np.int64)
    Kq = np.repeat(K, np.diff(lf))
    size = 256 * (np.where(Kq == 32, 2 * t64, -(-t64 // np.maximum(16 // Kq, 1))) + (-(-t64 // (32 // Kq)) if omit else 0))
    T32 = np.ascontiguousarray(T, dtype=np.int32)
    for p in range(len(caps)):
        a, b = int(lf[p]), int(lf[p + 1])
        if b > a and int(size[a:b].sum()) != ws_bytes_of(b - a, T32[a:].ctypes.data, int(caps[p])):
            raise RuntimeError("the workspace pieces disagree with ta_forced_page%s_gated_workspace_bytes" % ("_omit" if omit else ""))
    off = np.zeros(len(size), dtype=np.int64)
    if len(size):
        off[1:] = np.cumsum(size)[:-1]
    return off, int(size.sum())


PAGE_WINDOWS_STATUS = {_native.TA_PAGE_WINDOWS_BOUNDS: "the page's own offsets are out of bounds"}
PAGE_DOWNLOAD = ("reason", "lo", "hi", "frames", "score", "status", "h_status", "ops", "ops_len")


class PageRefining(object):
    """A chunk's refinement at PAGE scope on its way (alignToOCR.PageChunk.align with refine and page_margin; DESIGN.md
    section 14.14): ta_harvest_lines and ta_harvest_pack, ta_page_windows (lo, hi per line and a reason per page, from the
    harvest table where it lies) and ta_forced_align_pages_gated (one launch per variant up to the widest cap's; a page
    with a reason is passed over) enqueued behind the aligner's launch on the stream it went to, and ONE pinned download
    started behind them: reason, lo, hi, frames, score, status, the harvest's status -- and the aligner's columns, which a
    page that is not refined forms its syllables from.  The transcript's classes go up in the chunk's packed upload and
    are both the harvest's t_class and the aligner's labels (lab_off = the batch's t_off: the pages are not re-packed).
    complete() waits for that download alone.  Every device buffer is given back when the download has been started, the
    probabilities with the chunk.  ta_forced_align_lines, ta_refine_columns and their buffers play no part.
    keep: the device buffers stay (self.d) and windows() / forced() can be launched again -- tools/refine_page_time.py.
    omit_q: None, or the price (omit_units) at which the page's one path may leave a character out (DESIGN.md section
    14.17): the pieces are ta_forced_page_omit_gated_workspace_bytes', windows() calls ta_page_windows_omit and forced()
    ta_forced_align_pages_omit_gated; the same nine arrays come back in the same download.  complete() then accepts no
    NOPATH, gives a page whose frames are all OMITTED PAGE_ALL_OMITTED (it stays unrefined, as in _refine_at_page_scope)
    and counts the omitted characters of a refined page from its frames (PageScope.omitted)."""
    last_bytes = None                # (workspace, probabilities) of the most recent chunk: tools/refine_page_time.py
    conf = post = None               # (what PageChunk.finish() takes from a Refining: page scope has neither)

    def __init__(self, chunk, batch, ratio, margin, keep=False, omit_q=None):
        from . import harvest, page_batch as pb
        self.omit_q = None if omit_q is None else int(omit_q)
        rec, st = chunk.rec, chunk.st
        dev = batch.device
        o_line, line_first, T = chunk.line_table()
        nprob, nlines = int(batch.nprob), len(T)
        self.nprob, self.nlines, self.margin = nprob, nlines, int(margin)
        probs = st["probs"]
        cat = lambda arrs, dt: np.concatenate(arrs).astype(dt) if arrs else np.zeros(0, dt)        # noqa: E731
        classes = cat([harvest.transcript_classes(rec.model.codec, tr) for tr in chunk.transcripts], np.int32)
        o_cat = cat(o_line, np.int32)
        self.T = np.ascontiguousarray(T, dtype=np.int32)
        self.line_first = np.ascontiguousarray(line_first, dtype=np.int64)
        self.t_off = np.concatenate([[0], np.cumsum([len(tr) for tr in chunk.transcripts])]).astype(np.int64)
        self.caps = page_caps(chunk.transcripts)
        ws_off, ws_bytes = page_workspace_pieces(self.T, self.line_first, self.caps, omit=self.omit_q is not None)
        plain = np.asarray([pb.plain_page(tr, sy) for tr, sy in zip(chunk.transcripts, chunk.syls_all)], dtype=np.uint8)
        PageRefining.last_bytes = (ws_bytes, int(probs.numel()) * 4)
        self.ops_off, self.ops_cap = batch.ops_off_host, batch.cap_host
        self.stream = torch.cuda.current_stream(dev)
        probs.record_stream(self.stream)                 # written on the recogniser's stream, read here
        pad1 = lambda a: a if a.size else np.zeros(1, a.dtype)                                      # noqa: E731
        names = ("o_line", "t_class", "row", "T", "ws_off", "cap", "plain", "line_first")
        up = [pad1(o_cat), pad1(classes), np.ascontiguousarray(st["row_start_host"][:nlines], dtype=np.int64), self.T, ws_off,
              self.caps, plain, self.line_first]
        d = dict(zip(names, _native.upload_packed(up, dev)))
        tb = harvest.harvest_alignment(batch, d["o_line"] if len(o_cat) else o_cat, line_first,
                                       d["t_class"] if len(classes) else classes, d["T"], ratio)
        i32 = dict(dtype=torch.int32, device=dev)
        t_len = len(classes)
        d.update(probs=probs, batch=batch, tb=tb, t_len=t_len, ws_bytes=ws_bytes,
                 lo=torch.empty(nlines, **i32), hi=torch.empty(nlines, **i32), reason=torch.empty(nprob, **i32),
                 frames=torch.empty((max(t_len, 1), PAGE_FIELDS), **i32), score=torch.empty(nprob, dtype=torch.int64, device=dev),
                 status=torch.empty(nprob, **i32), work=torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev))
        self.d = d
        self.windows()
        self.forced()
        d.update(h_status=tb.status[:nprob], ops=batch.ops, ops_len=batch.ops_len)
        self.download = _native.download_begin([d[name] for name in PAGE_DOWNLOAD])
        if not keep:
            self.d = None
        self.refined = self.scope = None

    def windows(self):
        """ta_page_windows on the harvest's table and status, where they lie (with omit_q: ta_page_windows_omit)"""
        d, tb, p = self.d, self.d["tb"], lambda t: t.data_ptr()                                     # noqa: E731
        entry = "ta_page_windows" if self.omit_q is None else "ta_page_windows_omit"
        _native.check(getattr(_native.lib, entry)(
            p(tb.table), p(tb.status), p(d["line_first"]), p(d["batch"].t_off), p(d["t_class"]), p(d["T"]), p(d["plain"]),
            self.nprob, self.nlines, d["t_len"], self.margin, p(d["lo"]), p(d["hi"]), p(d["reason"]), self.stream.cuda_stream),
            entry)

    def forced(self):
        """ta_forced_align_pages_gated on the windows and reasons ta_page_windows wrote, where they lie (with omit_q:
        ta_forced_align_pages_omit_gated at that price)"""
        d, p = self.d, lambda t: t.data_ptr()                                                        # noqa: E731
        probs = d["probs"]
        if self.omit_q is not None:
            _native.check(_native.lib.ta_forced_align_pages_omit_gated(
                p(probs), p(d["row"]), p(d["T"]), p(d["line_first"]), p(d["lo"]), p(d["hi"]), p(d["t_class"]),
                p(d["batch"].t_off), p(d["ws_off"]), p(d["reason"]), p(d["cap"]), self.nprob, self.nlines, int(probs.shape[1]),
                int(probs.shape[0]), d["t_len"], self.T.ctypes.data, self.line_first.ctypes.data, self.t_off.ctypes.data,
                self.caps.ctypes.data, self.omit_q, p(d["work"]), d["ws_bytes"], p(d["frames"]), p(d["score"]), p(d["status"]),
                self.stream.cuda_stream), "ta_forced_align_pages_omit_gated")
            return
        _native.check(_native.lib.ta_forced_align_pages_gated(
            p(probs), p(d["row"]), p(d["T"]), p(d["line_first"]), p(d["lo"]), p(d["hi"]), p(d["t_class"]), p(d["batch"].t_off),
            p(d["ws_off"]), p(d["reason"]), p(d["cap"]), self.nprob, self.nlines, int(probs.shape[1]), int(probs.shape[0]),
            d["t_len"], self.T.ctypes.data, self.line_first.ctypes.data, self.t_off.ctypes.data, self.caps.ctypes.data,
            p(d["work"]), d["ws_bytes"], p(d["frames"]), p(d["score"]), p(d["status"]), self.stream.cuda_stream),
            "ta_forced_align_pages_gated")

    def complete(self, chunk, waiter=None):
        """wait for the download, refuse what the kernels refused (RuntimeError, the page named), and build on the host
        what refine_pages(scope="page") builds: replace_page_columns().  Leaves refined (a bool per chunk line) and scope
        (a PageScope per page)."""
        from . import harvest
        got, self.download = dict(zip(PAGE_DOWNLOAD, self.download.wait(waiter))), None
        self.d = None
        page = lambda p: chunk.page_ids[p] if chunk.page_ids is not None else p                      # noqa: E731

        def refused(entry, bad, status, texts):
            bad = np.flatnonzero(bad)
            if bad.size:
                raise RuntimeError("%s refused page %d on the device: %s"
                                   % (entry, page(int(bad[0])), texts.get(int(status[bad[0]]), "?")))
        reason, status = got["reason"].astype(np.int32), got["status"]
        refused("ta_harvest_lines", got["h_status"] != 0, got["h_status"], harvest.STATUS)
        omit = self.omit_q is not None
        aligner = "ta_forced_align_pages_omit_gated" if omit else "ta_forced_align_pages_gated"
        refused("ta_page_windows_omit" if omit else "ta_page_windows", reason < 0, reason, PAGE_WINDOWS_STATUS)
        refused(aligner, (status != OK) & ((status != NOPATH) | omit) & (status != CONF_SKIPPED), status, PAGE_STATUS)
        if ((status == CONF_SKIPPED) != (reason != 0)).any():
            raise RuntimeError("%s passed over a page that the window kernel found eligible, or the reverse" % aligner)
        lens = got["ops_len"][:self.nprob]
        if (lens < 0).any():
            raise RuntimeError("traceback of problem %d did not finish (a bounded wait between its waves ran out)"
                               % int(np.flatnonzero(lens < 0)[0]))
        reason[status == NOPATH] = PAGE_NO_PATH
        lf, t_off = self.line_first, self.t_off
        ops_old, page_frames, self.scope = [], [], []
        for p in range(self.nprob):
            end = int(self.ops_off[p] + self.ops_cap[p])
            ops_old.append(got["ops"][end - int(lens[p]):end].copy())
            a, b = int(lf[p]), int(lf[p + 1])
            win = (got["lo"][a:b].copy(), got["hi"][a:b].copy()) if reason[p] in (PAGE_REFINED, PAGE_NO_PATH) else None
            fr = got["frames"][int(t_off[p]):int(t_off[p + 1])].copy() if status[p] == OK else None
            if omit and fr is not None and (fr[:, 0] == OMITTED).all():
                reason[p], fr = PAGE_ALL_OMITTED, None   # a path that holds no character refines nothing
            page_frames.append(fr)
            self.scope.append(PageScope(reason[p], win, fr, int(got["score"][p]) if fr is not None else None,
                                        int((fr[:, 0] == OMITTED).sum()) if omit and fr is not None else None))
        self.refined = replace_page_columns(chunk, lf, self.T, ops_old, page_frames)[0]


def page_scope_without_lines(chunk, omit=False):
    """a chunk that has no text line at all has nothing for the device to do at page scope: a PageScope per page from
    page_scope_eligibility (omit: the rule of the lattice with omission) -- every page comes back unrefined, with the
    reason it would have had"""
    from . import harvest, page_batch as pb
    none = np.zeros((0, FIELDS), np.int32)
    return [PageScope(page_scope_eligibility(pb.plain_page(tr, sy), 0, harvest.transcript_classes(chunk.rec.model.codec, tr),
                                              none, none[:, 0], 0, omit=omit)[0])
            for tr, sy in zip(chunk.transcripts, chunk.syls_all)]


class RefineResult(object):
    """refine_pages' result: results (per page (syl_boxes, image, lines_peak_locs, all_chars), as process_batch returns
    them), indices / arrays (as its indices_out / arrays_out), refined (bool per text line, page after page), frames
    (per line an (L, 3) array of t_first, t_last, t_peak, None for a line that was not aligned), score (per line, None
    likewise), harvest (the HarvestResult), spans (locate: (a, b) per page, else None), object_pages (pages whose
    syllable search took the object path: returned unrefined).
    scope="page": page_scope (per page 0 = refined at page scope, else the reason it came back unrefined: the keys of
    PAGE_SCOPE), page_frames (per page the (n, 4) array line, t_first, t_last, t_peak of its transcript characters, None
    for a page that was not refined), page_score, windows (per page (lo, hi), None for a page that was not eligible);
    refined marks the lines of the refined pages, frames holds per such line the rows of the characters the path put on
    it, score stays None per line.  With scope="line" the four are None.
    page_omit: the reasons are the keys of PAGE_OMIT_SCOPE; page_frames[p] keeps the OMITTED
    rows of the characters the path left out, page_omitted[p] is their number (None for a page that was not refined,
    and the whole list None without page_omit), frames[q] holds line q's present characters.
    omitted (scope="line"): per line the number of characters of its text the path left out (always 0 without `omit`),
    None for a line that was not aligned; their rows of frames[q] are OMITTED.  None at page scope.
    refine_pages(confidence=True) (without it the four are None): confidence and rival (per line
    an (L,) int64 / int32 array at the line's own t_peak, None where frames[q] is None), char_confidence (per page an int64
    array over the page's transcript characters: kept character k of refined line q is character table[q][1] + k;
    NO_CONFIDENCE for a character on no refined line), syllable_confidence (per page a list aligned with results[p][0]:
    the smallest char_confidence among the syllable's transcript characters that have one, None if none has).
    refine_pages(posterior=True) (without it the six are None): posterior and rival_posterior (per
    line an (L,) float64 array at the line's own t_peak: the sum-product posterior of the character's state and the
    largest one of any other state), posterior_rival (per line (L,) int32: that state), loglik_bits (per line log2
    P(text | line)) -- each None where frames[q] is None; char_posterior (per page a float64 array over the page's
    transcript characters, char_confidence's mapping, NaN for a character on no refined line), syllable_posterior (per
    page a list aligned with results[p][0]: the smallest char_posterior among the syllable's characters that have one,
    None if none has).
    refine_pages(scope="page", page_confidence=True) (without it the two are None):
    page_confidence and page_rival (per page an (n,) int64 / int32 array over its transcript characters at the aligner's
    own line and t_peak, None for a page that was not refined); confidence, rival, char_confidence and syllable_confidence
    are filled from them as above (per line the values of the characters the path put on it), a rival being a PAGE state.
    refine_pages(scope="page", page_posterior=True) (without it the four are None):
    page_posterior, page_rival_posterior (per page an (n,) float64 array over its transcript characters at the aligner's
    own line and t_peak: the sum-product posterior over all legal paths of the page, and the largest one of any other
    live state), page_posterior_rival (per page (n,) int32: that PAGE state) and page_loglik_bits (per page log2
    P(transcript | page), a float) -- each None for a page that was not refined; posterior, rival_posterior,
    posterior_rival, char_posterior and syllable_posterior are filled from them as above, and loglik_bits[q] is None for
    every line: there is no likelihood per line at page scope."""
    omitted = page_omitted = None
    page_confidence = page_rival = None
    page_posterior = page_rival_posterior = page_posterior_rival = page_loglik_bits = None
    confidence = rival = char_confidence = syllable_confidence = None
    posterior = rival_posterior = posterior_rival = loglik_bits = char_posterior = syllable_posterior = None

    def __init__(self, results, indices, arrays, refined, frames, score, harvest, object_pages, page_scope=None):
        self.results, self.indices, self.arrays, self.refined = results, indices, arrays, refined
        self.frames, self.score, self.harvest, self.spans = frames, score, harvest, harvest.spans
        self.object_pages = object_pages
        self.page_scope, self.page_frames, self.page_score, self.windows = page_scope, None, None, None

    def __len__(self):
        return len(self.results)


class PageConfidence(object):
    """one page's confidences, as alignToOCR.process_batch / process hand them to confidence_out (DESIGN.md section
    14.10): char_confidence (int64 array over the page's transcript characters, NO_CONFIDENCE on no refined line),
    syllable_confidence (a list aligned with the page's syllable boxes: int, or None where no character of the syllable
    has a value), confidence / rival (per text line of the page an (L,) int64 / int32 array at the line's own t_peak, None
    for a line that was not aligned) -- the values RefineResult carries for the page under the same names"""
    __slots__ = ("char_confidence", "syllable_confidence", "confidence", "rival")

    def __init__(self, char_confidence, syllable_confidence, confidence, rival):
        self.char_confidence, self.syllable_confidence = char_confidence, syllable_confidence
        self.confidence, self.rival = confidence, rival


def result_confidence(res, p):
    """page p of a RefineResult of refine_pages(confidence=True) as a PageConfidence; likewise of
    refine_pages(scope="page", page_confidence=True), where `rival` holds PAGE states (0 .. 2 n of the page's text)"""
    a, b = int(res.harvest.line_first[p]), int(res.harvest.line_first[p + 1])
    return PageConfidence(res.char_confidence[p], res.syllable_confidence[p], res.confidence[a:b], res.rival[a:b])


class PagePosterior(object):
    """one page's posteriors, as alignToOCR.process_batch / process hand them to posterior_out:
    the values RefineResult carries for the page under the same names -- char_posterior, syllable_posterior, and per text
    line of the page posterior, rival_posterior, posterior_rival and loglik_bits (None for a line that was not aligned).
    PagePosterior(res, p): page p of a RefineResult of refine_pages(posterior=True); PagePosterior.of(...): the six values
    themselves (chunk_posterior).  page_loglik_bits: log2 P(transcript | page) of a page refined with
    refine_pages(scope="page", page_posterior=True) (rivals are PAGE states then, and loglik_bits
    holds None per line), else None."""
    __slots__ = ("char_posterior", "syllable_posterior", "posterior", "rival_posterior", "posterior_rival", "loglik_bits",
                 "page_loglik_bits")

    def __init__(self, res, p):
        a, b = int(res.harvest.line_first[p]), int(res.harvest.line_first[p + 1])
        self.char_posterior, self.syllable_posterior = res.char_posterior[p], res.syllable_posterior[p]
        self.posterior, self.rival_posterior = res.posterior[a:b], res.rival_posterior[a:b]
        self.posterior_rival, self.loglik_bits = res.posterior_rival[a:b], res.loglik_bits[a:b]
        bits = getattr(res, "page_loglik_bits", None)    # a result without page_posterior has none
        self.page_loglik_bits = None if bits is None else bits[p]

    @classmethod
    def of(cls, char_posterior, syllable_posterior, posterior, rival_posterior, posterior_rival, loglik_bits,
           page_loglik_bits=None):
        self = cls.__new__(cls)
        self.char_posterior, self.syllable_posterior = char_posterior, syllable_posterior
        self.posterior, self.rival_posterior = posterior, rival_posterior
        self.posterior_rival, self.loglik_bits = posterior_rival, loglik_bits
        self.page_loglik_bits = page_loglik_bits
        return self


def _page_values(none, n, indices, lines=(), spans=None, char=None, syl=None):
    """One page's values per transcript character and per syllable box, `none` marking "no value": NO_CONFIDENCE in int64
    arrays (a value is an int) or NaN in float64 ones (a float).  Characters: `char` where the device spread them, else the
    page's n characters with the values of `lines`, [(first character, values)], put in.  Syllables, for EVERY syllable of
    the transcript: `syl` where the device reduced them, else per (first, last) of `spans` the smallest value among its
    characters that have one; neither for a page off the array path (`syl` is empty then).  indices: per syllable box its
    syllable.  Returns (char, per box the value or None)."""
    nan = none != none
    have = (lambda v: ~np.isnan(v)) if nan else (lambda v: v != none)
    if char is None:
        char = np.full(n, none, dtype=np.float64 if nan else np.int64)
        for a, values in lines:
            char[a:a + len(values)] = values
    if spans is not None:
        syl = np.full(len(spans[0]), none, dtype=char.dtype)
        if len(syl):                                     # one reduceat serves every syllable: its range first .. last
            at = np.stack([spans[0], np.asarray(spans[1]) + 1], axis=1).astype(np.int64).reshape(-1)
            held = np.append(have(char), False)          # (one entry more: a range may end at the page's end)
            top = np.inf if nan else np.iinfo(np.int64).max
            least = np.minimum.reduceat(np.where(held, np.append(char, none), top), at)[::2]
            some = np.logical_or.reduceat(held, at)[::2]
            syl[some] = least[some]
    per_box = [None] * len(indices)
    if syl is not None and len(syl):
        picked = syl[np.asarray(indices, dtype=np.int64)]
        per_box = [(float if nan else int)(v) if h else None for v, h in zip(picked, have(picked))]
    return char, per_box


def _chunk_values(chunk, indices, got, none, per_line, make):
    """chunk_confidence and chunk_posterior: per page make(char, per box, *the page's lines of each name in per_line);
    got: what Refining.complete() left, None for a chunk that had nothing to refine"""
    first = chunk.first_line()
    out = []
    for p, tr in enumerate(chunk.transcripts):
        a, b = int(first[p]), int(first[p + 1])
        if got is None:
            out.append(make(*_page_values(none, len(tr), indices[p]), *[[None] * (b - a) for _ in per_line]))
        else:
            out.append(make(*_page_values(none, len(tr), indices[p], char=got["char"][p], syl=got["syllable"][p]),
                            *[got[name][a:b] for name in per_line]))
    return out


def chunk_confidence(chunk, indices):
    """per page of a finished PageChunk that refined with confidence its PageConfidence.  indices: per page the index of
    each syllable box's syllable among the transcript's non-empty syllables (finish()'s indices_out) -- they pick the
    boxes' values from the per-syllable array the device reduced.  A chunk that had nothing to refine has no values."""
    return _chunk_values(chunk, indices, chunk.conf, NO_CONFIDENCE, ("confidence", "rival"), PageConfidence)


def chunk_posterior(chunk, indices):
    """per page of a finished PageChunk that refined with posterior its PagePosterior, by chunk_confidence's rules: indices
    pick the boxes' values from the per-syllable array the device reduced; a chunk that had nothing to refine has no
    values (NaN per character, None per syllable and line), nor has a page off the array path per syllable."""
    return _chunk_values(chunk, indices, chunk.post, np.nan, ("posterior", "rival_posterior", "posterior_rival", "loglik_bits"),
                         PagePosterior.of)


def refine_pages(pages, transcripts, ocropus_model, seq_align_params=None, min_agreement=0.9, locate=False, scope="line",
                 margin=DEFAULT_MARGIN, omit=None, confidence=False, posterior=False, page_omit=None,
                 page_confidence=False, page_posterior=False, omit_confidence=False):
    """process_batch (one chunk) with the boxes of every ACCEPTED line refined by forced alignment: a RefineResult.

    The flow is harvest.harvest_pages' -- recognise, align, harvest -- with the recogniser's probabilities kept; one
    ta_forced_align then covers the accepted lines, and a line is refined if the harvest rule accepted it (reason 0:
    min_agreement and the other bits, harvest.py) and the kernel aligned it.  Every kept transcript character of a
    refined line gets the box the page path's construction yields for its peak; everything else keeps what it has.
    A page none of whose lines is refined comes out exactly as from process_batch.  ValueErrors as harvest_pages.
    scope="page": the lattice decides which character lies on which line.  A page is eligible if
    its syllables are formed on the array path, no transcript character is outside the codec, it has lines and text, the
    windows page_windows makes of its harvest rows and `margin` are no wider than 1023 characters and it has no more
    characters than frames; ONE ta_forced_align_pages call covers the eligible pages, and a page it finds a path for gets
    ALL its columns replaced by a pair column per transcript character, boxed as a refined line's characters are.  The
    harvest's accept / reject decisions and min_agreement play no part.  Every other page comes back as from
    process_batch, its reason in RefineResult.page_scope.  The page's OCR characters stay what they are.
    omit (line scope only): None, or the price in bits (omit_units) at which the forced alignment may leave a character of
    an accepted line's text out (the page abbreviates, spells differently, drops words).  A kept
    character the path omits becomes a transcript character alone, without a box, in its place; the present ones get
    their boxes as above; a line whose path holds no character at all is not refined.  RefineResult.frames[q] carries the
    OMITTED rows and RefineResult.omitted[q] their number.  The harvest rule is untouched: lower min_agreement to let the
    disagreeing lines in.  No value of omit has been validated on real pages.
    omit_confidence (line scope, with omit: ValueError without it, at page scope, or for anything but a bool): one more
    call, forced_omit_confidence on the aligned lines with omit_queries' queries and the probabilities still on the device
    (DESIGN.md section 14.18), fills RefineResult.confidence and rival per line -- a present character's confidence at its
    own t_peak on the lattice with omission, >= 0; an omitted character's largest confidence over the two frames around the
    place the path jumped it at, <= 0, minus it an UPPER bound of what the best path would lose if the character had to
    appear -- char_confidence with both kinds, and syllable_confidence, the smallest value among the syllable's PRESENT
    characters (None where it has none).  confidence=True together with omit stays the ValueError it is.  No threshold on it
    has been validated on real pages.
    confidence (line scope, strict lattice only: ValueError with omit or scope="page"): one more call,
    forced_confidence on the aligned lines with their own t_peak as queries and the probabilities still on the device,
    fills RefineResult.confidence, rival, char_confidence and syllable_confidence: how far the
    best path that keeps a character on its peak frame lies above the best path that puts anything else there.  No
    threshold on it has been validated on real pages.
    posterior (line scope, strict lattice only: ValueError with omit or scope="page"): one more call, forced_posterior on
    the aligned lines with their own t_peak as queries, fills RefineResult.posterior, rival_posterior, posterior_rival,
    loglik_bits, char_posterior and syllable_posterior: the probability, all paths summed, that a
    character holds its peak frame, and the text's likelihood per line.  Nothing about real pages has been measured.
    page_omit (page scope only; ValueError with scope="line", confidence or posterior, or outside 0 .. 1024 bits): None,
    or the price in bits (omit_units) at which the page's ONE path may leave a transcript character out (DESIGN.md
    section 14.12; `ta_forced_align_pages_omit`).  Eligibility is page scope's without the test of characters against
    frames -- every page with windows has a path -- and a page of more than 2^20 characters or 2^25 frames is
    PAGE_TOO_LONG.  A present character gets its pair column and box as above, an omitted one becomes a transcript
    character alone, without a box, in its place; a page whose path holds no character at all is left unrefined
    (PAGE_ALL_OMITTED).  RefineResult.page_frames[p] keeps the OMITTED rows, page_omitted[p] is their number and
    frames[q] holds line q's present characters; the reasons are PAGE_OMIT_SCOPE's.  NOT measured: the share of real
    pages this refines, the right page_omit, the right margin.
    page_confidence (page scope, strict lattice only: ValueError with scope="line", with page_omit, or for anything but a
    bool): one more call behind ta_forced_align_pages, forced_page_confidence over the pages it found a path for, with
    the aligner's own (line, t_peak) as queries and the probabilities still on the device: how
    far the best path through ALL lines of the page that keeps a character on its peak frame lies above the best one that
    puts any other live state there.  It fills RefineResult.page_confidence and page_rival (per page an (n,) int64 / int32
    array, None for a page that was not refined), confidence and rival (per line the page's values of the characters the
    path put on it), char_confidence (NO_CONFIDENCE throughout on a page that was not refined) and syllable_confidence,
    so result_confidence(res, p) works as at line scope -- but a rival is a PAGE state here, 0 .. 2 n of the page's text,
    not a state of the line's.  No threshold on it has been validated on real pages.
    page_posterior (page scope, strict lattice only: ValueError with scope="line", with page_omit, or for anything but a
    bool; allowed together with page_confidence): one more call behind ta_forced_align_pages, forced_page_posterior over
    the pages it found a path for, with the aligner's own (line, t_peak) as queries and the probabilities still on the
    device: the probability, ALL legal paths of the page summed, that a character holds its peak
    frame, and log2 P(transcript | page) -- the one fit measure that does not depend on how the harvest cut the transcript
    into lines.  It fills RefineResult.page_posterior, page_rival_posterior, page_posterior_rival (per page (n,) arrays)
    and page_loglik_bits (per page a float), None on a page that was not refined; posterior, rival_posterior and
    posterior_rival (per line the page's values of the characters the path put on it; loglik_bits[q] stays None: there is
    no likelihood per line at page scope), char_posterior (NaN throughout on a page that was not refined) and
    syllable_posterior, so PagePosterior(res, p) works as at line scope -- a rival is a PAGE state -- and carries the
    page's page_loglik_bits.  posterior=True at page scope stays the ValueError it is.  Nothing about real pages has been
    measured."""
    from . import harvest, ocr, page_batch as pb
    if scope not in ("line", "page"):
        raise ValueError("scope is 'line' or 'page'")
    if not isinstance(page_confidence, (bool, np.bool_)):
        raise ValueError("page_confidence is True or False")
    if page_confidence and scope != "page":
        raise ValueError("page_confidence goes with scope='page': at line scope the switch is confidence")
    if page_confidence and page_omit is not None:
        raise ValueError("page_confidence is defined on the strict lattice only: not with page_omit")
    if not isinstance(page_posterior, (bool, np.bool_)):
        raise ValueError("page_posterior is True or False")
    if page_posterior and scope != "page":
        raise ValueError("page_posterior goes with scope='page': at line scope the switch is posterior")
    if page_posterior and page_omit is not None:
        raise ValueError("page_posterior is defined on the strict lattice only: not with page_omit")
    if not isinstance(omit_confidence, (bool, np.bool_)):
        raise ValueError("omit_confidence is True or False")
    if omit_confidence and (omit is None or scope == "page"):
        raise ValueError("omit_confidence is the confidence on one line's lattice with omission: it needs omit and scope='line'")
    if page_omit is not None:
        if scope != "page":
            raise ValueError("page_omit goes with scope='page': at line scope the price is omit")
        if confidence or posterior:
            raise ValueError("confidence and posteriors are defined on the strict lattice of one line: not with page_omit")
        if omit is not None:
            raise ValueError("page scope has no omission through omit: the price at page scope is page_omit")
    page_omit_q = None if page_omit is None else omit_units(page_omit)
    if posterior and (omit is not None or scope == "page"):
        raise ValueError("posteriors are defined on the strict lattice of one line: not with omit or scope='page'")
    if confidence and (omit is not None or scope == "page"):
        raise ValueError("confidence is defined on the strict lattice of one line: not with omit or scope='page'")
    if omit is not None and scope == "page":
        raise ValueError("page scope has no omission through omit: omit goes with scope='line', the price at page scope "
                         "is page_omit")
    omit_q = None if omit is None else omit_units(omit)
    if scope == "page" and not (isinstance(margin, (int, np.integer)) and not isinstance(margin, bool) and margin >= 0):
        raise ValueError("margin is a number of characters, 0 or more")
    hres, chunk = harvest._harvest_flow(pages, transcripts, ocropus_model, seq_align_params, min_agreement, locate,
                                        want_probs=True)
    if scope == "page":
        return _refine_at_page_scope(hres, chunk, int(margin), page_omit_q, bool(page_confidence), bool(page_posterior))
    rec, st = chunk.rec, chunk.st
    nlines = len(hres)
    packed = hres.packed
    take = np.flatnonzero(packed["L"] <= MAX_TARGET)
    acc = packed["acc_line"][take].astype(np.int64)
    L, lab_off = packed["L"][take].astype(np.int64), packed["lab_off"][take]
    refined = np.zeros(nlines, dtype=bool)
    frames, score, omitted = [None] * nlines, [None] * nlines, [None] * nlines
    line_conf, line_rival = [None] * nlines, [None] * nlines
    line_post = [None] * nlines
    T_all = np.asarray(st["T_host"], dtype=np.int64)[:nlines]
    if len(acc):
        with torch.cuda.device(rec.device):
            got = forced_alignment(st["probs"], np.asarray(st["row_start_host"])[acc], T_all[acc], packed["labels"], lab_off, L,
                                   host=True, omit_q=omit_q)
        for k, q in enumerate(acc):
            if got["status"][k] == OK:
                frames[q] = got["frames"][lab_off[k]:lab_off[k] + L[k]]
                score[q] = int(got["score"][k])
                omitted[q] = int((frames[q][:, 0] == OMITTED).sum())
                refined[q] = omitted[q] < len(frames[q])     # a path that holds no character refines nothing
        ok = np.flatnonzero(got["status"] == OK)
        for on, entry, call in ((confidence, "ta_forced_confidence", forced_confidence),
                                (posterior, "ta_forced_posterior", forced_posterior)):
            if not (on and len(ok)):
                continue
            with torch.cuda.device(rec.device):
                m = call(st["probs"], np.asarray(st["row_start_host"])[acc[ok]], T_all[acc[ok]], packed["labels"], lab_off[ok],
                         L[ok], got["frames"][:, 2], host=True)
            bad = np.flatnonzero(m["status"])
            if bad.size:
                raise RuntimeError("%s refused line %d on the device: %s"
                                   % (entry, int(acc[ok[bad[0]]]), STATUS.get(int(m["status"][bad[0]]), "?")))
            for j, k in enumerate(ok):
                a, b = int(lab_off[k]), int(lab_off[k] + L[k])
                if call is forced_confidence:
                    line_conf[acc[k]], line_rival[acc[k]] = m["confidence"][a:b], m["rival"][a:b]
                else:
                    line_post[acc[k]] = LinePosterior(m, a, b, j)
        if omit_confidence and len(ok):
            qs_ = [omit_queries(got["frames"][lab_off[k]:lab_off[k] + L[k]], T_all[acc[k]]) for k in ok]
            nq = np.asarray([len(qc) for qc, _ in qs_], dtype=np.int64)
            q_off = np.concatenate([[0], np.cumsum(nq)[:-1]])
            with torch.cuda.device(rec.device):
                m = forced_omit_confidence(st["probs"], np.asarray(st["row_start_host"])[acc[ok]], T_all[acc[ok]],
                                           packed["labels"], lab_off[ok], L[ok], np.concatenate([qc for qc, _ in qs_]),
                                           np.concatenate([qf for _, qf in qs_]), q_off, nq, omit_q, host=True)
            bad = np.flatnonzero(m["status"])
            if bad.size:
                raise RuntimeError("ta_forced_omit_confidence refused line %d on the device: %s"
                                   % (int(acc[ok[bad[0]]]), STATUS.get(int(m["status"][bad[0]]), "?")))
            for j, k in enumerate(ok):
                a, b = int(q_off[j]), int(q_off[j] + nq[j])
                both = omit_values(L[k], qs_[j][0], m["confidence"][a:b], m["rival"][a:b])
                line_conf[acc[k]], line_rival[acc[k]] = both[:, 0].copy(), both[:, 1].astype(np.int32)
    transcripts_, syls_all = chunk.transcripts, chunk.syls_all
    object_pages = [p for p in range(len(transcripts_)) if not pb.plain_page(transcripts_[p], syls_all[p])]
    for p in object_pages:
        refined[int(hres.line_first[p]):int(hres.line_first[p + 1])] = False
    # ---- the refined lines' boxes, then every page's columns with their runs replaced ------------------------------------
    qs = np.flatnonzero(refined)
    x_min, y_min, y_max = chunk.strip_geometry(qs)
    here = {int(q): frames[q][:, 0] != OMITTED for q in qs}              # the characters the path shows: all, without omit
    Lq = np.array([int(here[int(q)].sum()) for q in qs], dtype=np.int64)
    old = np.asarray(chunk.boxes, dtype=np.int64).reshape(-1, 4)
    if len(qs):
        new = peak_boxes(np.concatenate([frames[q][here[int(q)], 2] for q in qs]), Lq, T_all[qs],
                         np.asarray(chunk.widths, dtype=np.int64)[qs], x_min, y_min, y_max, ocr.PAD)
    else:
        new = np.zeros((0, 4), np.int64)
    row_of = dict(zip(qs.tolist(), (len(old) + np.concatenate([[0], np.cumsum(Lq)[:-1]])).tolist() if len(qs) else []))
    ops_r, idx_r = [], []
    for p in range(len(transcripts_)):
        mine = [(q, int(hres.table[q][1]), int(hres.table[q][2]), int(row_of[q]))
                for q in range(int(hres.line_first[p]), int(hres.line_first[p + 1])) if refined[q]]
        o, i = refine_columns(hres.ops[p], chunk.idxs[p], hres.o_line[p], mine,
                              present=None if omit_q is None else [here[ln[0]] for ln in mine])
        ops_r.append(o)
        idx_r.append(i)
    chunk.replace_columns(ops_r, idx_r, np.concatenate([old, new]))
    indices, arrays = [], []
    results = chunk.finish(indices, arrays)
    out = RefineResult(results, indices, arrays, refined, frames, score, hres, object_pages)
    out.omitted = omitted
    def pages_of(none, values):                          # per page _page_values of the refined lines' `values`
        got = []
        for p, tr in enumerate(transcripts_):
            lines = [(int(hres.table[q][1]), values[q])
                     for q in range(int(hres.line_first[p]), int(hres.line_first[p + 1])) if refined[q]]
            # (the range the glue forms a syllable's box over)
            spans = None if p in object_pages else pb.syllable_spans(tr, syls_all[p])
            got.append(_page_values(none, len(tr), indices[p], lines=lines, spans=spans))
        return [c for c, _ in got], [s for _, s in got]
    if confidence:
        out.confidence, out.rival = line_conf, line_rival
        out.char_confidence, out.syllable_confidence = pages_of(NO_CONFIDENCE, line_conf)
    if omit_confidence:
        out.confidence, out.rival = line_conf, line_rival
        out.char_confidence, _ = pages_of(NO_CONFIDENCE, line_conf)
        shown = [None if c is None else np.where(frames[q][:, 0] != OMITTED, c, NO_CONFIDENCE) for q, c in enumerate(line_conf)]
        _, out.syllable_confidence = pages_of(NO_CONFIDENCE, shown)      # a syllable: its PRESENT characters
    if posterior:
        of = lambda name: [None if lp is None else getattr(lp, name) for lp in line_post]           # noqa: E731
        out.posterior, out.rival_posterior, out.posterior_rival = of("posterior"), of("rival_posterior"), of("rival_state")
        out.loglik_bits = of("loglik_bits")
        out.char_posterior, out.syllable_posterior = pages_of(np.nan, out.posterior)
    out.columns = (ops_r, idx_r, chunk.syl_boxes)       # what the boxes were formed from, for checking the rule
    out.probs, out.row_off, out.T = st["probs"], np.asarray(st["row_start_host"])[:nlines], T_all
    return out


def page_scope_eligibility(plain, h_status, classes, table_rows, T, margin, omit=False):
    """(reason, windows) of one page for page scope: reason 0 and (lo, hi), or why not and None.  plain: its syllables are
    formed on the array path; h_status: its harvest status; classes: the class of every transcript character; table_rows,
    T: the harvest rows and timesteps of its lines.  omit: for the lattice with omission -- characters are not counted
    against frames (every page has a path), and a page beyond PAGE_MAX_CHARS / PAGE_MAX_FRAMES is PAGE_TOO_LONG."""
    n = len(classes)
    if not plain:
        return PAGE_NOT_PLAIN, None
    if h_status != 0:
        return PAGE_HARVEST, None
    if n and (np.asarray(classes) == 0).any():
        return PAGE_CLASS0, None
    if n < 1:
        return PAGE_NO_TEXT, None
    if len(T) < 1:
        return PAGE_WINDOWS, None
    w = page_windows(table_rows, n, margin)
    if w is None:
        return PAGE_WINDOWS, None
    total = int(np.asarray(T, dtype=np.int64).sum())
    if omit and (n > PAGE_MAX_CHARS or total > PAGE_MAX_FRAMES):
        return PAGE_TOO_LONG, None
    if not omit and n > total:
        return PAGE_FRAMES, None
    return PAGE_REFINED, w


def _refine_at_page_scope(hres, chunk, margin, omit_q=None, confidence=False, posterior=False):
    """refine_pages(scope="page") behind the harvest: eligibility and windows on the host, ONE ta_forced_align_pages call
    (omit_q: ta_forced_align_pages_omit at that price), the refined pages' columns replaced.  confidence: one
    ta_forced_page_confidence call behind it over the pages that have a path, the aligner's frames as queries; posterior:
    one ta_forced_page_posterior call likewise"""
    from . import harvest, page_batch as pb
    rec, st = chunk.rec, chunk.st
    nlines, npages = len(hres), len(chunk.transcripts)
    lf = np.asarray(hres.line_first, dtype=np.int64)
    T_all = np.asarray(st["T_host"], dtype=np.int64)[:nlines]
    row_all = np.asarray(st["row_start_host"], dtype=np.int64)[:nlines]
    classes = [harvest.transcript_classes(rec.model.codec, tr) for tr in chunk.transcripts]
    reason = np.zeros(npages, dtype=np.int32)
    windows = [None] * npages
    for p in range(npages):
        a, b = int(lf[p]), int(lf[p + 1])
        reason[p], windows[p] = page_scope_eligibility(pb.plain_page(chunk.transcripts[p], chunk.syls_all[p]),
                                                       int(hres.status[p]), classes[p], hres.table[a:b], T_all[a:b], margin,
                                                       omit=omit_q is not None)
    take = [p for p in range(npages) if reason[p] == PAGE_REFINED]
    page_frames, page_score, page_omitted = [None] * npages, [None] * npages, [None] * npages
    page_conf, page_rival = [None] * npages, [None] * npages
    page_post = [None] * npages
    if take:
        qs = np.concatenate([np.arange(lf[p], lf[p + 1]) for p in take])
        sizes = lambda xs: np.concatenate([[0], np.cumsum(xs)]).astype(np.int64)                    # noqa: E731
        lab_off = sizes([len(classes[p]) for p in take])
        with torch.cuda.device(rec.device):
            got = forced_page_alignment(st["probs"], row_all[qs], T_all[qs], sizes([lf[p + 1] - lf[p] for p in take]),
                                        np.concatenate([windows[p][0] for p in take]),
                                        np.concatenate([windows[p][1] for p in take]),
                                        np.concatenate([classes[p] for p in take]), lab_off, host=True, omit_q=omit_q)
        for k, p in enumerate(take):
            status = int(got["status"][k])
            if status == NOPATH:
                reason[p] = PAGE_NO_PATH
            elif status != OK:
                raise RuntimeError("ta_forced_align_pages refused page %d on the device: %s" % (p, PAGE_STATUS.get(status, "?")))
            elif omit_q is not None and (got["frames"][lab_off[k]:lab_off[k + 1], 0] == OMITTED).all():
                reason[p] = PAGE_ALL_OMITTED             # a path that holds no character refines nothing
            else:
                page_frames[p] = got["frames"][lab_off[k]:lab_off[k + 1]]
                page_score[p] = int(got["score"][k])
                page_omitted[p] = int((page_frames[p][:, 0] == OMITTED).sum())
        ok = [k for k, p in enumerate(take) if page_frames[p] is not None]
        if confidence and ok:
            pick = [take[k] for k in ok]
            qs = np.concatenate([np.arange(lf[p], lf[p + 1]) for p in pick])
            off = sizes([len(classes[p]) for p in pick])
            with torch.cuda.device(rec.device):
                m = forced_page_confidence(st["probs"], row_all[qs], T_all[qs], sizes([lf[p + 1] - lf[p] for p in pick]),
                                           np.concatenate([windows[p][0] for p in pick]),
                                           np.concatenate([windows[p][1] for p in pick]),
                                           np.concatenate([classes[p] for p in pick]), off,
                                           np.concatenate([page_frames[p] for p in pick]), host=True)
            for j, p in enumerate(pick):
                if m["status"][j] != OK:
                    raise RuntimeError("ta_forced_page_confidence refused page %d on the device: %s"
                                       % (p, PAGE_CONF_STATUS.get(int(m["status"][j]), "?")))
                page_conf[p], page_rival[p] = m["confidence"][off[j]:off[j + 1]], m["rival"][off[j]:off[j + 1]]
        if posterior and ok:
            pick = [take[k] for k in ok]
            qs = np.concatenate([np.arange(lf[p], lf[p + 1]) for p in pick])
            off = sizes([len(classes[p]) for p in pick])
            with torch.cuda.device(rec.device):
                m = forced_page_posterior(st["probs"], row_all[qs], T_all[qs], sizes([lf[p + 1] - lf[p] for p in pick]),
                                          np.concatenate([windows[p][0] for p in pick]),
                                          np.concatenate([windows[p][1] for p in pick]),
                                          np.concatenate([classes[p] for p in pick]), off,
                                          np.concatenate([page_frames[p] for p in pick]), host=True)
            for j, p in enumerate(pick):
                if m["status"][j] != OK:
                    raise RuntimeError("ta_forced_page_posterior refused page %d on the device: %s"
                                       % (p, PAGE_CONF_STATUS.get(int(m["status"][j]), "?")))
                page_post[p] = LinePosterior(m, int(off[j]), int(off[j + 1]), j)
    score = [None] * nlines
    refined, frames, ops_r, idx_r = replace_page_columns(chunk, lf, T_all, hres.ops, page_frames)
    indices, arrays = [], []
    results = chunk.finish(indices, arrays)
    object_pages = [p for p in range(npages) if reason[p] == PAGE_NOT_PLAIN]
    out = RefineResult(results, indices, arrays, refined, frames, score, hres, object_pages, page_scope=reason)
    out.page_frames, out.page_score, out.windows = page_frames, page_score, windows
    if omit_q is not None:
        out.page_omitted = page_omitted
    if confidence:
        out.page_confidence, out.page_rival = page_conf, page_rival
        out.confidence, out.rival = [None] * nlines, [None] * nlines
        out.char_confidence, out.syllable_confidence = [], []
        for p, tr in enumerate(chunk.transcripts):
            if page_conf[p] is not None:
                on = page_frames[p][:, 0]
                for q in range(int(lf[p]), int(lf[p + 1])):
                    out.confidence[q], out.rival[q] = page_conf[p][on == q - lf[p]], page_rival[p][on == q - lf[p]]
            spans = None if reason[p] == PAGE_NOT_PLAIN else pb.syllable_spans(tr, chunk.syls_all[p])
            char, syl = _page_values(NO_CONFIDENCE, len(tr), indices[p], spans=spans,
                                     lines=[] if page_conf[p] is None else [(0, page_conf[p])])
            out.char_confidence.append(char)
            out.syllable_confidence.append(syl)
    if posterior:
        of = lambda name: [None if pp is None else getattr(pp, name) for pp in page_post]           # noqa: E731
        out.page_posterior, out.page_rival_posterior = of("posterior"), of("rival_posterior")
        out.page_posterior_rival, out.page_loglik_bits = of("rival_state"), of("loglik_bits")
        out.posterior, out.rival_posterior, out.posterior_rival = [None] * nlines, [None] * nlines, [None] * nlines
        out.loglik_bits = [None] * nlines                # no likelihood per line at page scope
        out.char_posterior, out.syllable_posterior = [], []
        for p, tr in enumerate(chunk.transcripts):
            pp = page_post[p]
            if pp is not None:
                on = page_frames[p][:, 0]
                for q in range(int(lf[p]), int(lf[p + 1])):
                    here = on == q - lf[p]
                    out.posterior[q], out.rival_posterior[q] = pp.posterior[here], pp.rival_posterior[here]
                    out.posterior_rival[q] = pp.rival_state[here]
            spans = None if reason[p] == PAGE_NOT_PLAIN else pb.syllable_spans(tr, chunk.syls_all[p])
            char, syl = _page_values(np.nan, len(tr), indices[p], spans=spans, lines=[] if pp is None else [(0, pp.posterior)])
            out.char_posterior.append(char)
            out.syllable_posterior.append(syl)
    out.columns = (ops_r, idx_r, chunk.syl_boxes)
    out.probs, out.row_off, out.T = st["probs"], row_all, T_all
    return out
