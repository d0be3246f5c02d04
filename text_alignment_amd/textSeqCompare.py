"""Affine-gap Needleman-Wunsch aligner on MI355X -- drop-in for the reference module of the
same name (reference textSeqCompare.py:1-177).

    from text_alignment_amd import textSeqCompare as tsc
    tra_align, ocr_align = tsc.perform_alignment(list(transcript), list(ocr), scoring_system)

`perform_alignment` keeps the reference's signature, return value and ValueError; the DP fill
and the traceback run in the HIP kernels of csrc/ta_nw.hip through the C ABI
(`ta_nw_batch`, include/text_alignment_amd.h).  `NWBatch` is the batched form behind it: many
independent problems (pages, or one page under many scoring systems as in the reference's
parameter grid search, evaluate_text_alignment.py:178-198) in one launch.
"""
import numpy as np
import torch

from . import _native

# module attributes of the reference (textSeqCompare.py:5-10)
default_match = 10
default_mismatch = -5
gap_open = -10
gap_extend = -1          # the boundary rows always use this one (textSeqCompare.py:54-59)
default_sys = [8, -4, -7, -7, -3, 0]

GAP = '_'


def parse_scoring_system(scoring_system):
    """The three accepted forms of textSeqCompare.py:24-42.

    Returns (params, fn): params = [match, mismatch, gap_open_x, gap_open_y, gap_extend_x,
    gap_extend_y]; fn is the caller's scoring callable for the 5-element form, else None.
    """
    if scoring_system is None:
        scoring_system = default_sys
    size = len(scoring_system)
    if size == 5 and callable(scoring_system[0]):
        return [0, 0] + [scoring_system[k] for k in range(1, 5)], scoring_system[0]
    if size == 6:
        return [scoring_system[k] for k in range(6)], None
    if size == 4:
        hit, miss, opn, ext = (scoring_system[k] for k in range(4))
        return [hit, miss, opn, opn, ext, ext], None
    raise ValueError('scoring_system {} invalid'.format(scoring_system))


def _is_integral(params):
    try:
        return all(float(v) == int(v) for v in params)
    except (TypeError, ValueError, OverflowError):
        return False


def integer_scoring(scoring_system):
    """the six numbers of a scoring system as ints if the integer kernels take it, None for a scoring callable or
    non-integral numbers; an invalid system is parse_scoring_system's ValueError"""
    params, fn = parse_scoring_system(scoring_system)
    if fn is not None or not _is_integral(params):
        return None
    return [int(v) for v in params]


def encode_tokens(*seqs):
    """Dense int32 ids for arbitrary hashable tokens; equal tokens <=> equal ids
    (the aligner only ever compares tokens with ==, textSeqCompare.py:32).  Sequences of single characters -- what
    alignToOCR.py:273 passes, `list(transcript)` -- are encoded by their code points in one numpy pass; anything else
    (the bigrams of textSeqCompare.py:185-186, numbers, tuples) token by token through a dict."""
    seqs = [seq if isinstance(seq, (list, tuple, str)) else list(seq) for seq in seqs]    # an iterator is read ONCE
    try:
        if all(type(tok) is str for seq in seqs for tok in seq) and \
                all(len(seq) == 0 or max(map(len, seq)) == 1 == min(map(len, seq)) for seq in seqs):
            cps = [np.frombuffer("".join(seq).encode("utf-32-le"), dtype="<u4") for seq in seqs]
            alphabet, first = np.unique(np.concatenate(cps) if cps else np.zeros(0, "<u4"), return_index=True)
            # ids in order of first appearance, as the dict path numbers them
            rank = np.empty(len(alphabet), dtype=np.int32)
            rank[np.argsort(first, kind="stable")] = np.arange(len(alphabet), dtype=np.int32)
            out = [rank[np.searchsorted(alphabet, c)] if len(c) else np.zeros(0, np.int32) for c in cps]
            ids = {chr(int(c)): int(r) for c, r in zip(alphabet, rank)}
            return out, ids
    except (TypeError, ValueError):       # ValueError: UnicodeEncodeError -- a lone surrogate is a token like any other
        pass
    ids = {}
    out = []
    for seq in seqs:
        arr = np.empty(len(seq), dtype=np.int32)
        for k, tok in enumerate(seq):
            arr[k] = ids.setdefault(tok, len(ids))
        out.append(arr)
    return out, ids


def ops_to_alignment(ops, transcript, ocr):
    """Alignment columns (0 pair, 1 transcript token over a gap, 2 gap over an OCR token) ->
    the reference's two token lists with '_' gap markers (textSeqCompare.py:116-162).  On arrays: the token a column
    shows is the running count of the columns that consumed one."""
    ops = np.asarray(ops)
    if ops.size == 0:
        return [], []
    has_t, has_o = ops != 2, ops != 1
    t_obj = np.fromiter(transcript, dtype=object, count=len(transcript))
    o_obj = np.fromiter(ocr, dtype=object, count=len(ocr))
    tra = np.full(ops.size, GAP, dtype=object)
    oc = np.full(ops.size, GAP, dtype=object)
    tra[has_t] = t_obj[:int(has_t.sum())]
    oc[has_o] = o_obj[:int(has_o.sum())]
    return tra.tolist(), oc.tolist()


def _batch_shape(batch, t_list, o_list, params, device):
    """what NWBatch and SpanBatch hold alike: the device resolved, the problems' sizes (nprob, n, m, max_n, max_m, cells)
    and params_stride, no download under way; returns the parameter rows, int64 (1 or nprob, 6)"""
    assert len(t_list) == len(o_list)
    batch.device = torch.device(device)
    if batch.device.type == "cuda" and batch.device.index is None:
        batch.device = torch.device("cuda", torch.cuda.current_device())
    batch.nprob = len(t_list)
    batch.n = np.array([len(t) for t in t_list], dtype=np.int64)
    batch.m = np.array([len(o) for o in o_list], dtype=np.int64)
    batch.max_n = int(batch.n.max()) if batch.nprob else 0
    batch.max_m = int(batch.m.max()) if batch.nprob else 0
    batch.cells = int((batch.n * batch.m).sum())
    p = np.asarray(params, dtype=np.int64)
    if p.ndim == 1:
        p = p.reshape(1, 6)
    if p.shape[1] != 6 or p.shape[0] not in (1, batch.nprob):
        raise ValueError("params must be 6 integers, or one row of 6 per problem")
    batch.params_stride = 0 if p.shape[0] == 1 else 6
    batch._download = None                     # fetch_begin's download, until results() has taken it
    return p


class NWBatch(object):
    """A batch of independent NW problems resident in HBM.

    t_list / o_list: per-problem int32 id arrays (host).  params: one scoring system
    (6 integers) or one per problem.  All device buffers are torch tensors on `device`;
    `run()` only enqueues kernels on torch's current stream.
    """

    def __init__(self, t_list, o_list, params, device="cuda", two_phase=None, wide=None):
        p = _batch_shape(self, t_list, o_list, params, device)
        # two-phase aligner (score-only fill + chunked pointer re-derivation, csrc/ta_nw2.hip):
        # its fill is half as expensive per cell, its traceback costs ~60 us more per 256-row strip
        # of the tallest problem (one wave walks the strips one after the other), and its workspace
        # is 8x smaller.  Measured break-even on MI355X (tools/nw_breakeven.py): total cells
        # ~ 1.8e8 x strips, i.e. once the batch fills the chip about twice (re-measured after the
        # round-2 changes of both paths: tools/nw_breakeven.py).
        if two_phase is None:
            nstrips = (self.max_n + 255) // 256
            two_phase = (self.cells > 1.8e8 * nstrips) or (self.cells > 64e9) or \
                (self.max_m > _native.lib.ta_nw_max_m())       # wider than the one-pass kernel's LDS row
        self.two_phase = bool(two_phase)
        # one-pass launch shape: None = library default (a problem is spread over several
        # workgroups when the batch has fewer problems than the GPU has CUs), True / False force it
        self.wide = wide
        # two-phase launch-shape overrides (tests, A/B timing): phase 1 without the score profile;
        # phase 1 with exactly this many waves per workgroup (None = the library's own choice)
        self.no_profile = False
        self.waves = None
        # phase 2 launch shape (TA_NW_TBWAVES: 1, 2, 4 waves per problem; 3 half-strip pairs; 5, 6 pairs with 2, 4 waves;
        # None = the library's choice by batch size)
        self.tb_waves = None
        # one-pass fill: rows per lane (2 or 4; None = the library's choice by batch size)
        self.rows = None
        # two-phase fill, band around the diagonal (csrc/ta_nw2.hip): 0 = the library's rule on this
        # batch's sizes and scoring systems, 1 = off, otherwise the band's half-width (tests, tuning).  Results are the
        # same either way: a problem whose banded score does not certify the band is filled again in full.
        self.band = 0
        # the band's shape: "auto" = a funnel inside the band (narrower towards the last cell, certified at its own
        # border: csrc/nw_band.h) where the rule bands, the uniform band under a forced width; "uniform" = the uniform
        # band throughout (A/B); "funnel" = the funnel inside a forced band = w as well, even on shapes the plan would
        # decline (tests); "funnel-lcs" = the funnel with the remainder of an exit bounded by the suffix LCS of the two
        # strings and narrower widths for it (nw_lcs_suffix_kernel; per problem, where the kernel applies) -- what "auto"
        # runs wherever it runs a funnel; "funnel" keeps the static bound and its widths (A/B)
        self.band_shape = "auto"
        self._band_plan = None
        self._params_host = np.ascontiguousarray(p, dtype=np.int32)
        pmax = int(np.abs(p).max()) if p.size else 0
        self.score_bound = (self.max_n + self.max_m + 2) * (3 * pmax + 2)
        if np.abs(p).max(initial=0) > 2 ** 20:
            raise OverflowError("scoring parameters too large for the integer kernels")
        if self.score_bound >= 2 ** 23:
            raise OverflowError("(n+m+2)*max|param| does not fit the 32-bit encoded scores")
        if self.max_m > (_native.lib.ta_nw2_max_m() if self.two_phase else _native.lib.ta_nw_max_m()):
            raise OverflowError("OCR string longer than the integer kernels take")

        lib = _native.lib
        t_off = np.zeros(self.nprob + 1, dtype=np.int64); np.cumsum(self.n, out=t_off[1:])
        o_off = np.zeros(self.nprob + 1, dtype=np.int64); np.cumsum(self.m, out=o_off[1:])
        ws_fn = lib.ta_nw2_workspace_bytes if self.two_phase else lib.ta_nw_workspace_bytes
        ws_sizes = np.array([ws_fn(int(a), int(b)) for a, b in zip(self.n, self.m)], dtype=np.int64)
        ws_off = np.zeros(self.nprob + 1, dtype=np.int64); np.cumsum(ws_sizes, out=ws_off[1:])
        self.ws_bytes = int(ws_off[-1])
        cap = self.n + self.m
        ops_off = np.zeros(self.nprob + 1, dtype=np.int64); np.cumsum(cap, out=ops_off[1:])
        self.ops_off_host = ops_off
        self.cap_host = cap

        cat_t = np.concatenate(t_list) if self.nprob and t_off[-1] else np.zeros(1, np.int32)
        cat_o = np.concatenate(o_list) if self.nprob and o_off[-1] else np.zeros(1, np.int32)
        if (cat_t.max(initial=0) >= 65535) or (cat_o.max(initial=0) >= 65535):
            raise OverflowError("more than 65534 distinct tokens in one batch")
        max_code = int(max(cat_t.max(initial=0), cat_o.max(initial=0)))
        self.codes8 = bool(max_code < 255)
        # hints for phase 1 of the two-phase aligner (include/text_alignment_amd.h): with a small
        # alphabet, byte-sized substitution scores and no free gap opens it keeps a score profile
        # in LDS instead of comparing token ids per cell
        self.hints = 0
        if p.size:
            sub = p[:, :2] - p[:, 4:5] - p[:, 5:6]
            if max_code < 254 and (p[:, 2:4] <= 0).all() and (np.abs(sub) <= 127).all():
                self.hints |= (max_code + 1) << _native.TA_NW_ALPHABET_SHIFT
            if (p[:, 2] == p[:, 3]).all():
                self.hints |= _native.TA_NW_OPENS_SAME
        (self.t_codes, self.o_codes, self.t_off, self.o_off, self.params, self.ws_off, self.ops_off) = _native.upload_packed(
            [cat_t.astype(np.int32), cat_o.astype(np.int32), t_off, o_off, p.astype(np.int32),
             ws_off[:-1].copy() if self.nprob else ws_off, ops_off[:-1].copy() if self.nprob else ops_off], self.device)
        self.ws = torch.empty(max(self.ws_bytes, 16), dtype=torch.uint8, device=self.device)
        self.ops = torch.empty(max(int(ops_off[-1]), 16), dtype=torch.uint8, device=self.device)
        self.ops_len = torch.zeros(max(self.nprob, 1), dtype=torch.int32, device=self.device)
        if self.two_phase and self.nprob:
            self.band_plan()                       # the bounds go up with the rest of the batch, not in the first run()

    def run(self, fill=True, traceback=True):
        if self.nprob == 0:
            return
        flags = (_native.TA_NW_FILL if fill else 0) | (_native.TA_NW_TRACEBACK if traceback else 0)
        if self.codes8:
            flags |= _native.TA_NW_CODES8
        if self.two_phase:
            flags |= self.phase1_flags()
        if self.wide is not None and not self.two_phase:
            flags |= _native.TA_NW_WIDE if self.wide else _native.TA_NW_NARROW
        if self.rows and not self.two_phase:
            flags |= (int(self.rows) & 0x7) << _native.TA_NW_ROWS_SHIFT
        stream = torch.cuda.current_stream(self.device).cuda_stream
        args = (self.t_codes.data_ptr(), self.t_off.data_ptr(),
                self.o_codes.data_ptr(), self.o_off.data_ptr(), self.nprob,
                self.params.data_ptr(), self.params_stride,
                self.ws.data_ptr(), self.ws_off.data_ptr(),
                self.ops.data_ptr(), self.ops_off.data_ptr(), self.ops_len.data_ptr(),
                self.max_n, self.max_m, self.score_bound, flags)
        if self.two_phase:
            plan = self.band_plan(flags)
            if plan["w"] > 0 and plan["shape"] == "funnel":
                rc = _native.lib.ta_nw2_batch_funnel_lcs(*args, plan["w"], plan["u_dev"].data_ptr(), plan["ok_dev"].data_ptr(),
                                                         plan["x0_dev"].data_ptr(), plan["cert_dev"].data_ptr(),
                                                         plan["lcs_dev"].data_ptr() if plan["lcs"] else None, stream)
            elif plan["w"] > 0:
                rc = _native.lib.ta_nw2_batch_band(*args, plan["w"], plan["u_dev"].data_ptr(), plan["ok_dev"].data_ptr(), stream)
            else:
                rc = _native.lib.ta_nw2_batch(*args, stream)
        else:
            rc = _native.lib.ta_nw_batch(*args, stream)
        _native.check(rc, "ta_nw2_batch" if self.two_phase else "ta_nw_batch")

    def band_plan(self, flags=None):
        """The band the two-phase fill of this batch runs under (ta_nw2_band_plan on the batch's own sizes and scoring
        systems -- a pure function of what the batch was built from, worked out once with the batch and again only when
        `band` or the launch-shape flags are changed, never from an earlier run's outcome): w (0: no band, today's fill), rule_w (the rule's
        width, -1: none), share (of the largest problem's groups the band runs), ranges ((first, end) group per strip
        of the largest problem), largest (its index), u (the bound per problem, host), shape ("funnel" or "uniform":
        band_shape applied to this plan; share and ranges are the shape's), uniform_share (the uniform band's share),
        x0 (funnel: the host part of the exit bound per problem), lcs (funnel: True if the LCS-bounded funnel runs
        where its kernel applies -- share and ranges are then its narrower ones for the largest problem when it is covered,
        static_share the static funnel's)."""
        if self.band_shape not in ("auto", "uniform", "funnel", "funnel-lcs"):
            raise ValueError("band_shape must be 'auto', 'uniform', 'funnel' or 'funnel-lcs'")
        if flags is None:
            flags = (_native.TA_NW_CODES8 if self.codes8 else 0) | self.phase1_flags()
        key = (int(self.band), int(flags) & ~(_native.TA_NW_FILL | _native.TA_NW_TRACEBACK), self.band_shape)
        if self._band_plan is not None and self._band_plan["key"] == key:
            return self._band_plan
        n32, m32 = self.n.astype(np.int32), self.m.astype(np.int32)
        out = np.zeros(8, dtype=np.int32)
        u = np.zeros(max(self.nprob, 1), dtype=np.int32)
        ranges = np.zeros(2 * ((self.max_n + 255) // 256 + 1), dtype=np.int32)
        rc = _native.lib.ta_nw2_band_plan(n32.ctypes.data, m32.ctypes.data, self.nprob, self._params_host.ctypes.data,
                                          self.params_stride, key[1], key[0], out.ctypes.data, u.ctypes.data,
                                          ranges.ctypes.data, len(ranges))
        _native.check(rc, "ta_nw2_band_plan")
        plan = {"key": key, "w": int(out[0]), "rule_w": int(out[1]), "share": out[2] / 1000.0, "largest": int(out[4]),
                "ranges": [(int(ranges[2 * k]), int(ranges[2 * k + 1])) for k in range(int(out[3]))], "u": u,
                "shape": "uniform"}
        funnel = plan["w"] > 0 and (self.band_shape in ("funnel", "funnel-lcs") or (self.band_shape == "auto" and out[5] == 1))
        if plan["w"] > 0:
            # the uniform band's figures for the same width (the plan reports the funnel's when it chose one)
            uni = np.zeros(len(ranges), dtype=np.int32)
            out_u = np.zeros(8, dtype=np.int32)
            rc = _native.lib.ta_nw2_band_plan(n32.ctypes.data, m32.ctypes.data, self.nprob, self._params_host.ctypes.data,
                                              self.params_stride, key[1], plan["w"], out_u.ctypes.data, None,
                                              uni.ctypes.data, len(uni))
            _native.check(rc, "ta_nw2_band_plan")
            plan["uniform_share"] = out_u[2] / 1000.0
            if not funnel:
                plan["share"] = plan["uniform_share"]
                plan["ranges"] = [(int(uni[2 * k]), int(uni[2 * k + 1])) for k in range(int(out[3]))]
        if funnel:
            x0 = np.zeros(max(self.nprob, 1), dtype=np.int32)
            fout = np.zeros(4, dtype=np.int32)
            rc = _native.lib.ta_nw2_funnel_plan(n32.ctypes.data, m32.ctypes.data, self.nprob, self._params_host.ctypes.data,
                                                self.params_stride, plan["w"], plan["largest"], x0.ctypes.data,
                                                ranges.ctypes.data, len(ranges), fout.ctypes.data)
            _native.check(rc, "ta_nw2_funnel_plan")
            plan.update(shape="funnel", x0=x0, share=fout[1] / 1000.0, funnel_own_ranges=bool(fout[0]),
                        ranges=[(int(ranges[2 * k]), int(ranges[2 * k + 1])) for k in range(int(out[3]))], lcs=False)
            alphabet = (int(flags) >> _native.TA_NW_ALPHABET_SHIFT) & 0xFF
            if self.band_shape != "funnel" and 0 < alphabet <= 64:
                plan["lcs"] = True
                plan["static_share"] = plan["share"]
                big = plan["largest"]
                prm_big = np.ascontiguousarray(self._params_host[big if self.params_stride else 0])
                if m32[big] <= _native.lib.ta_nw2_funnel_lcs_max_m() and prm_big[0] > prm_big[1]:
                    rc = _native.lib.ta_nw2_funnel_ranges(int(n32[big]), int(m32[big]), prm_big.ctypes.data, plan["w"],
                                                          _native.lib.ta_nw2_funnel_lcs_scale_pm(), ranges.ctypes.data,
                                                          len(ranges), fout.ctypes.data)
                    _native.check(rc, "ta_nw2_funnel_ranges")
                    if fout[0]:
                        plan.update(share=fout[1] / 1000.0,
                                    ranges=[(int(ranges[2 * k]), int(ranges[2 * k + 1])) for k in range(int(out[3]))])
        if plan["w"] > 0:
            (plan["u_dev"],) = _native.upload_packed([u], self.device)
            plan["ok_dev"] = torch.zeros(self.nprob, dtype=torch.int32, device=self.device)
            if funnel:
                (plan["x0_dev"],) = _native.upload_packed([plan["x0"]], self.device)
                plan["cert_dev"] = torch.zeros(4 * self.nprob, dtype=torch.int32, device=self.device)
                if plan["lcs"]:
                    words = int(_native.lib.ta_nw2_funnel_lcs_words(self.nprob, self.max_n))
                    plan["lcs_dev"] = torch.empty(max(words, 16), dtype=torch.int32, device=self.device)
        self._band_plan = plan
        return plan

    def band_fallbacks(self):
        """indices of the problems the last banded fill had to fill again in full (their certificate failed), sorted;
        empty without a band.  Synchronises: for tests and reports, not for timed code."""
        plan = self._band_plan
        if not self.two_phase or plan is None or plan["w"] <= 0:
            return []
        return [int(k) for k in np.nonzero(plan["ok_dev"].cpu().numpy() == 0)[0]]

    def band_certificate(self):
        """The funnel's certificate of the last fill, (nprob, 3) int32: v0 (the banded score of the walk's start), the exit
        maximum (no alignment that leaves the region scores more) and the strips counted, per problem; None without a
        funnel.  Synchronises: for tests and reports, not for timed code."""
        plan = self._band_plan
        if not self.two_phase or plan is None or plan["w"] <= 0 or plan["shape"] != "funnel":
            return None
        return plan["cert_dev"].cpu().numpy().reshape(self.nprob, 4)[:, :3]    # (the fourth word: the ranges' source)

    def phase1_flags(self):
        """Hint and override bits of a ta_nw2_batch / ta_nw2_phase1_plan_batch call for this batch."""
        flags = self.hints
        if getattr(self, "check_ids", False):        # debug guard: the library verifies the id bounds the hints assert
            flags |= _native.TA_NW_CHECK_IDS
        if self.no_profile:
            flags |= _native.TA_NW_NO_PROFILE
        if self.waves:
            flags |= (int(self.waves) & 0xF) << _native.TA_NW_WAVES_SHIFT
        if self.tb_waves:
            flags |= (int(self.tb_waves) & 0x7) << _native.TA_NW_TBWAVES_SHIFT
        return flags

    def traceback_kernel(self):
        """name of the traceback kernel run() launches for this batch (bench / profile labels)"""
        if not self.two_phase:
            return "nw_traceback_kernel"
        w = _native.lib.ta_nw2_traceback_plan(self.nprob, self.params_stride, self.phase1_flags())
        return {1: "nw_trace2_kernel", 2: "nw_trace2w_kernel<2>", 4: "nw_trace2w_kernel<4>", 3: "nw_trace2h_kernel",
                5: "nw_trace2hw_kernel<2>", 6: "nw_trace2hw_kernel<4>"}[w]

    def fetch_begin(self):
        """start the download of the alignment columns (_native.download_begin); `results()` then only waits for its
        event -- a caller with other host work puts it in between"""
        if self.nprob:
            self._download = _native.download_begin([self.ops, self.ops_len])

    def results(self, waiter=None):
        """Host copies of the alignment columns, one uint8 array per problem.  waiter: see _native.Download.wait."""
        if self.nprob == 0:
            return []
        if self._download is not None:
            (ops, lens), self._download = self._download.wait(waiter), None
        else:
            ops = self.ops.cpu().numpy()
            lens = self.ops_len.cpu().numpy()
        if (lens[:self.nprob] < 0).any():         # ta_nw2_batch resets the lengths to -1 before its traceback launch
            raise RuntimeError("traceback of problem %d did not finish (a bounded wait between its waves ran out)"
                               % int(np.nonzero(lens[:self.nprob] < 0)[0][0]))
        out = []
        for k in range(self.nprob):
            end = int(self.ops_off_host[k] + self.cap_host[k])
            out.append(ops[end - int(lens[k]):end].copy())
        return out


class SpanBatch(object):
    """A batch of span searches resident in HBM: where in transcript t does the text o lie (csrc/ta_nw_span.hip;
    DESIGN.md section 4.6)?  Works like NWBatch: t_list / o_list are per-problem int32 id arrays (host), params one
    scoring system (6 integers) or one per problem; `run()` only enqueues; `fetch_begin()` / `results()` give an
    (nprob, 3) int32 array of (i0, i1, score).  An array OBJECT that appears more than once in t_list -- the book every
    page of a chunk is searched in -- is uploaded once."""

    def __init__(self, t_list, o_list, params, device="cuda"):
        p = _batch_shape(self, t_list, o_list, params, device)
        lib = _native.lib
        self.max_param = int(np.abs(p).max()) if p.size else 0
        self.score_bound = (self.max_n + self.max_m + 2) * (3 * self.max_param + 2)
        if self.max_param > 2 ** 19:
            raise OverflowError("scoring parameters too large for the span fill")
        if self.score_bound >= 2 ** 23:
            raise OverflowError("(n+m+2)*max|param| does not fit the span fill's 24-bit scores")
        if self.max_m > lib.ta_nw_span_max_m():
            raise OverflowError("OCR string longer than the span fill takes (%d)" % lib.ta_nw_span_max_m())
        if self.max_n >= 2 ** 28:
            raise OverflowError("transcript longer than the span fill's origin field (2^28 - 1)")
        # every distinct transcript OBJECT once
        start_of, pieces, total = {}, [], 0
        t_start = np.zeros(self.nprob, dtype=np.int64)
        for k, t in enumerate(t_list):
            if id(t) not in start_of:
                start_of[id(t)] = total
                pieces.append(np.asarray(t, dtype=np.int32))
                total += len(t)
            t_start[k] = start_of[id(t)]
        self.uploaded_tokens = total
        o_off = np.zeros(self.nprob + 1, dtype=np.int64); np.cumsum(self.m, out=o_off[1:])
        cat_t = np.concatenate(pieces) if total else np.zeros(1, np.int32)
        cat_o = np.concatenate(o_list).astype(np.int32) if self.nprob and o_off[-1] else np.zeros(1, np.int32)
        if cat_t.min(initial=0) < 0 or cat_o.min(initial=0) < 0 or \
                cat_t.max(initial=0) >= 65535 or cat_o.max(initial=0) >= 65535:
            raise OverflowError("token ids must lie in 0 .. 65534")
        (self.t_codes, self.o_codes, self.t_start, self.t_len, self.o_off, self.params) = _native.upload_packed(
            [cat_t, cat_o, t_start, self.n.astype(np.int32), o_off, p.astype(np.int32)], self.device)
        self.ws_bytes = int(lib.ta_nw_span_workspace_bytes(self.nprob, self.max_n, self.max_m))
        if self.ws_bytes < 0:
            raise OverflowError("batch beyond the span fill's limits")
        self.ws = torch.empty(max(self.ws_bytes, 16), dtype=torch.uint8, device=self.device)
        self.out = torch.empty((max(self.nprob, 1), 3), dtype=torch.int32, device=self.device)

    def run(self):
        if self.nprob == 0:
            return
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = _native.lib.ta_nw_span_batch(
            self.t_codes.data_ptr(), self.t_start.data_ptr(), self.t_len.data_ptr(),
            self.o_codes.data_ptr(), self.o_off.data_ptr(), self.nprob,
            self.params.data_ptr(), self.params_stride, self.out.data_ptr(),
            self.max_n, self.max_m, self.score_bound, self.max_param,
            self.ws.data_ptr(), self.ws_bytes, stream)
        _native.check(rc, "ta_nw_span_batch")

    def fetch_begin(self):
        """start the download of the spans (_native.download_begin); `results()` then only waits for its event"""
        if self.nprob:
            self._download = _native.download_begin([self.out])

    def results(self, waiter=None):
        """(nprob, 3) int32: i0, i1, score per problem -- t[i0:i1] is what the global aligner is then given.  waiter: see
        _native.Download.wait."""
        if self.nprob == 0:
            return np.zeros((0, 3), dtype=np.int32)
        if self._download is not None:
            (out,), self._download = self._download.wait(waiter), None
            out = out[:self.nprob].copy()
        else:
            out = self.out.cpu().numpy()[:self.nprob]
        if (out[:, 1] < 0).any():
            raise OverflowError("span fill refused problem %d: scoring parameters beyond its limits"
                                % int(np.nonzero(out[:, 1] < 0)[0][0]))
        return out


def _span_systems(scoring_systems, count):
    """one scoring system for all, or one per pair -> int64 (1 or count, 6); callables and non-integral numbers are a
    ValueError (the span fill is an integer kernel and there is no other)"""
    if scoring_systems is None or not isinstance(scoring_systems, (list, tuple)) or \
            (len(scoring_systems) in (4, 6) and not isinstance(scoring_systems[0], (list, tuple, np.ndarray))) or \
            (len(scoring_systems) == 5 and callable(scoring_systems[0])):
        systems = [scoring_systems]
    else:
        systems = list(scoring_systems)
        if len(systems) != count:
            raise ValueError("need one scoring system per pair")
    rows = []
    for s in systems:
        params = integer_scoring(s)
        if params is None:
            raise ValueError("locate_span takes integer match/mismatch scoring systems only, got {}".format(s))
        rows.append(params)
    return np.array(rows, dtype=np.int64).reshape(-1, 6)


def locate_spans(pairs, scoring_systems=None):
    """[(i0, i1, score)] per (transcript, ocr) token-list pair: transcript[i0:i1] is the part of the transcript that the
    OCR text covers (ends free on the transcript side), in one launch.  scoring_systems as in
    perform_alignment_batch, integer forms only (ValueError otherwise).  A transcript OBJECT shared by several pairs is
    encoded and uploaded once."""
    pairs = [(t if isinstance(t, (list, tuple, str)) else list(t), o if isinstance(o, (list, tuple, str)) else list(o))
             for t, o in pairs]
    params = _span_systems(scoring_systems, len(pairs))
    _require_gpu()
    if not pairs:
        return []
    distinct = {}
    for t, _ in pairs:
        distinct.setdefault(id(t), t)
    keys = list(distinct)
    codes, _ = encode_tokens(*([distinct[k] for k in keys] + [o for _, o in pairs]))
    t_of = dict(zip(keys, codes[:len(keys)]))
    batch = SpanBatch([t_of[id(t)] for t, _ in pairs], codes[len(keys):], params)
    batch.run()
    return [tuple(int(v) for v in row) for row in batch.results()]


def locate_span(transcript, ocr, scoring_system=None):
    """(i0, i1, score): where in `transcript` the text `ocr` lies -- see locate_spans"""
    params = integer_scoring(scoring_system)               # raises ValueError like perform_alignment
    if params is None:
        raise ValueError("locate_span takes integer match/mismatch scoring systems only, got {}".format(scoring_system))
    return locate_spans([(list(transcript), list(ocr))], params)[0]


class SpanChainBatch(object):
    """Chained span searches resident in HBM: the pages of a book IN READING ORDER in one transcript
    (ta_nw_span_chain, csrc/ta_nw_span.hip).  Works like SpanBatch: t_list holds one int32 id
    array per CHAIN, o_lists one list of id arrays per chain (its pages in order), params one scoring system (6
    integers) or one per chain; `run()` only enqueues; `fetch_begin()` / `results()` give an (npages, 3) int32 array of
    (i0, i1, score), the pages of all chains one after the other with chain c's at page_first[c] .. page_first[c+1],
    and an (nchains,) int64 array of totals.  An array OBJECT that appears more than once in t_list is uploaded once.
    floor: the clamp of the carry, by default the call's score_bound."""

    def __init__(self, t_list, o_lists, params, device="cuda", floor=None):
        assert len(t_list) == len(o_lists)
        o_list = [o for pages in o_lists for o in pages]
        self.nchains = len(t_list)
        self.pages = np.array([len(pages) for pages in o_lists], dtype=np.int32)
        self.page_first = np.zeros(self.nchains + 1, dtype=np.int32); np.cumsum(self.pages, out=self.page_first[1:])
        page_chain = np.repeat(np.arange(self.nchains), self.pages)
        p = np.asarray(params, dtype=np.int64)
        if p.size == 0 or p.size % 6:
            raise ValueError("params must be 6 integers, or one row of 6 per chain")
        p = p.reshape(-1, 6)
        _batch_shape(self, [t_list[c] for c in page_chain], o_list, p[0], device)      # sizes per PAGE: n, m, cells
        self.npages = self.nprob
        self.max_n = max([len(t) for t in t_list] + [0])             # (a chain without pages still has a transcript)
        if p.shape[0] not in (1, self.nchains):
            raise ValueError("params must be 6 integers, or one row of 6 per chain")
        self.params_stride = 0 if p.shape[0] == 1 else 6
        lib = _native.lib
        self.max_param = int(np.abs(p).max()) if p.size else 0
        self.score_bound = (self.max_n + self.max_m + 2) * (3 * self.max_param + 2)
        self.floor = int(self.score_bound if floor is None else floor)
        if self.max_param > 2 ** 19:
            raise OverflowError("scoring parameters too large for the span fill")
        if self.floor <= 0:
            raise ValueError("the carry's floor must be positive")
        if self.score_bound + self.floor >= 2 ** 23:
            raise OverflowError("(n+m+2)*max|param| + floor does not fit the span fill's 24-bit scores")
        if self.max_m > lib.ta_nw_span_max_m():
            raise OverflowError("OCR string longer than the span fill takes (%d)" % lib.ta_nw_span_max_m())
        if self.max_n >= 2 ** 28:
            raise OverflowError("transcript longer than the span fill's origin field (2^28 - 1)")
        start_of, pieces, total = {}, [], 0                           # every distinct transcript OBJECT once
        t_start = np.zeros(self.nchains, dtype=np.int64)
        for k, t in enumerate(t_list):
            if id(t) not in start_of:
                start_of[id(t)] = total
                pieces.append(np.asarray(t, dtype=np.int32))
                total += len(t)
            t_start[k] = start_of[id(t)]
        self.uploaded_tokens = total
        t_len = np.array([len(t) for t in t_list], dtype=np.int32)
        o_off = np.zeros(self.npages + 1, dtype=np.int64); np.cumsum(self.m, out=o_off[1:])
        cat_t = np.concatenate(pieces) if total else np.zeros(1, np.int32)
        cat_o = np.concatenate(o_list).astype(np.int32) if self.npages and o_off[-1] else np.zeros(1, np.int32)
        if cat_t.min(initial=0) < 0 or cat_o.min(initial=0) < 0 or \
                cat_t.max(initial=0) >= 65535 or cat_o.max(initial=0) >= 65535:
            raise OverflowError("token ids must lie in 0 .. 65534")
        (self.t_codes, self.o_codes, self.t_start, self.t_len, self.o_off, self.d_page_first,
         self.params) = _native.upload_packed(
            [cat_t, cat_o, t_start, t_len, o_off, self.page_first, p.astype(np.int32)], self.device)
        self.ws_bytes = int(lib.ta_nw_span_chain_workspace_bytes(self.nchains, self.npages, self.max_n))
        if self.ws_bytes < 0:
            raise OverflowError("batch beyond the span fill's limits")
        self.ws = torch.empty(max(self.ws_bytes, 16), dtype=torch.uint8, device=self.device)
        self.out = torch.empty((max(self.npages, 1), 3), dtype=torch.int32, device=self.device)
        self.total = torch.empty(max(self.nchains, 1), dtype=torch.int64, device=self.device)

    def run(self):
        if self.nchains == 0:
            return
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = _native.lib.ta_nw_span_chain(
            self.t_codes.data_ptr(), self.t_start.data_ptr(), self.t_len.data_ptr(),
            self.o_codes.data_ptr(), self.o_off.data_ptr(), self.d_page_first.data_ptr(),
            self.nchains, self.npages, self.pages.ctypes.data,
            self.params.data_ptr(), self.params_stride, self.floor, self.out.data_ptr(), self.total.data_ptr(),
            self.max_n, self.max_m, self.score_bound, self.max_param,
            self.ws.data_ptr(), self.ws_bytes, stream)
        _native.check(rc, "ta_nw_span_chain")

    def fetch_begin(self):
        """start the download of the spans and totals (_native.download_begin); `results()` then only waits for its event"""
        if self.nchains:
            self._download = _native.download_begin([self.out, self.total])

    def results(self, waiter=None):
        """((npages, 3) int32: i0, i1, score per page; (nchains,) int64: the chains' totals).  waiter: see
        _native.Download.wait."""
        if self.nchains == 0:
            return np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.int64)
        if self._download is not None:
            (out, total), self._download = self._download.wait(waiter), None
            out, total = out[:self.npages].copy(), total[:self.nchains].copy()
        else:
            out, total = self.out.cpu().numpy()[:self.npages], self.total.cpu().numpy()[:self.nchains]
        if (total == np.iinfo(np.int64).min).any():
            raise OverflowError("span fill refused chain %d: sizes or scoring parameters beyond its limits"
                                % int(np.nonzero(total == np.iinfo(np.int64).min)[0][0]))
        return out, total


def locate_chains(books, scoring_systems=None):
    """[(spans, total)] per book (transcript, [ocr_0, ocr_1, ...]) of token lists, the OCR texts being the book's pages
    IN READING ORDER: spans = [(i0, i1, score)] per page with i1 of a page <= i0 of the next, total = the sum of the
    scores.  Where locate_spans searches every page on its own -- and puts a passage the book repeats on its first
    copy -- this is one chained search per book.  scoring_systems: one for all or one per
    book, integer forms only (ValueError otherwise); OverflowError for what the fill's limits refuse.  A transcript
    OBJECT shared by several books is encoded and uploaded once."""
    books = [(t if isinstance(t, (list, tuple, str)) else list(t),
              [o if isinstance(o, (list, tuple, str)) else list(o) for o in pages]) for t, pages in books]
    params = _span_systems(scoring_systems, len(books))
    _require_gpu()
    if not books:
        return []
    distinct = {}
    for t, _ in books:
        distinct.setdefault(id(t), t)
    keys = list(distinct)
    codes, _ = encode_tokens(*([distinct[k] for k in keys] + [o for _, pages in books for o in pages]))
    t_of = dict(zip(keys, codes[:len(keys)]))
    o_codes, o_lists = codes[len(keys):], []
    for _, pages in books:
        o_lists.append(o_codes[:len(pages)])
        o_codes = o_codes[len(pages):]
    batch = SpanChainBatch([t_of[id(t)] for t, _ in books], o_lists, params)
    batch.run()
    out, total = batch.results()
    first = batch.page_first
    return [([tuple(int(v) for v in row) for row in out[first[c]:first[c + 1]]], int(total[c]))
            for c in range(len(books))]


def locate_chain(transcript, ocr_texts, scoring_system=None):
    """(spans, total): where in `transcript` the texts of a book's pages lie, in reading order -- see locate_chains"""
    params = integer_scoring(scoring_system)               # raises ValueError like perform_alignment
    if params is None:
        raise ValueError("locate_chain takes integer match/mismatch scoring systems only, got {}".format(scoring_system))
    return locate_chains([(list(transcript), [list(o) for o in ocr_texts])], params)[0]


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("text_alignment_amd needs an AMD GPU (MI355X): torch.cuda.is_available() "
                           "is False and there is no CPU fallback")


def perform_alignment_batch(pairs, scoring_systems=None):
    """Align many (transcript, ocr) token-list pairs in one launch.

    scoring_systems: None, one scoring system for all, or a list with one per pair (integer
    match/mismatch forms only).  Returns a list of (tra_align, ocr_align).
    """
    _require_gpu()
    pairs = [(list(t), list(o)) for t, o in pairs]
    if scoring_systems is None or not isinstance(scoring_systems, (list, tuple)) or \
            (len(scoring_systems) in (4, 6) and not isinstance(scoring_systems[0], (list, tuple, np.ndarray))) or \
            (len(scoring_systems) == 5 and callable(scoring_systems[0])):
        systems = [scoring_systems] * len(pairs)
    else:
        systems = list(scoring_systems)
        if len(systems) != len(pairs):
            raise ValueError("need one scoring system per pair")
    parsed = [parse_scoring_system(s) for s in systems]
    if any(fn is not None for _, fn in parsed):      # a scoring callable: its table is per pair
        return [perform_alignment(t, o, s) for (t, o), s in zip(pairs, systems)]
    t_list, o_list = [], []
    for t, o in pairs:
        (ti, oi), _ = encode_tokens(t, o)
        t_list.append(ti); o_list.append(oi)
    all_ops = None
    if all(_is_integral(p) for p, _ in parsed):
        params = np.array([[int(v) for v in p] for p, _ in parsed], dtype=np.int64)
        if len(pairs) and (params == params[0]).all():
            params = params[:1]
        try:
            batch = NWBatch(t_list, o_list, params)
            batch.run()
            all_ops = batch.results()
        except OverflowError:       # beyond the 32-bit kernels' limits: the float64 kernel below
            pass
    if all_ops is None:             # non-integral numbers (or too large): float64 kernel, still one launch
        from . import nw_general
        all_ops = nw_general.align_batch(t_list, o_list, [[float(v) for v in p] for p, _ in parsed])
    return [ops_to_alignment(ops, t, o) for ops, (t, o) in zip(all_ops, pairs)]


def perform_alignment(transcript, ocr, scoring_system=None, verbose=False):
    '''
    @scoring_system must be array-like, of one of the following forms:
    [match_func(a,b), gap_open_x, gap_open_y, gap_extend_x, gap_extend_y]
    [match, mismatch, gap_open_x, gap_open_y, gap_extend_x, gap_extend_y]
    [match, mismatch, gap_open, gap_extend]

    Returns (tra_align, ocr_align): two equal-length token lists with '_' where the other
    sequence has no partner (reference textSeqCompare.py:13, :177).  Inputs are not mutated.
    '''
    params, fn = parse_scoring_system(scoring_system)      # raises ValueError like the reference
    _require_gpu()
    transcript = list(transcript)
    ocr = list(ocr)
    (t_ids, o_ids), ids = encode_tokens(transcript, ocr)
    if fn is None and _is_integral(params):
        try:
            batch = NWBatch([t_ids], [o_ids], [int(v) for v in params])
            batch.run()
            ops = batch.results()[0]
        except OverflowError:       # scores would not fit the 32-bit encoding: float64 kernel
            ops = _general_alignment(t_ids, o_ids, ids, params, fn)
    else:
        ops = _general_alignment(t_ids, o_ids, ids, params, fn)
    tra_align, ocr_align = ops_to_alignment(ops, transcript, ocr)
    if verbose:
        for a, b in zip(tra_align, ocr_align):
            mark = ' ' if (a == GAP or b == GAP) else ('O' if a == b else '~')
            print('{} {} {}'.format(a, b, mark))
    return (tra_align, ocr_align)


def _general_alignment(t_ids, o_ids, ids, params, fn):
    """float64 / substitution-table kernel for callable or non-integral scoring systems."""
    from . import nw_general
    return nw_general.align(t_ids, o_ids, ids, params, fn)
