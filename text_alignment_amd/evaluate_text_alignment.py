# -*- coding: utf-8 -*-
"""Scoring of syllable boxes against hand-drawn ground truth, and the scoring-system sweep -- the reference module of
the same name (reference evaluate_text_alignment.py:1-198).

    from text_alignment_amd import evaluate_text_alignment as eta
    pages = [eta.SweepPage.from_image(raw, transcript, load_ocr_pickle(pik), eta.read_gt_boxes(xml)) for ...]
    res = eta.sweep(pages)                  # all 729 scoring systems of the reference's grid, one call
    res.ranking()[-1]                       # the best system and its mean black-area IOU

Host semantics (`intersect`, `IOU`, `black_area_IOU`, `read_gt_boxes`, `score_alignment`, `evaluate_alignment`) keep
the reference's arithmetic and its quirks; `score_alignment` is the product's cross-check of the device path.
`sweep` runs the whole grid search: ONE NWBatch of pages x systems problems, then three kernels on the same stream
(csrc/ta_eval.hip: summed-area tables of the ink planes, syllable boxes read from the alignment columns where the
traceback left them, scores per (problem, ground-truth box)) and one download of the per-box results.

Black pixels: Gamera's `subimage(ul, lr)` includes the `lr` row and column, so a black-pixel count here covers
ul.x..lr.x x ul.y..lr.y inclusive, while `IOU`'s areas are the exclusive (lr - ul) products, as the reference mixes
them.  Gamera is not available to this project, so the inclusive reading is taken from Gamera's documented view
semantics and cannot be checked against it (deviations).  A rectangle that is not inside the page raises
RuntimeError, as Gamera's view constructor does.
"""
import itertools
import json
import os
import xml.etree.ElementTree as ET

import numpy as np

from . import _native
from . import latinSyllabification as latsyl
from . import page as page_mod
from . import page_batch
from . import textSeqCompare as tsc

# the reference's grid (evaluate_text_alignment.py:181-188)
GRID = ([5, 8, 11], [-4, -7, -10], [-2, -5, -7], [-2, -5, -7], [0, -3, -5], [0, -3, -5])

STATUS_NAMES = {_native.TA_EVAL_OK: "ok", _native.TA_EVAL_UNFINISHED: "traceback unfinished",
                _native.TA_EVAL_MISMATCH: "alignment disagrees with the page", _native.TA_EVAL_OUT_OF_RANGE:
                "rectangle outside the page", _native.TA_EVAL_ZERO_AREA: "zero black-area denominator"}


# ------------------------------------------------------------------------------------------------ host semantics
def intersect(bb1, bb2):
    '''area of the overlap of two boxes, or False if they do not overlap (reference :16-30)'''
    lr1, ul1, lr2, ul2 = bb1['lr'], bb1['ul'], bb2['lr'], bb2['ul']
    dx = min(lr1[0], lr2[0]) - max(ul1[0], ul2[0])
    dy = min(lr1[1], lr2[1]) - max(ul1[1], ul2[1])
    if (dx > 0) and (dy > 0):
        return dx * dy
    return False


def IOU(bb1, bb2):
    '''intersection over union of two boxes, exclusive (lr - ul) areas (reference :33-52)'''
    lr1, ul1, lr2, ul2 = bb1['lr'], bb1['ul'], bb2['lr'], bb2['ul']
    area_int = (min(lr1[0], lr2[0]) - max(ul1[0], ul2[0])) * (min(lr1[1], lr2[1]) - max(ul1[1], ul2[1]))
    area_1 = (lr1[0] - ul1[0]) * (lr1[1] - ul1[1])
    area_2 = (lr2[0] - ul2[0]) * (lr2[1] - ul2[1])
    return float(area_int) / (area_1 + area_2 - area_int)


def ink_plane(image):
    """2-D bool array (True = ink) of a preproc_gpu.DeviceBinImage, or of a 2-D bool / uint8 array (nonzero = ink)"""
    ink = getattr(image, "ink", None)
    if ink is None:
        ink = image
    if type(ink).__module__.split(".")[0] == "torch":
        ink = ink.cpu().numpy()
    ink = np.asarray(ink)
    if ink.ndim != 2:
        raise TypeError("an ink plane is a 2-D array")
    return ink if ink.dtype == bool else ink != 0


def _black(ink, ul, lr):
    """black_area() of Gamera's subimage(ul, lr): ul..lr INCLUSIVE; outside the page -> RuntimeError"""
    x0, y0, x1, y1 = int(ul[0]), int(ul[1]), int(lr[0]), int(lr[1])
    h, w = ink.shape
    if x0 < 0 or y0 < 0 or x1 >= w or y1 >= h or x1 < x0 or y1 < y0:
        raise RuntimeError("Image view dimensions out of range for data")
    return int(np.count_nonzero(ink[y0:y1 + 1, x0:x1 + 1]))


def black_area_IOU(bb1, bb2, image):
    '''intersection over union of the black pixels of two boxes (reference :55-76).  `image`: a DeviceBinImage or a
    2-D bool / uint8 array.  Counts are inclusive of the lower-right row and column (Gamera's subimage; see the module
    docstring); a rectangle outside the page raises RuntimeError, a zero denominator ZeroDivisionError.'''
    ink = ink_plane(image)
    return _black_iou(bb1, bb2, ink)


def _black_iou(bb1, bb2, ink):
    lr1, ul1, lr2, ul2 = bb1['lr'], bb1['ul'], bb2['lr'], bb2['ul']
    new_ul = (max(ul1[0], ul2[0]), max(ul1[1], ul2[1]))
    new_lr = (min(lr1[0], lr2[0]), min(lr1[1], lr2[1]))
    b1 = _black(ink, ul1, lr1)
    b2 = _black(ink, ul2, lr2)
    bi = _black(ink, new_ul, new_lr)
    return float(bi) / (b1 + b2 - bi)


def read_gt_boxes(source):
    """a VOC-style ground-truth file (path or XML text) -> [{'syl', 'difficult', 'ul', 'lr'}] (reference :82-97).
    Only <object> children of the root are read."""
    if isinstance(source, str) and source.lstrip().startswith("<"):
        root = ET.fromstring(source)
    else:
        root = ET.parse(source).getroot()
    out = []
    for el in list(root):
        if not el.tag == 'object':
            continue
        bb = el.find('bndbox')
        out.append({'syl': el.find('name').text, 'difficult': int(el.find('difficult').text),
                    'ul': (int(bb.find('xmin').text), int(bb.find('ymin').text)),
                    'lr': (int(bb.find('xmax').text), int(bb.find('ymax').text))})
    return out


def score_alignment(gt_boxes, syl_boxes, image, eval_difficult=False):
    """(mean IOU, mean black-area IOU) of predicted syllable boxes against ground truth: the array core of the
    reference's evaluate_alignment (:109-131), on the host.  Scores are keyed by syllable NAME (a later box of a name
    overwrites the value, the name keeps its first position); the best predicted box is the first maximum of the
    intersections; no candidate or no overlap scores 0; no scored box gives numpy's nan."""
    ink = ink_plane(image)
    score, area_score = {}, {}
    for box in gt_boxes:
        if box['difficult'] and not eval_difficult:
            continue
        same = [x for x in syl_boxes if x['syl'] in box['syl'] or box['syl'] in x['syl']]
        if not same:
            score[box['syl']] = 0
            area_score[box['syl']] = 0
            continue
        ints = [intersect(box, x) for x in same]
        if not any(ints):
            score[box['syl']] = 0
            area_score[box['syl']] = 0
            continue
        best = same[ints.index(max(ints))]
        score[box['syl']] = IOU(box, best)
        area_score[box['syl']] = _black_iou(box, best, ink)
    return np.mean(list(score.values())), np.mean(list(area_score.values()))


def evaluate_alignment(manuscript, ind, eval_difficult=False, json_dict=None, root='.'):
    """the reference's evaluate_alignment (:79-131) on its file layout under `root`: ground-truth-alignments/
    {m}_{i}_gt.xml, out_json/{m}_{i}.json (unless json_dict is given), png/{m}_{i}_text.png (PIL, then the device
    preprocessing without rotation correction, as the reference does at :106-107)."""
    from PIL import Image
    from . import textAlignPreprocessing as preproc
    fname = '{}_{}'.format(manuscript, ind)
    gt_boxes = read_gt_boxes(os.path.join(root, 'ground-truth-alignments', '{}_gt.xml'.format(fname)))
    if json_dict:
        align_boxes = json_dict['syl_boxes']
    else:
        with open(os.path.join(root, 'out_json', '{}.json'.format(fname)), 'r') as j:
            align_boxes = json.load(j)['syl_boxes']
    raw = np.asarray(Image.open(os.path.join(root, 'png', fname + '_text.png')))
    image, _, _ = preproc.preprocess_images(raw, correct_rotation=False)
    return score_alignment(gt_boxes, align_boxes, image, eval_difficult)


def default_grid():
    """the reference's 729 scoring systems (:181-188) in itertools.product order, int64 [729, 6] (the reference
    shuffles them; the order changes no score)"""
    return np.array(list(itertools.product(*GRID)), dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the sweep
def _dim(d):
    if hasattr(d, "ncols"):
        return page_mod.Dim(d.ncols, d.nrows)
    return page_mod.Dim(int(d[0]), int(d[1]))


class SweepPage(object):
    """One ground-truth page of a sweep: cached OCR characters (CharBox list, as process(..., existing_ocr_pickle=)
    loads them), the transcript, the gt boxes (read_gt_boxes), the deskewing angle and the deskewed / raw page sizes
    (objects with ncols / nrows, or (ncols, nrows)), and the evaluation ink plane (DeviceBinImage or 2-D array)."""

    def __init__(self, all_chars, transcript, gt_boxes, angle, image_dim, raw_dim, ink):
        self.all_chars, self.transcript, self.gt_boxes = list(all_chars), transcript, list(gt_boxes)
        self.angle, self.image_dim, self.raw_dim, self.ink = angle, _dim(image_dim), _dim(raw_dim), ink
        self._prep = None

    @classmethod
    def from_image(cls, raw_image, transcript, all_chars, gt_boxes):
        """angle and deskewed size from the device preprocessing `process` runs, the ink plane from the pass without
        rotation correction that the reference's evaluation runs (:106-107)"""
        from . import alignToOCR
        from . import textAlignPreprocessing as preproc
        image, _, angle = preproc.preprocess_images(raw_image)
        ev_image, _, _ = preproc.preprocess_images(raw_image, correct_rotation=False)
        return cls(all_chars, transcript, gt_boxes, angle, image.dim, alignToOCR._raw_dim(raw_image), ev_image)

    def prepared(self):
        """everything that does not depend on the scoring system, once: expanded OCR text and boxes, token ids,
        syllables and their transcript spans"""
        if self._prep is None:
            text = ''.join(str(c.char) for c in self.all_chars)
            boxes = np.array([[c.ulx, c.uly, c.lrx, c.lry] for c in self.all_chars], dtype=np.int64).reshape(-1, 4)
            text, idx = page_batch.expand_abbreviations(text, np.arange(len(text), dtype=np.int64), latsyl.abbreviations)
            if '_' in text:              # a literal '_' counts as a gap marker in align_page: the reference's assert
                raise AssertionError('all_chars not same length as alignment')
            if page_batch._META & set(self.transcript):
                raise ValueError("the sweep takes transcripts without regular-expression metacharacters")
            syls = latsyl.syllabify_text(self.transcript)
            first, last = page_batch.syllable_spans(self.transcript, syls)       # AttributeError if not found
            (t_ids, o_ids), _ = tsc.encode_tokens(list(self.transcript), list(text))
            self._prep = dict(boxes=boxes[np.asarray(idx, dtype=np.int64)], names=[s for s in syls if s],
                              first=first, last=last, t_ids=t_ids, o_ids=o_ids)
        return self._prep

    def representatives(self, eval_difficult=False):
        """(names, boxes [r, 4], candidates per box, pick): every COUNTED gt box (difficult ones only with
        eval_difficult) in file order -- each is scored, and any of them can stop the reference's loop (:109-129) --
        the syllable indices whose name contains or is contained in the box's, ascending; and for the names in the
        order they were first counted, the index of the LAST box of that name (the value the reference's dict keeps)"""
        counted = [b for b in self.gt_boxes if eval_difficult or not b['difficult']]
        order, last = [], {}
        for k, b in enumerate(counted):
            if b['syl'] not in last:
                order.append(b['syl'])
            last[b['syl']] = k
        names = self.prepared()['names']
        uniq = {}
        for k, s in enumerate(names):
            uniq.setdefault(s, []).append(k)
        cands = []
        for b in counted:
            g = b['syl']
            ks = [k for s, idx in uniq.items() if s in g or g in s for k in idx]
            cands.append(np.sort(np.asarray(ks, dtype=np.int64)))
        boxes = np.array([[b['ul'][0], b['ul'][1], b['lr'][0], b['lr'][1]] for b in counted],
                         dtype=np.int64).reshape(-1, 4)
        return order, boxes, cands, np.array([last[g] for g in order], dtype=np.int64)


class SweepResult(object):
    """systems [S, 6]; iou, area, status [P, S] (status: TA_EVAL_* codes, STATUS_NAMES); score [S] = the mean over pages
    of `area`, the reference's try_params value (:175)"""

    def __init__(self, systems, iou, area, status):
        self.systems, self.iou, self.area, self.status = systems, iou, area, status
        # np.mean of each system's list of page values (rows made contiguous: numpy's reduction per row)
        self.score = np.mean(np.ascontiguousarray(area.T), axis=1) if area.shape[0] else np.full(len(systems), np.nan)

    def ranking(self):
        """[(system tuple, score)] sorted by score, ascending: the reference's final list (:195-198)"""
        return sorted([(tuple(int(v) for v in s), float(x)) for s, x in zip(self.systems, self.score)], key=lambda t: t[1])


def _systems_array(systems):
    if systems is None:
        return default_grid()
    rows = []
    for k, s in enumerate(systems):
        if callable(s) or (hasattr(s, '__len__') and len(s) and callable(s[0])):
            raise ValueError("scoring system %d: the sweep takes integral scoring systems, not callables" % k)
        params, _ = tsc.parse_scoring_system(s)
        if not tsc._is_integral(params):
            raise ValueError("scoring system %d (%r) is not integral" % (k, list(params)))
        rows.append([int(v) for v in params])
    return np.array(rows, dtype=np.int64).reshape(-1, 6)


def _rotation_table(pages):
    ang = (-1 * np.asarray([p.angle for p in pages], dtype=np.float64)) * np.pi / 180
    sn, cs = np.sin(ang), np.cos(ang)
    rot = np.empty((len(pages), 6), dtype=np.float64)
    for k, p in enumerate(pages):
        px, py = p.image_dim.ncols // 2, p.image_dim.nrows // 2
        dx = (p.image_dim.ncols - p.raw_dim.ncols) // 2
        dy = (p.image_dim.nrows - p.raw_dim.nrows) // 2
        rot[k] = (sn[k], cs[k], px, py, px - dx, py - dy)
    return rot


def _device_ink(ink, device):
    import torch
    plane = getattr(ink, "plane", None)
    if plane is not None and plane.dtype == torch.uint8 and plane.device == device:
        return plane.contiguous()
    return torch.from_numpy(np.ascontiguousarray(ink_plane(ink), dtype=np.uint8)).to(device)


def sweep(pages, systems=None, eval_difficult=False, device="cuda", timings=None):
    """The reference's grid search (try_params over every system, :134-198) in one call: every page aligned under
    every system in ONE NWBatch, then syllable boxes and scores on the device.  Returns a SweepResult.  Raises up
    front for a page what `process` would raise whatever the system (a literal '_' in the OCR text: AssertionError; a
    syllable not in the transcript: AttributeError) and for a system that is not integral (ValueError).  A rectangle
    outside the page or a zero black-area denominator only marks its (page, system): status code, means nan.
    `timings`: a dict that receives host / device times in ms (tools/sweep_time.py)."""
    import time
    import torch
    tsc._require_gpu()
    t0 = time.perf_counter()
    sysarr = _systems_array(systems)
    pages = list(pages)
    P, S = len(pages), len(sysarr)
    preps = [p.prepared() for p in pages]
    reps = [p.representatives(eval_difficult) for p in pages]
    t1 = time.perf_counter()
    if P == 0 or S == 0:
        z = np.zeros((P, S))
        return SweepResult(sysarr, z, z.copy(), np.zeros((P, S), np.int32))
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    events = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if timings is not None else None
    if events:
        events[0].record()
    batch = tsc.NWBatch([q['t_ids'] for q in preps for _ in range(S)], [q['o_ids'] for q in preps for _ in range(S)],
                        np.tile(sysarr, (P, 1)), device=dev)
    batch.run()
    if events:
        events[1].record()
    lib = _native.lib
    stream = torch.cuda.current_stream(dev).cuda_stream
    NP = P * S
    nsyl = np.array([len(q['names']) for q in preps], dtype=np.int64)
    nrep = np.array([len(r[1]) for r in reps], dtype=np.int64)
    max_syl, max_rep = int(max(nsyl.max(), 1)), int(nrep.max())
    char_off = np.zeros(P + 1, np.int64); np.cumsum([len(q['boxes']) for q in preps], out=char_off[1:])
    syl_off = np.zeros(P + 1, np.int64); np.cumsum(nsyl, out=syl_off[1:])
    rep_off = np.zeros(P + 1, np.int64); np.cumsum(nrep, out=rep_off[1:])
    cand_all = [c for r in reps for c in r[2]]
    cand_off = np.zeros(len(cand_all) + 1, np.int64); np.cumsum([len(c) for c in cand_all], out=cand_off[1:])
    cand = np.concatenate(cand_all).astype(np.int32) if cand_all and cand_off[-1] else np.zeros(1, np.int32)
    prob_page = np.repeat(np.arange(P, dtype=np.int32), S)
    out_off = np.zeros(NP + 1, np.int64); np.cumsum(nrep[prob_page], out=out_off[1:])
    total = int(out_off[-1])
    max_cols = int(max(2 * len(q['t_ids']) + len(q['o_ids']) for q in preps))
    inks = [_device_ink(p.ink, dev) for p in pages]
    sats = [torch.empty(tuple(t.shape), dtype=torch.int32, device=dev) for t in inks]
    sat_h = np.array([t.shape[0] for t in inks], dtype=np.int32)
    sat_w = np.array([t.shape[1] for t in inks], dtype=np.int32)
    sat_ptr = np.array([t.data_ptr() for t in sats], dtype=np.uint64)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)          # noqa: E731
    (d_page, d_cbox, d_coff, d_first, d_last, d_soff, d_rot, d_gt, d_roff, d_cof, d_cand, d_satp, d_sh, d_sw,
     d_oof) = _native.upload_packed(
        [prob_page, i32(np.concatenate([q['boxes'] for q in preps]).reshape(-1, 4)) if char_off[-1] else np.zeros(4, np.int32),
         char_off, i32(np.concatenate([q['first'] for q in preps])) if syl_off[-1] else np.zeros(1, np.int32),
         i32(np.concatenate([q['last'] for q in preps])) if syl_off[-1] else np.zeros(1, np.int32), syl_off,
         _rotation_table(pages), i32(np.concatenate([r[1] for r in reps])) if rep_off[-1] else np.zeros(4, np.int32),
         rep_off, cand_off, cand, sat_ptr.view(np.int64), sat_h, sat_w, out_off], dev)
    ink_ptr = np.array([t.data_ptr() for t in inks], dtype=np.uint64)
    _native.check(lib.ta_eval_integral(P, ink_ptr.ctypes.data, sat_h.ctypes.data, sat_w.ctypes.data, sat_ptr.ctypes.data,
                                       stream), "ta_eval_integral")
    if events:
        events[2].record()
    boxes = torch.empty((NP, max_syl, 4), dtype=torch.int32, device=dev)
    present = torch.empty((NP, max_syl), dtype=torch.uint8, device=dev)
    box_status = torch.empty(NP, dtype=torch.int32, device=dev)
    _native.check(lib.ta_eval_syllable_boxes(
        batch.ops.data_ptr(), batch.ops_off.data_ptr(), batch.ops_len.data_ptr(), batch.t_off.data_ptr(),
        batch.o_off.data_ptr(), NP, d_page.data_ptr(), d_cbox.data_ptr(), d_coff.data_ptr(), d_first.data_ptr(),
        d_last.data_ptr(), d_soff.data_ptr(), d_rot.data_ptr(), max_syl, max_cols, boxes.data_ptr(), present.data_ptr(),
        box_status.data_ptr(), stream), "ta_eval_syllable_boxes")
    if events:
        events[3].record()
    # per-box results in ONE buffer: iou, area (float64), status (int32)
    buf = torch.empty(max(20 * total, 16), dtype=torch.uint8, device=dev)
    d_iou, d_area = buf[:8 * total].view(torch.float64), buf[8 * total:16 * total].view(torch.float64)
    d_st = buf[16 * total:20 * total].view(torch.int32)
    _native.check(lib.ta_eval_score(
        NP, d_page.data_ptr(), boxes.data_ptr(), present.data_ptr(), box_status.data_ptr(), max_syl, d_gt.data_ptr(),
        d_roff.data_ptr(), d_cof.data_ptr(), d_cand.data_ptr(), d_satp.data_ptr(), d_sh.data_ptr(), d_sw.data_ptr(),
        d_oof.data_ptr(), max_rep, d_iou.data_ptr(), d_area.data_ptr(), d_st.data_ptr(), stream), "ta_eval_score")
    if events:
        events[4].record()
    host = buf.cpu().numpy()
    t2 = time.perf_counter()
    h_iou, h_area = host[:8 * total].view(np.float64), host[8 * total:16 * total].view(np.float64)
    h_st = host[16 * total:20 * total].view(np.int32)
    iou, area = np.full((P, S), np.nan), np.full((P, S), np.nan)
    status = np.zeros((P, S), dtype=np.int32)
    for k in range(P):
        a, r = int(out_off[k * S]), int(nrep[k])
        if r == 0:                     # no counted gt box: numpy's mean of nothing, nan (status stays 0)
            continue
        st = h_st[a:a + S * r].reshape(S, r)
        pick = reps[k][3]
        if len(pick) == 0:
            continue
        iou[k] = np.mean(np.ascontiguousarray(h_iou[a:a + S * r].reshape(S, r)[:, pick]), axis=1)
        area[k] = np.mean(np.ascontiguousarray(h_area[a:a + S * r].reshape(S, r)[:, pick]), axis=1)
        bad = (st != 0).any(axis=1)
        if bad.any():
            status[k, bad] = st[bad][np.arange(int(bad.sum())), np.argmax(st[bad] != 0, axis=1)]
            iou[k, bad] = np.nan
            area[k, bad] = np.nan
    res = SweepResult(sysarr, iou, area, status)
    if timings is not None:
        t3 = time.perf_counter()
        timings.update(host_prep_ms=1e3 * (t1 - t0), host_means_ms=1e3 * (t3 - t2),
                       nw_ms=events[0].elapsed_time(events[1]), integral_ms=events[1].elapsed_time(events[2]),
                       boxes_ms=events[2].elapsed_time(events[3]), score_ms=events[3].elapsed_time(events[4]))
    res.device_boxes = (boxes, present, box_status)
    res.batch = batch
    return res


def try_params(params, pages):
    """the reference's try_params (:134-175) for one scoring system: mean over pages of the black-area IOU"""
    return float(sweep(pages, [params]).score[0])
