#!/usr/bin/env python3
"""tools/gen_golden_eval.py -- capture the reference's alignment evaluation as tests/golden/eval.json.

Runs ONLY in the build container (needs the reference tree, which never travels to the GPU box).  It reuses
tools/gen_golden.py's `import_reference()` (stand-in Gamera) and `run_process()` (canned OCR), builds three
seeded synthetic pages, and for EVERY scoring system of the reference's grid (evaluate_text_alignment.py:181-188,
3^6 = 729 of them) runs the imported reference's

    process -> to_JSON_dict -> evaluate_alignment

on each page: 2 187 reference `process` calls on ~200 x 200 problems, spread over a process pool (~1-2 minutes on
eight cores).  The evaluation image is a stand-in whose `subimage(ul, lr).black_area()` counts the page's ink
plane over ul..lr INCLUSIVE (Gamera's subimage includes the lower-right row and column) and raises RuntimeError
outside the page, as Gamera's view constructor does.  Python 3 needs `list(...)` around the reference's
`np.mean(dict.values())`; a wrapper numpy handed to the reference module does that.

Only data is written: the page inputs (ink planes as packed bits, zlib, base64), the gt XML text, both means per
(page, system), the reference's `syl_boxes` for a seeded sample of systems, and a handful of direct
intersect / IOU / black_area_IOU cases.

    python tools/gen_golden_eval.py [--jobs 8]
"""
import argparse
import base64
import itertools
import json
import multiprocessing
import os
import sys
import tempfile
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from tools.gen_golden import GOLD, import_reference, layout_chars, run_process  # noqa: E402

GRID = [[5, 8, 11], [-4, -7, -10], [-2, -5, -7], [-2, -5, -7], [0, -3, -5], [0, -3, -5]]
MANUSCRIPT = "synth"

VOCAB = ("dominus deus meus alleluia gloria patri et filio spiritui sancto sicut erat in principio nunc semper "
         "saecula saeculorum amen laudate eum omnes gentes quoniam confirmata est super nos misericordia eius "
         "veritas manet aeternum a domino factum est istud").split()


# ----------------------------------------------------------------------------- stand-in evaluation image
class _SubImage(object):
    def __init__(self, count):
        self.count = count

    def black_area(self):
        return [self.count]


class InkImage(object):
    """what evaluate_alignment reads from the preprocessed page: subimage(ul, lr).black_area()[0]"""

    def __init__(self, ink):
        self.ink = np.asarray(ink, dtype=bool)

    def subimage(self, ul, lr):
        x0, y0, x1, y1 = int(ul[0]), int(ul[1]), int(lr[0]), int(lr[1])
        h, w = self.ink.shape
        if x0 < 0 or y0 < 0 or x1 >= w or y1 >= h or x1 < x0 or y1 < y0:
            raise RuntimeError("Image view dimensions out of range for data")
        return _SubImage(int(self.ink[y0:y1 + 1, x0:x1 + 1].sum()))


class _ListMeanNumpy(object):
    """numpy, except that mean() reads a dict view as the list Python 2's dict.values() was"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def mean(a, *args, **kw):
        if isinstance(a, type({}.values())):
            a = list(a)
        return np.mean(a, *args, **kw)


# ----------------------------------------------------------------------------- synthetic pages
def rotate_np(boxes, angle, orig_dim, target_dim):
    """the reference's rotate_bbox on an int array [k, 4] (even dimensions: its divisions are exact)"""
    px, py = orig_dim[0] // 2, orig_dim[1] // 2
    dx, dy = (orig_dim[0] - target_dim[0]) // 2, (orig_dim[1] - target_dim[1]) // 2
    a = angle * np.pi / 180
    s, c = np.sin(a), np.cos(a)
    x = boxes[:, 0::2] - px
    y = boxes[:, 1::2] - py
    rx = np.round((x * c) - (y * s) + (px - dx)).astype(np.int64)
    ry = np.round((x * s) + (y * c) + (py - dy)).astype(np.int64)
    return np.stack([rx[:, 0], ry[:, 0], rx[:, 1], ry[:, 1]], axis=1)


def make_page(seed, angle, img_dim, raw_dim, latsyl, length=170):
    """a seeded page: transcript, noisy OCR laid out 24 characters per line, ink plane of the raw page, gt boxes
    (tests/test_evaluate_gpu.py builds its page-size cases with it too)"""
    rng = np.random.default_rng(seed)
    words = []
    while len(" ".join(words)) < length + int(rng.integers(0, 60)):
        words.append(VOCAB[int(rng.integers(0, len(VOCAB)))])
    if "dominus" not in words:
        words[int(rng.integers(0, len(words)))] = "dominus"
    tr = " ".join(words)
    # OCR: substitutions, drops, insertions; src[k] = transcript position of OCR char k (-1: inserted)
    abb_at = tr.find("dominus")
    oc, src = [], []
    k = 0
    while k < len(tr):
        if k == abb_at:                          # one abbreviation: 'dominus' read as 'dns'
            for j, ch in zip((0, 3, 6), "dns"):
                oc.append(ch)
                src.append(k + j)
            k += len("dominus")
            continue
        ch = tr[k]
        u = rng.random()
        if u < 0.05:
            k += 1
            continue
        oc.append("abcdefghilmnorstu "[int(rng.integers(0, 18))] if u < 0.15 else ch)
        src.append(k)
        if rng.random() < 0.04:
            oc.append("il.t"[int(rng.integers(0, 4))])
            src.append(-1)
        k += 1
    oc = "".join(oc)
    chars = layout_chars(oc, per_line=24, x0=40, dx=18, w=16, y0=60, dy=90, h=36)
    nlines = (len(oc) + 23) // 24
    peaks = [78 + 90 * i for i in range(nlines + 1)]
    img_boxes = np.array([[ul[0], ul[1], lr[0], lr[1]] for _, ul, lr in chars], dtype=np.int64)
    raw_boxes = rotate_np(img_boxes, -angle, img_dim, raw_dim)
    # ink plane of the raw page: strokes under every non-space character, plus specks
    W, H = raw_dim
    ink = np.zeros((H, W), dtype=bool)
    for (ch, _, _), b in zip(chars, raw_boxes):
        if ch == " ":
            continue
        x0, y0, x1, y1 = (int(v) for v in b)
        x0, y0, x1, y1 = max(x0 + 2, 0), max(y0 + 4, 0), min(x1 - 2, W - 1), min(y1 - 4, H - 1)
        if x1 <= x0 or y1 <= y0:
            continue
        ink[y0:y1, x0:x1] |= rng.random((y1 - y0, x1 - x0)) < 0.45
    sp = rng.integers(0, H * W, size=400)
    ink.reshape(-1)[sp] = True
    # ground truth: per syllable, union of the boxes of the OCR characters that came from its letters (lowest line)
    syls = latsyl.syllabify_text(tr)
    ocr_of_t = {}
    for j, s in enumerate(src):
        if s >= 0:
            ocr_of_t.setdefault(s, []).append(j)
    gt = []
    cur = 0
    for syl in syls:
        if not syl:
            continue
        p = tr.find(syl, cur)
        cur = p + len(syl)
        js = [j for t in range(p, cur) for j in ocr_of_t.get(t, [])]
        if not js:
            continue
        bx = raw_boxes[js]
        low = bx[:, 1].max()
        bx = bx[bx[:, 1] == low]
        box = [int(bx[:, 0].min()), int(bx[:, 1].min()), int(bx[:, 2].max()), int(bx[:, 3].max())]
        box = [v + int(rng.integers(-3, 4)) for v in box]
        gt.append(dict(syl=syl, difficult=int(rng.random() < 0.1), box=box))
    # the named cases
    named = [g for g in gt if not g["difficult"]]
    dup = named[len(named) // 3]
    b = list(named[2 * len(named) // 3]["box"])
    gt.append(dict(syl=dup["syl"], difficult=0, box=b))                          # same name, another box
    with_a = [g for g in named if "a" in g["syl"] and g["syl"] != "a"]
    gt.append(dict(syl="a", difficult=0, box=list(with_a[0]["box"])))           # a substring of other names
    gt.append(dict(syl="zzx", difficult=0, box=list(named[1]["box"])))          # absent from the transcript
    gt.append(dict(syl=named[0]["syl"], difficult=0, box=[W - 40, H - 40, W - 10, H - 10]))   # meets nothing
    gt.insert(3, dict(syl=named[5]["syl"], difficult=1, box=list(named[6]["box"])))          # difficult, shadowed
    for g in gt:
        x0, y0, x1, y1 = g["box"]
        g["box"] = [max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)]
    return dict(transcript=tr, chars=[[c, list(ul), list(lr)] for c, ul, lr in chars], peak_locs=peaks,
                angle=angle, img_dim=list(img_dim), raw_dim=list(raw_dim), gt=gt), ink


def gt_xml(gt):
    rows = ["<annotation>", "  <filename>page.png</filename>", "  <size><width>0</width><height>0</height></size>"]
    for g in gt:
        x0, y0, x1, y1 = g["box"]
        rows += ["  <object>", "    <name>%s</name>" % g["syl"], "    <pose>Unspecified</pose>",
                 "    <truncated>0</truncated>", "    <difficult>%d</difficult>" % g["difficult"],
                 "    <bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox>" % (x0, y0, x1, y1),
                 "  </object>"]
    rows.append("</annotation>")
    return "\n".join(rows) + "\n"


def pack_ink(ink):
    return dict(shape=list(ink.shape), bits=base64.b64encode(zlib.compress(np.packbits(ink).tobytes(), 9)).decode())


# ----------------------------------------------------------------------------- reference runs (pool workers)
_W = {}


def _init_worker(pages, inks):
    tsc, latsyl, atocr = import_reference()
    import evaluate_text_alignment as ev
    ev.np = _ListMeanNumpy()
    _W.update(atocr=atocr, ev=ev, pages=pages, inks=inks, tmp=tempfile.mkdtemp(prefix="gen_eval_"))
    os.makedirs(os.path.join(_W["tmp"], "ground-truth-alignments"), exist_ok=True)
    for k, pg in enumerate(pages):
        with open(os.path.join(_W["tmp"], "ground-truth-alignments", "%s_%d_gt.xml" % (MANUSCRIPT, k)), "w") as f:
            f.write(pg["xml"])


def _run_one(job):
    k, sys_row = job
    atocr, ev, pg = _W["atocr"], _W["ev"], _W["pages"][k]
    js, _ = run_process(atocr, pg["transcript"], [(c, tuple(ul), tuple(lr)) for c, ul, lr in pg["chars"]],
                        pg["peak_locs"], pg["angle"], pg["img_dim"], pg["raw_dim"], list(sys_row))
    image = InkImage(_W["inks"][k])
    ev.gc.load_image = lambda path: None
    ev.preproc.preprocess_images = lambda raw, correct_rotation=True: (image, None, 0)
    cwd = os.getcwd()
    os.chdir(_W["tmp"])
    try:
        iou, area = ev.evaluate_alignment(MANUSCRIPT, k, eval_difficult=False, json_dict=js)
    finally:
        os.chdir(cwd)
    return k, list(sys_row), float(iou), float(area), js["syl_boxes"]


def direct_cases(ev, ink):
    img = InkImage(ink)
    pairs = [((50, 60, 90, 100), (70, 80, 120, 130)), ((50, 60, 90, 100), (50, 60, 90, 100)),
             ((40, 60, 160, 96), (100, 62, 130, 90)), ((10, 10, 20, 20), (30, 30, 40, 40)),
             ((10, 10, 20, 20), (20, 10, 30, 20)), ((100, 150, 230, 190), (95, 148, 180, 200))]
    out = []
    for a, b in pairs:
        ba, bb = dict(ul=a[:2], lr=a[2:]), dict(ul=b[:2], lr=b[2:])
        row = dict(a=list(a), b=list(b), intersect=ev.intersect(ba, bb), iou=ev.IOU(ba, bb))
        try:
            row["black_iou"] = ev.black_area_IOU(ba, bb, img)
        except (RuntimeError, ZeroDivisionError) as e:
            row["black_iou"] = type(e).__name__
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    _, latsyl, _ = import_reference()
    import evaluate_text_alignment as ev
    specs = [(7101, 0, (560, 1000), (560, 1000)), (7102, 1.35, (600, 1040), (560, 1000)),
             (7103, -0.85, (580, 1024), (560, 1000))]
    pages, inks = [], []
    for seed, angle, img_dim, raw_dim in specs:
        pg, ink = make_page(seed, angle, img_dim, raw_dim, latsyl)
        pg["xml"] = gt_xml(pg.pop("gt"))
        pages.append(pg)
        inks.append(ink)
        print("page", seed, len(pg["transcript"]), "transcript chars", len(pg["chars"]), "OCR chars", flush=True)
    systems = [list(p) for p in itertools.product(*GRID)]
    rng = np.random.default_rng(20261016)
    sample = sorted(int(i) for i in rng.choice(len(systems), size=8, replace=False))
    jobs = [(k, s) for k in range(len(pages)) for s in systems]
    iou = np.zeros((len(pages), len(systems)))
    area = np.zeros((len(pages), len(systems)))
    boxes = {}
    index = {tuple(s): i for i, s in enumerate(systems)}
    with multiprocessing.get_context("fork").Pool(args.jobs, _init_worker, (pages, inks)) as pool:
        for n, (k, s, a, b, sb) in enumerate(pool.imap_unordered(_run_one, jobs, chunksize=16)):
            i = index[tuple(s)]
            iou[k, i], area[k, i] = a, b
            if i in sample:
                boxes["%d:%d" % (k, i)] = sb
            if n % 200 == 0:
                print("reference evaluations", n, "/", len(jobs), flush=True)
    out = dict(manuscript=MANUSCRIPT, grid=GRID, pages=[], sample_systems=sample, direct=direct_cases(ev, inks[0]))
    for k, (pg, ink) in enumerate(zip(pages, inks)):
        out["pages"].append(dict(pg, ink=pack_ink(ink), iou=iou[k].tolist(), area=area[k].tolist(),
                                 syl_boxes={str(i): boxes["%d:%d" % (k, i)] for i in sample}))
    path = os.path.join(GOLD, "eval.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=False, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
