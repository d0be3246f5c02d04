"""Harvest line-level training data from page images and page transcripts -- the step between the page pipeline and
`tools/rtrain.py`: no hand-made line ground truth.

    python tools/rharvest.py PAGES -m MODEL.pyrnn.gz -o OUT [--min-agreement 0.9] [--params 8,-4,-7,-7,-3,0]
                             [--report OUT/report.tsv] [--batch 16]

PAGES holds page images (png, jpg, tif) and same-named NAME.txt transcripts.  Every page goes through the recogniser and
the aligner, and the alignment is cut into per-line texts on the device (text_alignment_amd/harvest.py; DESIGN.md section
14.6).  For every ACCEPTED line OUT gets NAME-LLL.png (the line's strip as the recogniser saw it) and NAME-LLL.gt.txt (its
piece of the transcript) -- the pairs tools/rtrain.py reads.  The report is one TSV row per line, accepted or not: page,
line, reason bits and names, t_first, the counts, the text.  --min-agreement: the least share of a line's columns that
must be pairs of equal characters, a number in (0, 1] or NUM/DEN.
"""
import argparse
import glob
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".tif", ".tiff")


def find_pages(directory):
    """[(name, image path, transcript path)] for every image with a same-named .txt, sorted by name"""
    found = []
    for path in sorted(glob.glob(os.path.join(directory, "*"))):
        stem, ext = os.path.splitext(path)
        if ext.lower() in IMAGE_SUFFIXES and os.path.exists(stem + ".txt"):
            found.append((os.path.basename(stem), path, stem + ".txt"))
    return found


def parse_agreement(s):
    if "/" in s:
        num, den = s.split("/", 1)
        return int(num), int(den)
    return s


def report_row(name, ln, t_first):
    c = ln.counts
    return [name, str(ln.line), str(ln.reason), ",".join(ln.reasons()) or "accepted", str(t_first),
            str(len(ln.text or "")), str(c["equal"]), str(c["unequal"]), str(c["interior"]), str(c["op2"]), str(c["seam"]),
            (ln.text or "").replace("\t", " ").replace("\n", " ")]


HEADER = ["page", "line", "reason", "reasons", "t_first", "L", "equal", "unequal", "interior", "op2", "seam", "text"]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("directory")
    ap.add_argument("-m", "--model", required=True, help="the line model (.pyrnn.gz) to recognise with")
    ap.add_argument("-o", "--output", required=True, help="directory for the NAME-LLL.png + NAME-LLL.gt.txt pairs")
    ap.add_argument("--min-agreement", default="0.9")
    ap.add_argument("--params", default=None, help="the aligner's scoring system, comma-separated integers")
    ap.add_argument("--report", default=None, help="TSV report (default: OUTPUT/report.tsv)")
    ap.add_argument("--batch", type=int, default=16, help="pages per call")
    args = ap.parse_args(argv)
    from PIL import Image
    from text_alignment_amd import alignToOCR as atocr, harvest
    ratio = harvest.agreement_ratio(parse_agreement(args.min_agreement))
    params = [int(v) for v in args.params.split(",")] if args.params else None
    found = find_pages(args.directory)
    if not found:
        sys.exit("no page image with a same-named .txt in %s" % args.directory)
    os.makedirs(args.output, exist_ok=True)
    report = args.report or os.path.join(args.output, "report.tsv")
    rec = atocr._recognizer_for(args.model)
    total = accepted = 0
    with open(report, "w", encoding="utf-8") as rep:
        rep.write("\t".join(HEADER) + "\n")
        for a in range(0, len(found), max(args.batch, 1)):
            group = found[a:a + max(args.batch, 1)]
            pages = [np.ascontiguousarray(np.array(Image.open(img).convert("L"), dtype=np.uint8)) for _, img, _ in group]
            trs = [atocr.read_file(txt) for _, _, txt in group]
            res = harvest.harvest_pages(pages, trs, rec, params, ratio)
            for q, ln in enumerate(res.lines):
                name = group[ln.page][0]
                rep.write("\t".join(report_row(name, ln, int(res.table[q, 1]))) + "\n")
                total += 1
                if ln.reason == 0:
                    accepted += 1
                    stem = os.path.join(args.output, "%s-%03d" % (name, ln.line))
                    Image.fromarray(np.ascontiguousarray(ln.source.pixels)).save(stem + ".png")
                    with open(stem + ".gt.txt", "w", encoding="utf-8") as f:
                        f.write(ln.text + "\n")
    print("%d of %d lines accepted at %d/%d; pairs in %s, report %s" % (accepted, total, ratio[0], ratio[1], args.output, report))


if __name__ == "__main__":
    main()
