"""Character positions for lines whose text is known -- `ocropus-rpred --llocs` with the text given instead of decoded:
character-level ground truth from line-level ground truth.

    python tools/rforced.py DIR -m MODEL

DIR holds NAME.png + NAME.gt.txt pairs, as tools/rtrain.py reads them.  Every line is recognised with MODEL (a
.pyrnn.gz), its probabilities are aligned with its text on the device (text_alignment_amd/forced.py: the best CTC path
through exactly that text) and NAME.llocs is written beside it: one `character<TAB>x` row per
character of the text, x the position of the character's peak in pixels of the line image, one decimal.  A line whose
text has a character the model's codec lacks, or more characters than its timesteps can hold, is reported and skipped.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.rtrain import read_pairs  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("directory")
    ap.add_argument("-m", "--model", required=True, help="a .pyrnn.gz line model")
    args = ap.parse_args(argv)
    from text_alignment_amd import forced, ocr
    pairs = [p for p in read_pairs(args.directory) if p[1]]
    if not pairs:
        sys.exit("no NAME.png + NAME.gt.txt pairs in %s" % args.directory)
    rec = forced._recognizer(args.model)
    written = []
    for img, text, png in pairs:                       # line by line: one bad text does not cost the others theirs
        try:
            (chars, score), = forced.align_lines(rec, [img], [text])
        except ValueError as e:
            print("skipped %s: %s" % (png, e), file=sys.stderr)
            continue
        out = png[:-len(".png")] + ".llocs"
        with open(out, "w", encoding="utf-8") as f:
            f.write(ocr.llocs_text([(c[0], c[4]) for c in chars]))
        written.append((out, score))
    print("%d of %d lines written" % (len(written), len(pairs)))
    return written


if __name__ == "__main__":
    main()
