"""Character positions for lines whose text is known -- `ocropus-rpred --llocs` with the text given instead of decoded:
character-level ground truth from line-level ground truth.

    python tools/rforced.py DIR -m MODEL

DIR holds NAME.png + NAME.gt.txt pairs, as tools/rtrain.py reads them.  Every line is recognised with MODEL (a
.pyrnn.gz), its probabilities are aligned with its text on the device (text_alignment_amd/forced.py: the best CTC path
through exactly that text) and NAME.llocs is written beside it: one `character<TAB>x` row per
character of the text, x the position of the character's peak in pixels of the line image, one decimal.  A line whose
text has a character the model's codec lacks, or more characters than its timesteps can hold, is reported and skipped.

    python tools/rforced.py DIR -m MODEL --omit BITS

The path may leave characters of the text out at BITS each (an abbreviation, a spelling the
scribe did not use).  NAME.llocs then holds the rows of the characters the path shows; the omitted ones are listed on
stderr and counted in the summary.  No value of BITS has been validated on real pages.

    python tools/rforced.py DIR -m MODEL --omit BITS --omit-confidence

Also writes NAME.conf beside NAME.llocs, from the max-marginals of the lattice with omission: one
`character<TAB>bits<TAB>rival` row per character of the TEXT, in --confidence's format, with a fourth field `omitted` on the
row of a character the path left out.  A present character's bits are >= 0: how far the best path that keeps it on its peak
frame lies above the best one that puts anything else there.  An omitted character's are <= 0: the best path through its
state at one of the two frames around the place it was jumped at, against the best path itself -- minus it bounds from
ABOVE what the best path would lose if the character had to appear; near 0 the omission was a coin toss.  The summary names
the lowest value of a present character and the omission nearest to 0.  Not with --page.  No threshold has been validated
on real pages.

    python tools/rforced.py DIR -m MODEL --confidence

Also writes NAME.conf beside NAME.llocs: one `character<TAB>bits<TAB>rival` row per character --
how many bits (three decimals) the best path that keeps the character on its peak frame lies above the best path that
puts anything else there, and the character of that rival (`~` for a blank).  The summary names the lowest value.  Not
with --omit or --page.  No threshold has been validated on real pages.

    python tools/rforced.py DIR -m MODEL --posterior

Also writes NAME.post beside NAME.llocs: one `character<TAB>posterior<TAB>rival<TAB>posterior`
row per character -- the probability (four decimals), all CTC paths through the text summed, that the character holds its
peak frame, then the state with the largest posterior among the others at that frame (its character, `~` for a blank) and
that posterior.  Every line's log2 P(text | line) per frame is printed, and the summary names the lowest.  Not with --omit
or --page.  Nothing about real pages has been measured.

    python tools/rforced.py DIR -m MODEL --page TEXT

DIR holds the line images NAME.png of ONE page, taken in name order, and TEXT is a file with the page's text (line breaks
count as spaces).  One best path through all the lines decides which character lies on which line (forced.align_page_lines;
DESIGN.md section 14.8), and every NAME.llocs receives the rows of the characters that fell to it.

    python tools/rforced.py DIR -m MODEL --page TEXT --page-omit BITS

The page's path may leave characters of TEXT out at BITS each, so a text with more characters
than the lines have frames still has a path.  Every NAME.llocs holds the rows of the characters that are present; the
omitted ones are named on stderr and counted in the summary.  No value of BITS has been validated on real pages.

    python tools/rforced.py DIR -m MODEL --page TEXT --page-confidence

Also writes NAME.conf beside every NAME.llocs, in --confidence's format, from the max-marginals of the page's ONE lattice
(DESIGN.md section 14.13): how many bits the best path through all the lines that keeps the character on its line and peak
frame lies above the best one that puts anything else there, and the character of that rival -- any character of TEXT
that line's window holds (`~` for a blank).  The summary names the lowest value.  Not with --page-omit.  No threshold has
been validated on real pages.

    python tools/rforced.py DIR -m MODEL --page TEXT --page-posterior

Also writes NAME.post beside every NAME.llocs, in --posterior's format, from the sum-product posteriors of the page's ONE
lattice: the probability, ALL legal paths through all the lines summed, that the character holds
its line and peak frame, then the live state with the largest posterior among the others at that frame (any character of
TEXT that line's window holds, `~` for a blank) and that posterior.  The page's log2 P(text | page) per frame is printed.
Goes with --page-confidence; not with --page-omit.  No threshold on a posterior has been validated on real pages.
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
    ap.add_argument("--page", metavar="TEXT", help="a text file: the images are the lines of one page with this text")
    ap.add_argument("--omit", metavar="BITS", type=float,
                    help="the path may leave a character of the text out at this price in bits (not with --page)")
    ap.add_argument("--page-omit", metavar="BITS", type=float,
                    help="with --page: the page's path may leave a character of the text out at this price in bits")
    ap.add_argument("--confidence", action="store_true",
                    help="also write NAME.conf: per character its confidence in bits and its rival (not with --omit, --page)")
    ap.add_argument("--omit-confidence", action="store_true",
                    help="with --omit: also write NAME.conf, per character of the text its confidence on the lattice with "
                         "omission, an omitted character marked")
    ap.add_argument("--posterior", action="store_true",
                    help="also write NAME.post: per character its sum-product posterior and its rival's (not with --omit, --page)")
    ap.add_argument("--page-confidence", action="store_true",
                    help="with --page: also write NAME.conf per line, from the page's one lattice (not with --page-omit)")
    ap.add_argument("--page-posterior", action="store_true",
                    help="with --page: also write NAME.post per line, from the page's one lattice (not with --page-omit)")
    args = ap.parse_args(argv)
    if args.page_posterior and (not args.page or args.page_omit is not None):
        ap.error("--page-posterior goes with --page and the strict lattice: not with --page-omit")
    if args.page_confidence and (not args.page or args.page_omit is not None):
        ap.error("--page-confidence goes with --page and the strict lattice: not with --page-omit")
    if args.posterior and (args.omit is not None or args.page):
        ap.error("--posterior goes with the strict alignment of single lines: not with --omit or --page")
    if args.confidence and (args.omit is not None or args.page):
        ap.error("--confidence goes with the strict alignment of single lines: not with --omit or --page")
    if args.omit_confidence and (args.omit is None or args.page):
        ap.error("--omit-confidence goes with --omit on single lines: not without it, not with --page")
    from text_alignment_amd import forced, ocr
    if args.page:
        if args.omit is not None:
            sys.exit("--page has no omission through --omit: the price at page scope is --page-omit")
        if args.page_omit is not None:
            try:
                forced.omit_units(args.page_omit)
            except ValueError as e:
                sys.exit("--page-omit: %s" % e)
        return page(args, forced, ocr)
    if args.page_omit is not None:
        sys.exit("--page-omit goes with --page")
    if args.omit is not None:
        try:
            forced.omit_units(args.omit)
        except ValueError as e:
            sys.exit("--omit: %s" % e)
    pairs = [p for p in read_pairs(args.directory) if p[1]]
    if not pairs:
        sys.exit("no NAME.png + NAME.gt.txt pairs in %s" % args.directory)
    rec = forced._recognizer(args.model)
    written, omitted, lowest, worst, nearest = [], 0, None, None, None
    for img, text, png in pairs:                       # line by line: one bad text does not cost the others theirs
        try:
            if args.posterior:
                got = forced.align_lines(rec, [img], [text], want_run=True, confidence=args.confidence, posterior=True)
                ((chars, score),), run, (post,) = got[0], got[1], got[-1]
                conf = got[2][0] if args.confidence else None
            elif args.confidence:
                ((chars, score),), (conf,) = forced.align_lines(rec, [img], [text], confidence=True)
            elif args.omit_confidence:
                ((chars, score),), (conf,) = forced.align_lines(rec, [img], [text], omit=args.omit, omit_confidence=True)
            else:
                (chars, score), = forced.align_lines(rec, [img], [text], omit=args.omit)
        except ValueError as e:
            print("skipped %s: %s" % (png, e), file=sys.stderr)
            continue
        gone = [(k, c[0]) for k, c in enumerate(chars) if c[4] is None]
        if gone:
            print("%s: omitted %s" % (png, " ".join("%d:%r" % g for g in gone)), file=sys.stderr)
            omitted += len(gone)
        out = png[:-len(".png")] + ".llocs"
        with open(out, "w", encoding="utf-8") as f:
            f.write(ocr.llocs_text([(c[0], c[4]) for c in chars if c[4] is not None]))
        if args.confidence:
            with open(png[:-len(".png")] + ".conf", "w", encoding="utf-8") as f:
                f.write(conf_text(text, conf, forced))
            lowest = min(int(conf[:, 0].min()), lowest if lowest is not None else int(conf[:, 0].min()))
        if args.omit_confidence:
            absent = [c[4] is None for c in chars]
            with open(png[:-len(".png")] + ".conf", "w", encoding="utf-8") as f:
                f.write(conf_text(text, conf, forced, omitted=absent))
            for (c, _), a in zip(conf.tolist(), absent):
                if a:
                    nearest = c if nearest is None else max(nearest, c)
                else:
                    lowest = c if lowest is None else min(lowest, c)
        if args.posterior:
            with open(png[:-len(".png")] + ".post", "w", encoding="utf-8") as f:
                f.write(post_text(text, post))
            per_frame = post.loglik_bits / int(run["T"][0])
            print("%s: log2 P(text | line) %.3f bits per frame" % (png, per_frame))
            worst = per_frame if worst is None else min(worst, per_frame)
        written.append((out, score))
    if args.posterior:
        print("lowest log2 P(text | line) per frame %s" % ("none" if worst is None else "%.3f bits" % worst))
    if args.confidence:
        print("%d of %d lines written, lowest confidence %s" % (
            len(written), len(pairs), "none" if lowest is None else "%.3f bits" % forced.confidence_bits(lowest)))
    elif args.omit_confidence:
        bits = lambda c: "none" if c is None else "%.3f bits" % forced.confidence_bits(c)          # noqa: E731
        print("%d of %d lines written, %d characters omitted, lowest confidence of a present character %s, "
              "the omission nearest to 0 %s" % (len(written), len(pairs), omitted, bits(lowest), bits(nearest)))
    elif args.omit is None:
        print("%d of %d lines written" % (len(written), len(pairs)))
    else:
        print("%d of %d lines written, %d characters omitted" % (len(written), len(pairs), omitted))
    return written


def conf_text(text, conf, forced, at=0, omitted=None):
    """the rows of NAME.conf: character, confidence in bits (three decimals), the rival state's character (`~`: a blank).
    at: the rows are those of the characters text[at:at + len(conf)] (--page-confidence: a line's share of the page's
    text, the rival a state of the page's).  omitted (--omit-confidence): per row whether the path left the character
    out; such a row ends in a fourth field, `omitted`"""
    rows = []
    for k, (ch, (c, s)) in enumerate(zip(text[at:], conf)):
        rows.append("%s\t%.3f\t%s%s\n" % (ch, forced.confidence_bits(c), text[(int(s) - 1) // 2] if int(s) & 1 else "~",
                                          "\tomitted" if omitted is not None and omitted[k] else ""))
    return "".join(rows)


def post_text(text, post, at=0, upto=None):
    """the rows of NAME.post: character, posterior (four decimals), the rival state's character (`~`: a blank), its posterior.
    at, upto: the rows are those of the characters text[at:upto] (--page-posterior: a line's share of the page's text, the
    rival a state of the page's)"""
    rows = []
    for ch, p, s, r in zip(text[at:upto], post.posterior[at:upto], post.rival_state[at:upto], post.rival_posterior[at:upto]):
        rows.append("%s\t%.4f\t%s\t%.4f\n" % (ch, p, text[(int(s) - 1) // 2] if int(s) & 1 else "~", r))
    return "".join(rows)


def page(args, forced, ocr):
    """--page: every .png of the directory in name order against one text; returns ([(NAME.llocs, rows)], score)"""
    import numpy as np
    from PIL import Image
    names = sorted(f for f in os.listdir(args.directory) if f.endswith(".png"))
    if not names:
        sys.exit("no NAME.png line images in %s" % args.directory)
    with open(args.page, encoding="utf-8") as f:
        text = " ".join(f.read().split())
    images = [np.ascontiguousarray(np.array(Image.open(os.path.join(args.directory, n)).convert("L"), dtype=np.uint8)) for n in names]
    gone = []
    try:
        got = forced.align_page_lines(forced._recognizer(args.model), images, text, omit=args.page_omit,
                                      confidence=args.page_confidence, posterior=args.page_posterior,
                                      want_run=args.page_posterior)
        lines, score = got[:2]
        conf = got[2 + args.page_posterior] if args.page_confidence else None
        post = got[-1] if args.page_posterior else None
        if args.page_omit is not None:
            gone = got[2]
    except ValueError as e:
        sys.exit("%s: %s" % (args.directory, e))
    if gone:
        print("%s: omitted %s" % (args.directory, " ".join("%d:%r" % (i, text[i]) for i in gone)), file=sys.stderr)
    written, at = [], 0
    for name, chars in zip(names, lines):
        out = os.path.join(args.directory, name[:-len(".png")] + ".llocs")
        with open(out, "w", encoding="utf-8") as f:
            f.write(ocr.llocs_text([(c[0], c[4]) for c in chars]))
        if args.page_confidence:                         # the path is strict: a line holds the next len(chars) characters
            with open(out[:-len(".llocs")] + ".conf", "w", encoding="utf-8") as f:
                f.write(conf_text(text, conf[at:at + len(chars)], forced, at))
        if args.page_posterior:
            with open(out[:-len(".llocs")] + ".post", "w", encoding="utf-8") as f:
                f.write(post_text(text, post, at, at + len(chars)))
        at += len(chars)
        written.append((out, len(chars)))
    if args.page_posterior:
        frames = int(np.asarray(got[2]["T"]).sum())
        print("log2 P(text | page) %.3f bits per frame (%.3f bits on %d frames)"
              % (post.loglik_bits / frames, post.loglik_bits, frames))
    if args.page_confidence:
        print("%d characters on %d lines, score %d, lowest confidence %.3f bits"
              % (len(text), len(names), score, forced.confidence_bits(int(conf[:, 0].min()))))
    elif args.page_omit is None:
        print("%d characters on %d lines, score %d" % (len(text), len(names), score))
    else:
        print("%d characters on %d lines, %d omitted, score %d" % (len(text) - len(gone), len(names), len(gone), score))
    return written, score


if __name__ == "__main__":
    main()
