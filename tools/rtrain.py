"""Train a line model from a directory of NAME.png + NAME.gt.txt pairs -- the in-process counterpart of
`ocropus-rtrain` (reference README.md, "Training a New OCRopus model").

    python tools/rtrain.py DIR -o MODEL [--ntrain 100000] [--lrate 1e-4] [--savefreq 1000] [--load MODEL.pyrnn.gz]
                           [--distort 3.0 [--dsigma 10.0]] [--validate DIR [--valfreq K]]

Lines are drawn at random (seeded), one update per line as ocropy does (--lines-per-update B sums B lines' gradients
into one update: a departure from ocropy, see text_alignment_amd/train.py).  Every --savefreq updates the model is
written as MODEL-%08d.pyrnn.gz.  Images are read with PIL as greyscale strips (white background) and normalised on the
device.  --distort D turns on ocropy's random line distortion (`rdistort`: displacements of up to D pixels, smoothed
with sigma --dsigma), generated on the device before the normaliser (text_alignment_amd/augment.py; DESIGN.md section
14.4); it is off by default, and a run is reproducible from --seed.  --validate DIR scores the current weights on the
held-out pairs of DIR every --valfreq updates (default: --savefreq) on the device (text_alignment_amd/errs.py; DESIGN.md
section 14.5), prints the character error rate and keeps a copy of the best model so far as MODEL-best.pyrnn.gz;
tools/rerrs.py scores saved checkpoints afterwards.  Without --validate nothing of this happens.
"""
import argparse
import glob
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def read_pairs(directory):
    from PIL import Image
    pairs = []
    for gt in sorted(glob.glob(os.path.join(directory, "*.gt.txt"))):
        png = gt[:-len(".gt.txt")] + ".png"
        if not os.path.exists(png):
            continue
        with open(gt, encoding="utf-8") as f:
            text = f.read().strip("\n")
        pairs.append((np.ascontiguousarray(np.array(Image.open(png).convert("L"), dtype=np.uint8)), text, png))
    return pairs


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("directory")
    ap.add_argument("-o", "--output", required=True, help="model file prefix")
    ap.add_argument("--ntrain", type=int, default=100000, help="number of updates")
    ap.add_argument("--lrate", type=float, default=1e-4)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--savefreq", type=int, default=1000)
    ap.add_argument("--load", help="continue from this .pyrnn.gz")
    ap.add_argument("--lines-per-update", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--distort", type=float, default=None, help="maximal random displacement in pixels (off by default; rdistort's is 3.0)")
    ap.add_argument("--dsigma", type=float, default=10.0, help="smoothing sigma of the displacement fields in pixels")
    ap.add_argument("--validate", metavar="DIR", help="held-out NAME.png + NAME.gt.txt pairs to score the model on")
    ap.add_argument("--valfreq", type=int, default=None, help="updates between two validations (default: --savefreq)")
    args = ap.parse_args(argv)
    from text_alignment_amd import model_io, train
    pairs = read_pairs(args.directory)
    if not pairs:
        sys.exit("no NAME.png + NAME.gt.txt pairs in %s" % args.directory)
    held_out, best_cer = [], None
    if args.validate:
        held_out = read_pairs(args.validate)
        if not held_out:
            sys.exit("no NAME.png + NAME.gt.txt pairs in %s" % args.validate)
    valfreq = args.valfreq if args.valfreq else args.savefreq
    kw = dict(lrate=args.lrate, momentum=args.momentum, lines_per_update=args.lines_per_update, seed=args.seed,
              distort=args.distort, dsigma=args.dsigma)
    tr = (train.LineTrainer(model=model_io.load_pyrnn(args.load), **kw) if args.load
          else train.LineTrainer(charset=[t for _, t, _ in pairs], **kw))
    rng = np.random.default_rng(args.seed)
    B = args.lines_per_update
    for k in range(1, args.ntrain + 1):
        pick = rng.integers(0, len(pairs), size=B)
        try:
            res = tr.train([pairs[i][0] for i in pick], [pairs[i][1] for i in pick])
            print("%d %.4f %s | %s" % (k, res[0]["error"], pairs[pick[0]][1], res[0]["decoded"]))
        except ValueError as e:                         # a text that does not fit its line, a character --load's codec lacks
            print("%d skipped %s: %s" % (k, pairs[pick[0]][2], e))
        if k % args.savefreq == 0 or k == args.ntrain:
            path = "%s-%08d.pyrnn.gz" % (args.output, k)
            model_io.save_pyrnn(tr.model(), path)
            print("# saved", path)
        if held_out and (k % valfreq == 0 or k == args.ntrain):
            res = tr.evaluate([p[0] for p in held_out], [p[1] for p in held_out])
            print("# validation %d: %d errors in %d characters of %d lines, cer %.5f"
                  % (k, res["errors"], res["chars"], res["lines"], res["cer"]))
            if res["chars"] and (best_cer is None or res["cer"] < best_cer):
                best_cer = res["cer"]
                path = "%s-best.pyrnn.gz" % args.output
                model_io.save_pyrnn(tr.model(), path)
                print("# best so far, saved", path)


if __name__ == "__main__":
    main()
