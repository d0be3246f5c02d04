"""Score line-model checkpoints on held-out lines -- the in-process counterpart of `ocropus-errs` / `ocropus-econf`:
which of the MODEL-%08d.pyrnn.gz files that tools/rtrain.py wrote should `process` use?

    python tools/rerrs.py DIR MODEL [MODEL ...] [--kind exact|nospace] [--confusions N]

DIR holds NAME.png + NAME.gt.txt pairs the models were NOT trained on.  The strips are normalised once on the device;
every model recognises them and its decoded lines are compared with the ground truth there (text_alignment_amd/errs.py;
DESIGN.md section 14.5).  Prints one line per model -- errors, characters, character error rate, path -- then, with
--confusions N, the N most frequent confusions of each (count, what the model read, what the truth says; "_" = nothing,
"?" = a character the model's codec lacks), and the best model last.
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
    ap.add_argument("models", nargs="+")
    ap.add_argument("--kind", choices=("exact", "nospace"), default="exact", help="whitespace rule of the comparison")
    ap.add_argument("--confusions", type=int, default=0, metavar="N", help="print each model's N most frequent confusions")
    args = ap.parse_args(argv)
    from text_alignment_amd import errs
    pairs = read_pairs(args.directory)
    if not pairs:
        sys.exit("no NAME.png + NAME.gt.txt pairs in %s" % args.directory)
    lines, texts = [p[0] for p in pairs], [p[1] for p in pairs]
    results = errs.evaluate_models(args.models, lines, texts, kind=args.kind)
    best = None
    for path, res in zip(args.models, results):
        print("%8d %8d %9.5f %s" % (res["errors"], res["chars"], res["cer"], path))
        for count, got, want in res["confusions"][:args.confusions]:
            print("    %6d %-2s %-2s" % (count, got, want))
        if res["chars"] and (best is None or res["cer"] < best[0]):
            best = (res["cer"], path)
    if best is not None:
        print("# best %.5f %s" % best)
    return results


if __name__ == "__main__":
    main()
