"""How close the training kernels are to the float64 checker, relative to the checker's own float32-versus-float64 gap
(tests/train_ref.py) -- the quantity tests/test_train_gpu.py bounds.  Writes profiles/train_agreement.json.

    python tools/train_agreement.py [--out profiles/train_agreement.json]

ratio = max|GPU - checker64| / max|checker32 - checker64| per compared array; a float32 implementation sits near 1.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_agreement.json"))
    args = ap.parse_args()
    import train_ref as R
    from text_alignment_amd import ocr, train

    def flat(g):
        return ([("fwd " + k, g["fwd"][k]) for k in R.GATES + R.PEEPS] + [("rev " + k, g["rev"][k]) for k in R.GATES + R.PEEPS]
                + [("W2", g["W2"])])
    fwd, rev, W2, codec, lines, texts, codes = R.spec_batch()
    tr = train.LineTrainer(model=ocr.LineModel(fwd, rev, W2, codec))
    out = {"aligned": [], "gradients": [], "updates20": []}
    for (al, probs), cs in zip(tr.align(lines, texts, want_probs=True), codes):
        err, gap, ratio = R.closeness(al, R.ctc_align_targets(probs, cs), R.ctc_align_targets(probs, cs, dtype=np.float32))
        out["aligned"].append({"T": int(al.shape[0]), "error": err, "float32_gap": gap, "ratio": ratio})
    for g, xs, cs in zip(tr.gradients(lines, texts), lines, codes):
        r64, r32 = R.gradients(fwd, rev, W2, xs, cs), R.gradients(fwd, rev, W2, xs, cs, dtype=np.float32)
        for (name, a), (_, b), (_, c) in zip(flat(g), flat(r64), flat(r32)):
            err, gap, ratio = R.closeness(a, b, c)
            out["gradients"].append({"T": int(xs.shape[0]), "array": name, "error": err, "float32_gap": gap, "ratio": ratio})
    lengths = [40 + 8 * k for k in range(20)]
    _, _, _, _, lines, texts, codes = R.spec_batch(seed=32, lengths=lengths)
    tr = train.LineTrainer(model=ocr.LineModel(fwd, rev, W2, codec), lrate=1e-2, momentum=0.9)
    tr.train(lines, texts)
    c64, c32 = R.Trainer(fwd, rev, W2, 1e-2, 0.9), R.Trainer(fwd, rev, W2, 1e-2, 0.9, dtype=np.float32)
    for xs, cs in zip(lines, codes):
        c64.update([xs], [cs])
        c32.update([xs], [cs])
    m = tr.model()
    for (name, a), (_, b), (_, c) in zip(flat({"fwd": m.fwd, "rev": m.rev, "W2": m.W2}),
                                         flat({"fwd": c64.fwd, "rev": c64.rev, "W2": c64.W2}),
                                         flat({"fwd": c32.fwd, "rev": c32.rev, "W2": c32.W2})):
        err, gap, ratio = R.closeness(a, b, c)
        out["updates20"].append({"array": name, "error": err, "float32_gap": gap, "ratio": ratio})
    out["worst_ratio"] = {k: max(e["ratio"] for e in v) for k, v in out.items()}
    out["note"] = "ratio = max|GPU - float64 checker| / max|float32 checker - float64 checker| (tests/train_ref.py)"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["worst_ratio"]))


if __name__ == "__main__":
    main()
