"""How close the training kernels are to the float64 checker (tests/train_ref.py) -- the quantities
tests/test_train_gpu.py and tests/test_train_edges_gpu.py bound.  Writes profiles/train_agreement.json.

    python tools/train_agreement.py [--out profiles/train_agreement.json]

Per compared array:
  ratio    = max|GPU - checker64| / max|checker32 - checker64|: against the checker's own float32 gap; a float32
             implementation sits near 1 (the spec batch only: the float32 checker is not finite on a saturated model)
  quotient = max|GPU - checker64| / max(noise64, 4 ulp of the largest reference magnitude), noise64 = max|checker64 -
             checker in long double|: against the float64 checker's own rounding; the tests require quotient <= 64
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
    import train_cases as C
    import train_ref as R
    from text_alignment_amd import ocr, train

    def flat(g):
        return ([("fwd " + k, g["fwd"][k]) for k in R.GATES + R.PEEPS] + [("rev " + k, g["rev"][k]) for k in R.GATES + R.PEEPS]
                + [("W2", g["W2"])])

    def entry(got, r64, r32, rld, **where):
        err, gap, ratio = R.closeness(got, r64, r32)
        noise = R.noise64(r64, rld)
        e = dict(where, error=err, float32_gap=gap, ratio=ratio, noise64=noise,
                 quotient=err / (R.bound64(r64, noise) / R.FACTOR64))
        return e
    fwd, rev, W2, codec, lines, texts, codes = R.spec_batch()
    tr = train.LineTrainer(model=ocr.LineModel(fwd, rev, W2, codec))
    out = {"aligned": [], "gradients": [], "updates20": []}
    for (al, probs), cs in zip(tr.align(lines, texts, want_probs=True), codes):
        out["aligned"].append(entry(al, R.ctc_align_targets(probs, cs), R.ctc_align_targets(probs, cs, dtype=np.float32),
                                    R.ctc_align_targets(probs, cs, dtype=np.longdouble), T=int(al.shape[0])))
    for g, xs, cs in zip(tr.gradients(lines, texts), lines, codes):
        r64, r32, rld = (R.gradients(fwd, rev, W2, xs, cs, dtype=dt) for dt in (np.float64, np.float32, np.longdouble))
        for (name, a), (_, b), (_, c), (_, e) in zip(flat(g), flat(r64), flat(r32), flat(rld)):
            out["gradients"].append(entry(a, b, c, e, T=int(xs.shape[0]), array=name))
    lengths = [40 + 8 * k for k in range(20)]
    _, _, _, _, lines, texts, codes = R.spec_batch(seed=32, lengths=lengths)
    tr = train.LineTrainer(model=ocr.LineModel(fwd, rev, W2, codec), lrate=1e-2, momentum=0.9)
    tr.train(lines, texts)
    cs3 = [R.Trainer(fwd, rev, W2, 1e-2, 0.9, dtype=dt) for dt in (np.float64, np.float32, np.longdouble)]
    for xs, cs in zip(lines, codes):
        for c in cs3:
            c.update([xs], [cs])
    m = tr.model()
    for (name, a), (_, b), (_, c), (_, e) in zip(flat({"fwd": m.fwd, "rev": m.rev, "W2": m.W2}),
                                                 *(flat({"fwd": c.fwd, "rev": c.rev, "W2": c.W2}) for c in cs3)):
        out["updates20"].append(entry(a, b, c, e, array=name))
    out["worst_ratio"] = {k: max(e["ratio"] for e in v) for k, v in out.items()}
    # the edge cases of tests/train_cases.py, as tests/test_train_edges_gpu.py compares them
    edges, missed = [], []

    def held(check, *a, **kw):                             # (a miss is recorded like everything else; the tests assert)
        try:
            check(*a, record=edges, **kw)
        except AssertionError as e:
            missed.append(str(e))
    for name, _, _ in C.lattice_cases():
        held(C.lattice_want(name).check, C.device_lattice(name), name)
    for name, _, _, _ in C.net_cases():
        for b, (w, g) in enumerate(zip(C.net_want(name), C.device_net(name))):
            held(w.check, g, "%s line %d" % (name, b))
    lib = C.bind(train._native.lib)
    no, three = C.three_lattice_lines()
    pk = C.pack_ctc(lib, three, no)
    d = C.Device(pk, C.CTC_INPUTS, C.CTC_OUTPUTS)
    assert C.call_ctc(lib, pk, d.ptr, d.stream()) == 0
    held(C.check_ctc, d.back(), pk, C.three_lattice_wants(), what="C ABI, three lines")
    for name, model, nlines, _ in C.net_cases():
        pk = C.pack_net(model, nlines, C.net_want(name))
        d = C.Device(pk, C.NET_INPUTS, C.NET_OUTPUTS)
        assert C.call_forward(lib, pk, d.ptr, d.stream()) == 0 and C.call_backward(lib, pk, d.ptr, d.stream()) == 0
        held(C.check_net, d.back(), pk, C.net_want(name), what="C ABI, " + name)
    out["edges"], out["missed"] = edges, missed
    out["worst_quotient"] = {k: max(e["quotient"] for e in out[k]) for k in ("aligned", "gradients", "updates20", "edges")}
    out["quotient_bound"] = R.FACTOR64
    out["note"] = ("ratio = max|GPU - float64 checker| / max|float32 checker - float64 checker|; quotient = max|GPU - "
                   "float64 checker| / max(noise64, 4 ulp of the largest reference magnitude), noise64 = max|float64 checker "
                   "- long-double checker| (tests/train_ref.py)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"worst_ratio": out["worst_ratio"], "worst_quotient": out["worst_quotient"]}))


if __name__ == "__main__":
    main()
