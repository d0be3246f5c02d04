"""Updates per second of the line trainer at T ~ 1000, lines_per_update 1 and 16, against the float64 numpy checker on
one core (tests/train_ref.py).  HIP events around whole passes, median of the repeats.  Writes profiles/train_time.json.

    python tools/train_time.py [--repeats 7] [--out profiles/train_time.json] [--no-cpu]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_time.json"))
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    import train_ref as R
    from text_alignment_amd import ocr, train
    lengths = [1000 + 3 * k for k in range(16)]
    fwd, rev, W2, codec, lines, texts, codes = R.spec_batch(seed=41, no=96, lengths=lengths)
    out = {"T": lengths, "classes": 96, "device": torch.cuda.get_device_name(0), "repeats": args.repeats}
    for B in (1, 16):
        tr = train.LineTrainer(model=ocr.LineModel(fwd, rev, W2, codec), lines_per_update=B)
        tr.train(lines, texts)                                     # warm-up: allocator, code objects
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.train(lines, texts)                                 # 16 lines: 16 updates at B = 1, one at B = 16
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        out["lines_per_update_%d" % B] = {"pass_ms": ms, "median_ms": med, "lines_per_s": 16e3 / med,
                                          "updates_per_s": (16 // B) * 1e3 / med}
    if not args.no_cpu:
        from threadpoolctl import threadpool_limits
        c = R.Trainer(fwd, rev, W2)
        with threadpool_limits(limits=1):                          # one core: the BLAS under numpy kept to one thread
            t0 = time.perf_counter()
            for xs, cs in zip(lines[:2], codes[:2]):
                c.update([xs], [cs])
            dt = (time.perf_counter() - t0) / 2
        out["numpy_checker_one_core"] = {"s_per_update": dt, "updates_per_s": 1 / dt}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != "pass_ms"})
                      for k, v in out.items() if k != "T"}))


if __name__ == "__main__":
    main()
