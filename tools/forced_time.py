"""What forced alignment costs, on a real MI355X:

(a) `ta_forced_align` alone on the benchmark's 1 920 synthetic lines (bench.synthetic_lines: 800 .. 2000 columns) with
    random texts of ~60 characters, HIP events around the call on resident probabilities, beside the recogniser's own
    time (LineRecognizer.run: recurrence, output layer, decode) for the same lines in the same run;
(b) `forced.refine_pages` against `harvest.harvest_pages` on the same 64 synthetic pages (tools/harvest_time.py's), wall
    milliseconds.
Medians of --passes repeats after a warm-up each.  Writes profiles/forced_time.json; no threshold is set here.  The
model is random, so in (b) nearly every line is rejected and refine_pages aligns next to none: (b) shows what keeping the
probabilities costs, (a) what aligning every line would.

    python tools/forced_time.py [--lines 1920] [--pages 64] [--passes 10] [--out profiles/forced_time.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1920)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "forced_time.json"))
    args = ap.parse_args()
    import torch
    import bench
    from text_alignment_amd import forced, harvest, ocr
    from tools.harvest_time import synthetic_pages
    model = ocr.LineModel.random(7001, no=96)
    rec = ocr.LineRecognizer(model)
    out = {"device": torch.cuda.get_device_name(0), "precision": ocr.DEFAULT_PRECISION, "passes": args.passes}

    def events(fn):
        ms = []
        for k in range(args.passes + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if k:
                ms.append(e0.elapsed_time(e1))
        return {"ms": ms, "median_ms": statistics.median(ms)}

    # ---- (a) the kernel beside the recogniser ------------------------------------------------------------------------------
    lines = bench.synthetic_lines(args.lines, 20250)
    rng = np.random.default_rng(9)
    L = rng.integers(50, 71, size=args.lines)
    labels = rng.integers(1, model.no, size=int(L.sum())).astype(np.int32)
    lab_off = np.concatenate([[0], np.cumsum(L)[:-1]])
    st = rec.prepare(lines)
    rec.run(st, want_probs=True)
    torch.cuda.synchronize()
    T, row_off = np.asarray(st["T_host"])[:args.lines], np.asarray(st["row_start_host"])[:args.lines]
    d_labels = torch.from_numpy(labels).to(rec.device)
    kept = {}

    def align():
        kept["got"] = forced.forced_alignment(st["probs"], row_off, T, d_labels, lab_off, L)
    out["a"] = {"lines": args.lines, "timesteps": int(T.sum()), "labels": int(L.sum()),
                "recogniser": events(lambda: rec.run(st)), "forced_alignment": events(align)}
    assert int(kept["got"][2].cpu().numpy().max()) == 0
    out["a"]["ratio_to_recogniser"] = out["a"]["forced_alignment"]["median_ms"] / out["a"]["recogniser"]["median_ms"]
    del st, kept["got"]

    # ---- (b) refine_pages against harvest_pages ------------------------------------------------------------------------------
    pages, trs = synthetic_pages(args.pages, 20, 4100)
    params = [8, -1, -9, -9, -4, -4]

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.passes):
            t0 = time.perf_counter()
            kept["res"] = fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        return {"ms": ms, "median_ms": statistics.median(ms)}
    out["b"] = {"pages": args.pages, "lines_per_page": 20,
                "harvest_pages": wall(lambda: harvest.harvest_pages(pages, trs, rec, params, 0.9)),
                "refine_pages": wall(lambda: forced.refine_pages(pages, trs, rec, params, 0.9))}
    out["b"]["difference_ms"] = out["b"]["refine_pages"]["median_ms"] - out["b"]["harvest_pages"]["median_ms"]
    out["b"]["refined_lines_of_this_noise_model"] = int(np.sum(kept["res"].refined))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    strip = lambda d: {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "ms"}     # noqa: E731
    print(json.dumps(strip(out)))


if __name__ == "__main__":
    main()
