"""What held-out scoring costs: `errs.evaluate` on 1 920 synthetic lines (the shape of bench.py's
OCR leg: 48 x W', W' ~ U[800, 2000], a random 96-class model, texts of 20 .. 200 characters) against the same
recogniser pass without the scoring step, the scoring call alone on the resident decoder output, and the host route
-- `decoded()` plus the plain-Python checker tests/errs_ref.py on one core (timed on the first --cpu-lines lines and
scaled).  HIP events around whole calls after a warm-up call, median of the repeats.  Writes profiles/errs_time.json;
no threshold is set here.

    python tools/errs_time.py [--lines 1920] [--repeats 7] [--cpu-lines 96] [--out profiles/errs_time.json]
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


def synthetic_lines(nlines, seed):
    """already-normalised lines (T, 48), T - 32 ~ U[800, 2000], as bench.py's OCR leg draws them"""
    rng = np.random.default_rng(seed)
    lines = []
    for _ in range(nlines):
        w = int(rng.integers(800, 2001))
        xs = np.zeros((w + 32, 48), dtype=np.float32)
        xs[16:16 + w] = (rng.random((w, 48)) < 0.15) * rng.random((w, 48))
        lines.append(xs)
    return lines


def timed(fn, repeats):
    import torch
    fn()                                                           # warm-up: allocator, code objects
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms": ms, "median_ms": statistics.median(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1920)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cpu-lines", type=int, default=96, help="lines the host route is timed on (0: skip it)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "errs_time.json"))
    args = ap.parse_args()
    import torch
    from text_alignment_amd import errs, ocr
    model = ocr.LineModel.random(7001, no=96)
    rec = ocr.LineRecognizer(model)
    lines = synthetic_lines(args.lines, 8000)
    rng = np.random.default_rng(9)
    letters = [c for c in model.codec if c]
    texts = ["".join(rng.choice(letters, size=int(rng.integers(20, 201)))) for _ in range(args.lines)]
    targets = [errs.encode_target(model.codec, t) for t in texts]
    out = {"lines": args.lines, "classes": model.no, "precision": ocr.DEFAULT_PRECISION,
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats}

    def recognise_only():
        st = rec.prepare(lines)
        rec.run(st)
        rec.check_status(st["dec_n"].cpu().numpy())                # the download evaluate() ends with, without the scorer
        return st
    res = errs.evaluate(rec, lines, texts)
    out["result"] = {k: res[k] for k in ("errors", "chars", "lines", "cer")}
    out["decoded_characters"] = int(res["per_line"][:, 1].sum())
    out["evaluate"] = timed(lambda: errs.evaluate(rec, lines, texts), args.repeats)
    out["recognise_only"] = timed(recognise_only, args.repeats)
    st = recognise_only()
    out["score_decoded"] = timed(lambda: errs.score_decoded(st["dec_c"], st["row_off"], st["dec_n"], st["T_host"], targets,
                                                            model.no), args.repeats)
    out["ratios"] = {"evaluate_over_recognise_only": out["evaluate"]["median_ms"] / out["recognise_only"]["median_ms"],
                     "score_decoded_over_recognise_only": out["score_decoded"]["median_ms"] / out["recognise_only"]["median_ms"]}
    if args.cpu_lines > 0:
        import errs_ref as R
        k = min(args.cpu_lines, args.lines)
        t0 = time.perf_counter()
        dec = rec.decoded(st)
        t1 = time.perf_counter()
        per, _ = R.score([[c for _, c in d] for d in dec[:k]], [R.encode_target(model.codec, t) for t in texts[:k]], model.no + 1)
        t2 = time.perf_counter()
        assert np.array_equal(per, res["per_line"][:k])
        cells = int((res["per_line"][:, 1].astype(np.int64) * res["per_line"][:, 2]).sum())
        cells_k = int((per[:, 1].astype(np.int64) * per[:, 2]).sum())
        scaled = (t2 - t1) * cells / max(cells_k, 1)
        out["host_route_one_core"] = {"decoded_s": t1 - t0, "checker_lines": k, "checker_s": t2 - t1,
                                      "checker_s_scaled_to_all_lines_by_cells": scaled}
        out["ratios"]["host_route_over_score_decoded"] = (t1 - t0 + scaled) * 1e3 / out["score_decoded"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != "ms"}) for k, v in out.items()}))


if __name__ == "__main__":
    main()
