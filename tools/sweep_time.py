#!/usr/bin/env python3
"""tools/sweep_time.py -- wall and device time of ONE evaluate_text_alignment.sweep call over the reference's whole
grid search: 3 seeded pages of ~1 000 characters x the 729 scoring systems (2 187 NW problems), one JSON line.

    python tools/sweep_time.py [--runs 10] [--warmup 2]

Fields: wall ms of `sweep` (median of --runs after --warmup), device ms of the NW step and of each evaluation kernel
(events on the sweep's stream, from the median run's neighbour: one extra timed call), host ms that does not depend
on the scoring system (abbreviations, syllables, spans, representatives, candidates) and of the per-row means, and
the CPU figure the sweep replaces: the reference's NW rate (bench.py's cpu_baseline leg, the record under profiles/)
times the sweep's DP cells -- the reference's evaluation itself (box IOUs) is not counted in that figure.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BENCH_RECORD = os.path.join(REPO, "profiles", "r06_bench_run.json")


def pages():
    from text_alignment_amd import evaluate_text_alignment as eta
    from text_alignment_amd import latinSyllabification as latsyl
    from text_alignment_amd.alignToOCR import CharBox
    from tools.gen_golden_eval import make_page
    out = []
    for seed, angle, img_dim in [(9201, 0, (560, 4300)), (9202, 0.35, (600, 4340)), (9203, -0.4, (580, 4324))]:
        pg, ink = make_page(seed, angle, img_dim, (560, 4300), latsyl, length=950)
        chars = [CharBox(c, tuple(ul), tuple(lr)) for c, ul, lr in pg["chars"]]
        gt = [{"syl": g["syl"], "difficult": g["difficult"], "ul": tuple(g["box"][:2]), "lr": tuple(g["box"][2:])}
              for g in pg["gt"]]
        out.append(eta.SweepPage(chars, pg["transcript"], gt, angle, img_dim, (560, 4300), ink))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    from text_alignment_amd import evaluate_text_alignment as eta
    pg = pages()
    for _ in range(args.warmup):
        eta.sweep(pg)
    torch.cuda.synchronize()
    walls = []
    for _ in range(args.runs):
        for p in pg:                    # the system-independent host work is part of every call
            p._prep = None
        t0 = time.perf_counter()
        res = eta.sweep(pg)
        walls.append(1e3 * (time.perf_counter() - t0))
    tm = {}
    for p in pg:
        p._prep = None
    res = eta.sweep(pg, timings=tm)
    cells = int(res.batch.cells)
    ref_rate = None
    try:
        with open(BENCH_RECORD) as f:
            ref_rate = json.load(f)["cpu_baseline"]["value"]
    except (OSError, KeyError, ValueError):
        pass
    out = {"metric": "sweep_wall_ms", "value": float(np.median(walls)), "unit": "ms",
           "pages": len(pg), "systems": int(len(res.systems)), "problems": int(res.batch.nprob),
           "transcript_chars": [len(p.transcript) for p in pg], "dp_cells": cells,
           "wall_ms_runs": [round(w, 3) for w in walls],
           "device_ms": {"nw": tm["nw_ms"], "ta_eval_integral": tm["integral_ms"],
                         "ta_eval_syllable_boxes": tm["boxes_ms"], "ta_eval_score": tm["score_ms"]},
           "host_ms": {"system_independent": tm["host_prep_ms"], "per_row_means": tm["host_means_ms"]},
           "two_phase": bool(res.batch.two_phase), "nan_rows": int(np.isnan(res.area).sum()),
           "best": list(res.ranking()[-1][0]), "best_score": res.ranking()[-1][1]}
    if ref_rate:
        out["reference_cpu"] = {"nw_cells_per_s": ref_rate, "source": os.path.relpath(BENCH_RECORD, REPO),
                                "nw_seconds": cells / ref_rate, "nw_hours": cells / ref_rate / 3600.0,
                                "speedup_vs_wall": cells / ref_rate / (out["value"] * 1e-3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
