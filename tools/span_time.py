"""Time the span-locating fill (ta_nw_span_batch) beside the aligner's score-only fill on the same inputs.

    python tools/span_time.py [--repeats 7] [--out profiles/span_time.json]

Per shape: HIP events around whole launches, the median of the repeats, both kernels in this one process; cells/s and
the ratio span / score-only.  The score-only fill is NWBatch(two_phase=True).run(fill=True, traceback=False) -- phase 1
of the two-phase aligner, which carries no origins (and, with these inputs, keeps a score profile in LDS).
Shapes: 64 pages against one shared 50 000-token transcript (64 workgroups on 256 CUs: latency-shaped), 64 pages
against their own 3 000 tokens, and a chip-filling 1 024 x (2 048 x 2 048).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("64 x (50000 x 1000), one shared transcript", 64, 50000, 1000, True),
          ("64 x (3000 x 1000)", 64, 3000, 1000, False),
          ("1024 x (2048 x 2048)", 1024, 2048, 2048, False)]
SYSTEM = [8, -4, -7, -7, -3, 0]


def _median_ms(torch, launch, repeats):
    launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), [round(t, 4) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "span_time.json"))
    args = ap.parse_args()
    import torch
    from text_alignment_amd import textSeqCompare as tsc
    assert torch.cuda.is_available(), "needs the GPU"
    rng = np.random.RandomState(1)
    rows = []
    for name, nprob, n, m, shared in SHAPES:
        book = rng.randint(0, 25, size=n).astype(np.int32)
        t_list = [book] * nprob if shared else [rng.randint(0, 25, size=n).astype(np.int32) for _ in range(nprob)]
        o_list = []
        for k in range(nprob):
            a = int(rng.randint(0, max(n - m, 1)))
            o = t_list[k][a:a + m].copy()
            flip = rng.randint(0, len(o), size=len(o) // 5)
            o[flip] = rng.randint(0, 25, size=len(flip))
            o_list.append(o)
        cells = float(nprob) * n * m
        span = tsc.SpanBatch(t_list, o_list, SYSTEM)
        span_ms, span_all = _median_ms(torch, span.run, args.repeats)
        spans = span.results()
        fill = tsc.NWBatch([np.array(t) for t in t_list], o_list, SYSTEM, two_phase=True)
        fill_ms, fill_all = _median_ms(torch, lambda: fill.run(fill=True, traceback=False), args.repeats)
        row = {"shape": name, "nprob": nprob, "n": n, "m": m, "cells": cells, "uploaded_transcript_tokens": span.uploaded_tokens,
               "span_ms": round(span_ms, 4), "span_cells_per_s": cells / (span_ms * 1e-3), "span_ms_all": span_all,
               "score_fill_ms": round(fill_ms, 4), "score_fill_cells_per_s": cells / (fill_ms * 1e-3),
               "score_fill_ms_all": fill_all, "ratio_span_over_score_fill": span_ms / fill_ms,
               "median_span_length": float(np.median(spans[:, 1] - spans[:, 0]))}
        rows.append(row)
        print("%-46s span %9.3f ms (%.3g cells/s)   score-only fill %9.3f ms (%.3g cells/s)   ratio %.2f"
              % (name, span_ms, row["span_cells_per_s"], fill_ms, row["score_fill_cells_per_s"], row["ratio_span_over_score_fill"]))
        del span, fill
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "timing": "HIP events around whole launches, median",
           "system": SYSTEM, "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
