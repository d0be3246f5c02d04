"""Time the chained span search (ta_nw_span_chain) beside the independent search (ta_nw_span_batch) on the same pages.

    python tools/span_chain_time.py [--repeats 10] [--out profiles/span_chain_time.json]

Per shape: HIP events around whole calls, the median of the repeats after a warm-up, both searches in this one process.
Shapes: one chain of 64 pages x 1 000 OCR tokens in a 50 000-token transcript, and 16 chains of 4 pages x 3 000 tokens
(a 12 500-token transcript each).  No ratio is promised: a chain is P dependent steps of one workgroup per chain, so the
first shape should cost about 64 times one page's latency (`chain_ms_per_step` beside `one_page_ms`, the independent
search of ONE page against the same transcript), where the independent search runs its 64 pages side by side.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("1 chain x 64 pages x 1000 in 50000", 1, 64, 50000, 1000),
          ("16 chains x 4 pages x 3000 in 12500", 16, 4, 12500, 3000)]
SYSTEM = [8, -12, -6, -6, -2, -2]


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
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "span_chain_time.json"))
    args = ap.parse_args()
    import torch
    from text_alignment_amd import textSeqCompare as tsc
    assert torch.cuda.is_available(), "needs the GPU"
    rng = np.random.RandomState(1)
    rows = []
    for name, nchains, npages, n, m in SHAPES:
        ts, page_lists = [], []
        for _ in range(nchains):
            t = rng.randint(0, 25, size=n).astype(np.int32)
            step = (n - m) // max(npages - 1, 1) if n > m else 0
            pages = []
            for p in range(npages):                        # the pages in reading order (overlapping where m > n / P)
                o = t[p * step:p * step + m].copy()
                flip = rng.randint(0, len(o), size=len(o) // 5)
                o[flip] = rng.randint(0, 25, size=len(flip))
                pages.append(o)
            ts.append(t)
            page_lists.append(pages)
        cells = float(nchains) * npages * n * m
        chain = tsc.SpanChainBatch(ts, page_lists, SYSTEM)
        chain_ms, chain_all = _median_ms(torch, chain.run, args.repeats)
        spans, totals = chain.results()
        alone = tsc.SpanBatch([ts[c] for c in range(nchains) for _ in range(npages)],
                              [o for pages in page_lists for o in pages], SYSTEM)
        alone_ms, alone_all = _median_ms(torch, alone.run, args.repeats)
        same = int((alone.results()[:, :2] == spans[:, :2]).all(axis=1).sum())
        one = tsc.SpanBatch([ts[0]], [page_lists[0][0]], SYSTEM)
        one_ms, one_all = _median_ms(torch, one.run, args.repeats)
        row = {"shape": name, "nchains": nchains, "pages_per_chain": npages, "n": n, "m": m, "cells": cells,
               "workspace_bytes": chain.ws_bytes,
               "chain_ms": round(chain_ms, 4), "chain_ms_all": chain_all, "chain_cells_per_s": cells / (chain_ms * 1e-3),
               "chain_ms_per_step": round(chain_ms / npages, 4),
               "independent_ms": round(alone_ms, 4), "independent_ms_all": alone_all,
               "one_page_ms": round(one_ms, 4), "one_page_ms_all": one_all,
               "chain_step_over_one_page": chain_ms / npages / one_ms,
               "pages_with_the_independent_span": same, "pages": nchains * npages}
        rows.append(row)
        print("%-40s chain %9.3f ms (%.3f per step)   independent %9.3f ms   one page %9.3f ms   step / one page %.2f"
              % (name, chain_ms, chain_ms / npages, alone_ms, one_ms, row["chain_step_over_one_page"]))
        del chain, alone, one
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "timing": "HIP events around whole calls, median after a warm-up", "system": SYSTEM, "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
