"""Prices the banded fill's worst case and its plan: one batch of UNRELATED random pairs (every certificate fails, so
every problem is filled twice: the band's groups, then all of them) and one of related pairs, each timed with the band
as the plan chooses it (a funnel inside the rule's band), with the uniform band of the same width, and with the band off (device time of fill and traceback, median of 10 after 3 warm-ups).
python tools/band_worst_case.py [nprob] [n]  ->  one JSON line per batch"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.nw_configs import DEFAULT_SYS, time_batch      # noqa: E402
from tools.synth import synth_pair_ids                     # noqa: E402


def main():
    import torch
    from text_alignment_amd import textSeqCompare as tsc
    nprob = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    rng = np.random.default_rng(77)
    unrelated = [(rng.integers(0, 27, n).astype(np.int32), rng.integers(0, 27, n).astype(np.int32)) for _ in range(64)]
    related = [synth_pair_ids(n, n, 1234 + k) for k in range(64)]
    for name, uniq in (("unrelated", unrelated), ("related", related)):
        probs = [uniq[k % len(uniq)] for k in range(nprob)]
        row = {"batch": name, "problems": nprob, "n": n, "m": n}
        outs = {}
        for key, band, shape in (("band_auto", 0, "auto"), ("band_uniform", 0, "uniform"), ("band_off", 1, "auto")):
            batch = tsc.NWBatch([p[0] for p in probs], [p[1] for p in probs], DEFAULT_SYS, two_phase=True)
            batch.band = band
            batch.band_shape = shape
            total, fill, tb = time_batch(torch, batch)
            plan = batch.band_plan()
            row[key] = {"ms": round(total, 4), "fill_ms": round(fill, 4), "traceback_ms": round(tb, 4), "w": plan["w"],
                        "shape": plan["shape"], "share_of_groups": plan["share"], "fallbacks": len(batch.band_fallbacks())}
            outs[key] = batch.results()
            del batch
            torch.cuda.empty_cache()
        row["same_alignments"] = all(a.tolist() == b.tolist() == c.tolist()
                                     for a, b, c in zip(outs["band_auto"], outs["band_uniform"], outs["band_off"]))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
