"""Which problems of the benchmark's headline batch the banded fill has to fill again in full, and with what margin
the others certify -- outside timed code (it synchronises).  The batch is bench.py's: `distinct` problems
synth_pair_ids(n, m, 1234 + k), repeated up to nprob.
python tools/band_fallbacks.py [nprob] [n] [m]  ->  one JSON line"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.nw_configs import DEFAULT_SYS                    # noqa: E402
from tools.synth import synth_pair_ids                      # noqa: E402


def main():
    import torch
    from text_alignment_amd import textSeqCompare as tsc
    nprob = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    m = int(sys.argv[3]) if len(sys.argv) > 3 else n
    uniq = [synth_pair_ids(n, m, 1234 + k) for k in range(min(nprob, 256))]
    probs = [uniq[k % len(uniq)] for k in range(nprob)]
    batch = tsc.NWBatch([p[0] for p in probs], [p[1] for p in probs], DEFAULT_SYS, two_phase=True)
    batch.run()
    torch.cuda.synchronize()
    plan = batch.band_plan()
    row = {"problems": nprob, "n": n, "m": m, "w": plan["w"], "shape": plan.get("shape"), "share_of_groups": plan["share"],
           "uniform_share": plan.get("uniform_share"), "ranges": plan["ranges"], "fallbacks": batch.band_fallbacks()}
    cert = batch.band_certificate()
    if cert is not None:
        bound = np.maximum(cert[:, 1], plan["u"][:nprob])
        margin = cert[:, 0].astype(np.int64) - bound
        row.update(v0_min=int(cert[:, 0].min()), v0_max=int(cert[:, 0].max()), exit_max=int(cert[:, 1].max()),
                   exit0=int(plan["x0"][0]), u=int(plan["u"][0]), margin_min=int(margin.min()),
                   margin_mean=round(float(margin.mean()), 1), strips_counted=sorted(set(cert[:, 2].tolist())))
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
