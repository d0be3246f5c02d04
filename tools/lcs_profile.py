"""Where nw_lcs_suffix_kernel's time goes: a build with -DTA_LCS_PROFILE=1 leaves per-problem counter ticks (mask
set-up, the steps, the stores with their schedule's advance, the chunk tail: feed reload and column 0) in the spare
words behind each problem's edge counts.  Printed for two batch sizes: at the larger one the waves share their SIMDs,
at the smaller every wave has a SIMD to itself, so its ticks per step are the lone wave's.
Build:  hipcc ... -DTA_LCS_PROFILE=1 -c ta_nw2.hip, linked with the other objects into a library of its own;
run with TA_HIP_LIB=<that .so>:  python tools/lcs_profile.py [nprob] [nprob_lone] [n] [m]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from text_alignment_amd import textSeqCompare as tsc
from tools.nw_configs import DEFAULT_SYS
from tools.synth import synth_pair_ids

nprob = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
nprob_lone = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
n = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
m = int(sys.argv[4]) if len(sys.argv) > 4 else 4096
uniq = [synth_pair_ids(n, m, 1234 + k) for k in range(16)]


def profile(count):
    batch = tsc.NWBatch([uniq[k % 16][0] for k in range(count)], [uniq[k % 16][1] for k in range(count)], DEFAULT_SYS,
                        two_phase=True)
    batch.run()
    torch.cuda.synchronize()
    plan = batch.band_plan()
    if not plan.get("lcs"):
        sys.exit("the plan of %d x %d x %d does not run the LCS-bounded funnel" % (count, n, m))
    stride = ((n + 1 + 63) & ~63) + 192 * ((n + 255) // 256)
    spare = 64 * ((n + 255) // 256)
    tab = plan["lcs_dev"].cpu().numpy()[:count * stride].reshape(count, stride)
    c = tab[:, spare:spare + 8].copy().view(np.int64).astype(np.float64)
    setup, steps, stores, tail = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    tot = setup + steps + stores + tail
    nsteps = 64 * ((n + 63 + 63) // 64)
    print("%d problems of %d x %d: counter ticks per wave %.0f (min %.0f, max %.0f), %.2f per step of %d"
          % (count, n, m, tot.mean(), tot.min(), tot.max(), tot.mean() / nsteps, nsteps))
    for name, v in (("mask set-up", setup), ("steps", steps), ("stores + advance", stores), ("chunk tail", tail)):
        print("  %-18s %10.0f ticks  %5.1f %%" % (name, v.mean(), 100 * v.sum() / tot.sum()))
    return tot.mean()


a = profile(nprob)
b = profile(nprob_lone)
print("wave's total at %d problems against %d: x %.2f" % (nprob, nprob_lone, a / b))
