"""How narrow may the LCS-bounded funnel run?  A CPU sweep that chooses kFunnelLcsScalePm (csrc/nw_band.h).

For each scale (per mille of the static funnel's rem-proportional widths) and each seed of the bench generator
(tools.synth.synth_pair_ids, the pairs bench.py aligns) the host-side replay of the LCS kernel and of the banded fill
(tests/native/sim_nw_funnel_lcs.cpp, built once per scale with -DTA_FUNNEL_LCS_SCALE_PM) gives the certificate's words
on BANDED values: v0, the exit word, U.  Margin = v0 - max(exit word, U).  The baseline is the static funnel's margin
from its own replay (tests/native/sim_nw_funnel.cpp).  Rule: the smallest scale at which every problem certifies and the
minimum margin stays at least half of the static funnel's minimum.

    python tools/funnel_lcs_estimate.py [--n 4096 --m 4096 --seeds 64 --scales 1000,800,600,500,400,300,200]
prints one JSON line per scale and the choice.  Nothing rests on the constant for correctness.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools.nw_configs import DEFAULT_SYS                    # noqa: E402
from tools.synth import synth_pair_ids                      # noqa: E402

BUILD = os.path.join(REPO, "tests", "native", "build")


def _build(stem, tag, flags):
    so = os.path.join(BUILD, "libest_%s_%s.so" % (stem, tag))
    src = os.path.join(REPO, "tests", "native", "sim_%s.cpp" % stem)
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(
            os.path.join(REPO, "text_alignment_amd", "csrc", "nw_band.h"))):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC"] + flags + ["-o", so, src])
    return so


def _band_w(n, m, system):
    """the outer band the plan gives this shape (host functions of the library; no GPU needed)"""
    from text_alignment_amd import _native
    n32, m32 = np.array([n], np.int32), np.array([m], np.int32)
    prm = np.array(system, np.int32)
    out = np.zeros(8, np.int32)
    flags = 28 << _native.TA_NW_ALPHABET_SHIFT | _native.TA_NW_OPENS_SAME
    rc = _native.lib.ta_nw2_band_plan(n32.ctypes.data, m32.ctypes.data, 1, prm.ctypes.data, 0, flags, 0, out.ctypes.data,
                                      None, None, 0)
    assert rc == 0
    return int(out[1])


def _one(args):
    so, static_so, n, m, seed, w = args
    t, o = synth_pair_ids(n, m, seed)
    t, o = np.ascontiguousarray(t, np.int32), np.ascontiguousarray(o, np.int32)
    p = np.array(DEFAULT_SYS, np.int32)
    if so is None:                                          # the static funnel's replay
        lib = ctypes.CDLL(static_so)
        lib.sim_nw2_funnel.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                                       ctypes.c_void_p, ctypes.c_void_p]
        info = np.zeros(8, np.int32)
        ops = np.zeros(n + m + 1, np.uint8)
        ln = ctypes.c_int(0)
        rc = lib.sim_nw2_funnel(t.ctypes.data, n, o.ctypes.data, m, p.ctypes.data, w, 2064, ops.ctypes.data,
                                ctypes.byref(ln), info.ctypes.data, None)
        assert rc == 0, rc
        return bool(info[0]), int(info[1]) - max(int(info[3]), int(info[2])), 0.0
    lib = ctypes.CDLL(so)
    lib.sim_nw2_funnel_lcs.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    info = np.zeros(10, np.int32)
    nstrips = (n + 255) // 256
    ranges = np.zeros(2 * nstrips, np.int32)
    rc = lib.sim_nw2_funnel_lcs(t.ctypes.data, n, o.ctypes.data, m, p.ctypes.data, w, 27, info.ctypes.data, None,
                                ranges.ctypes.data)
    assert rc == 0 and info[7] == 2 and info[8] == 1 and info[3] == info[5], (rc, info.tolist())
    groups = int((ranges[1::2] - ranges[0::2]).sum())
    return bool(info[0]), int(info[1]) - max(int(info[3]), int(info[2])), groups / float(nstrips * ((m + 63 + 3) // 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--first-seed", type=int, default=1234)
    ap.add_argument("--scales", default="1000,800,600,500,400,300,200")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    w = _band_w(a.n, a.m, DEFAULT_SYS)
    seeds = list(range(a.first_seed, a.first_seed + a.seeds))
    static_so = _build("nw_funnel", "static", [])
    rows = []
    with ProcessPoolExecutor(a.jobs) as ex:
        base = list(ex.map(_one, [(None, static_so, a.n, a.m, s, w) for s in seeds]))
        base_min = min(r[1] for r in base)
        print(json.dumps({"static_funnel": True, "w": w, "seeds": len(seeds), "certified": sum(r[0] for r in base),
                          "margin_min": base_min, "margin_mean": round(float(np.mean([r[1] for r in base])), 1)}), flush=True)
        for pm in [int(v) for v in a.scales.split(",")]:
            so = _build("nw_funnel_lcs", "pm%d" % pm, ["-DTA_FUNNEL_LCS_SCALE_PM=%d" % pm])
            res = list(ex.map(_one, [(so, None, a.n, a.m, s, w) for s in seeds]))
            row = {"scale_pm": pm, "share_of_groups": round(res[0][2], 4), "certified": sum(r[0] for r in res),
                   "margin_min": min(r[1] for r in res), "margin_mean": round(float(np.mean([r[1] for r in res])), 1)}
            row["qualifies"] = row["certified"] == len(seeds) and 2 * row["margin_min"] >= base_min
            rows.append(row)
            print(json.dumps(row), flush=True)
    ok = [r["scale_pm"] for r in rows if r["qualifies"]]
    print(json.dumps({"choice_scale_pm": min(ok) if ok else None, "rule": "all certify, margin_min >= half the static funnel's"}))


if __name__ == "__main__":
    main()
