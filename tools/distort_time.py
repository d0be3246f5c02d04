"""What the line distortion costs: `augment.distort_strips` on 16 strips of 60 x 1400 at the
default parameters, the trainer's lines_per_update = 16 pass on the same raw strips with `distort` off and on, and the
numpy checker (tests/distort_ref.py) on one core for one strip.  HIP events around whole calls after a warm-up call,
median of the repeats.  Writes profiles/distort_time.json; no threshold is set here.

    python tools/distort_time.py [--repeats 7] [--out profiles/distort_time.json] [--no-cpu]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

H, W, LINES = 60, 1400, 16


def glyph_strip(rng, h, w):
    """dark blobs on a white strip, grey edges: enough ink for the normaliser to measure a band"""
    yy = np.arange(h)[:, None]
    dens = 0.6 * np.exp(-0.5 * ((yy - h / 2.0) / (h / 7.0)) ** 2) * ((np.arange(w)[None, :] // 23) % 3 > 0)
    ink = rng.random((h, w)) < dens
    return np.where(ink, rng.integers(0, 90, size=(h, w)), rng.integers(235, 256, size=(h, w))).astype(np.uint8)


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
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "distort_time.json"))
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    from text_alignment_amd import augment, train
    rng = np.random.default_rng(41)
    strips = [glyph_strip(rng, H, W) for _ in range(LINES)]
    texts = ["abcde" * 8] * LINES
    out = {"strips": [H, W, LINES], "distort": augment.DISTORT, "dsigma": augment.DSIGMA,
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats}
    out["distort_strips"] = timed(lambda: augment.distort_strips(strips), args.repeats)
    out["distort_strips"]["ms_per_strip"] = out["distort_strips"]["median_ms"] / LINES
    out["distort_strips"]["sha256_out"] = hashlib.sha256(augment.distort_strips(strips)[0].buffer.cpu().numpy().tobytes()).hexdigest()
    for name, distort in (("update_distort_off", None), ("update_distort_on", augment.DISTORT)):
        tr = train.LineTrainer(charset="abcde", lines_per_update=LINES, distort=distort, dsigma=augment.DSIGMA)
        out[name] = timed(lambda: tr.train(strips, texts), args.repeats)
    off, on = out["update_distort_off"]["median_ms"], out["update_distort_on"]["median_ms"]
    out["ratios"] = {"update_on_over_off": on / off, "distort_strips_over_update_off": out["distort_strips"]["median_ms"] / off}
    if not args.no_cpu:
        import distort_ref as R
        from threadpoolctl import threadpool_limits
        with threadpool_limits(limits=1):
            t0 = time.perf_counter()
            R.distort_strip(strips[0], augment.DISTORT, augment.DSIGMA, 0, 0)
            dt = time.perf_counter() - t0
        out["numpy_checker_one_core"] = {"s_per_strip": dt}
        out["ratios"]["checker_over_device_per_strip"] = dt * 1e3 / out["distort_strips"]["ms_per_strip"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != "ms"}) for k, v in out.items()}))


if __name__ == "__main__":
    main()
