"""What the sum-product posteriors cost beside the alignment and the max-marginal confidence, on
a real MI355X: `ta_forced_align`, `ta_forced_confidence` and `ta_forced_posterior` on the benchmark's 1 920 synthetic lines
(bench.synthetic_lines: 800 .. 2000 columns) with random texts of 50 .. 70 characters -- tools/forced_conf_time.py's lines,
texts and method: HIP events around the three C entry points alone, on resident probabilities and arguments that already
lie on the device, all in the same run, confidence and posterior queried at the alignment's own t_peak.  Medians of
--passes repeats after a warm-up each, and their ratios.  Writes profiles/forced_post_time.json; no threshold is set here.

    python tools/forced_post_time.py [--lines 1920] [--passes 10] [--out profiles/forced_post_time.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1920)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "forced_post_time.json"))
    args = ap.parse_args()
    import torch
    import bench
    from text_alignment_amd import _native, forced, ocr
    model = ocr.LineModel.random(7001, no=96)
    rec = ocr.LineRecognizer(model)

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

    lines = bench.synthetic_lines(args.lines, 20250)
    rng = np.random.default_rng(9)
    L = rng.integers(50, 71, size=args.lines)
    labels = rng.integers(1, model.no, size=int(L.sum())).astype(np.int32)
    lab_off = np.concatenate([[0], np.cumsum(L)[:-1]]).astype(np.int64)
    st = rec.prepare(lines)
    rec.run(st, want_probs=True)
    torch.cuda.synchronize()
    T, row_off = np.asarray(st["T_host"])[:args.lines], np.asarray(st["row_start_host"])[:args.lines]
    lib = _native.lib
    names = ("forced", "forced_confidence", "forced_posterior")
    size_of = {n: getattr(lib, "ta_%s_workspace_bytes" % n) for n in names}

    def pieces(f):
        size = np.asarray([f(int(t), int(l)) for t, l in zip(T, L)], dtype=np.int64)
        return np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64), int(size.sum())
    T32, L32 = np.ascontiguousarray(T, dtype=np.int32), np.ascontiguousarray(L, dtype=np.int32)
    off = {n: pieces(size_of[n]) for n in names}
    d = _native.upload_packed([np.ascontiguousarray(row_off, dtype=np.int64), T32, lab_off, L32, labels] +
                              [off[n][0] for n in names], rec.device)
    d_off = dict(zip(names, d[5:]))
    dev = dict(device=rec.device)
    new = lambda n, dt: torch.empty(n, dtype=dt, **dev)                                            # noqa: E731
    work = {n: new(off[n][1], torch.uint8) for n in names}
    nlab, nl = len(labels), args.lines
    frames, score = torch.empty((nlab, 3), dtype=torch.int32, **dev), new(nl, torch.int64)
    conf, rival = new(nlab, torch.int64), new(nlab, torch.int32)
    post = [new(nlab, torch.float64), new(nlab, torch.int32), new(nlab, torch.float64), new(nlab, torch.int32),
            new(nlab, torch.int32), new(nl, torch.float64), new(nl, torch.int32)]
    status = {n: new(nl, torch.int32) for n in names}
    probs = st["probs"]
    p = lambda t: t.data_ptr()                                                                     # noqa: E731
    head = (p(probs), p(d[0]), p(d[1]), p(d[4]), p(d[2]), p(d[3]))
    sizes = (nl, int(probs.shape[1]), int(probs.shape[0]), nlab, T32.ctypes.data, L32.ctypes.data)
    stream = torch.cuda.current_stream(rec.device).cuda_stream

    def tail(n, outs):
        return sizes + (p(work[n]), off[n][1]) + tuple(p(o) for o in outs) + (p(status[n]), stream)

    def align():
        _native.check(lib.ta_forced_align(*(head + (p(d_off["forced"]),) + tail("forced", [frames, score]))), "ta_forced_align")
    align()
    t_peak = frames[:, 2].contiguous()

    def confidence():
        _native.check(lib.ta_forced_confidence(*(head + (p(d_off["forced_confidence"]), p(t_peak)) +
                                                 tail("forced_confidence", [conf, rival]))), "ta_forced_confidence")

    def posterior():
        _native.check(lib.ta_forced_posterior(*(head + (p(d_off["forced_posterior"]), p(t_peak)) +
                                                tail("forced_posterior", post))), "ta_forced_posterior")
    out = {"device": torch.cuda.get_device_name(0), "precision": ocr.DEFAULT_PRECISION, "passes": args.passes,
           "lines": nl, "timesteps": int(T.sum()), "labels": nlab,
           "workspace_bytes": {"forced_alignment": off["forced"][1], "forced_confidence": off["forced_confidence"][1],
                               "forced_posterior": off["forced_posterior"][1]},
           "kernels": {"forced_alignment": events(align), "forced_confidence": events(confidence),
                       "forced_posterior": events(posterior)}}
    k = out["kernels"]
    k["ratio_posterior_to_alignment"] = k["forced_posterior"]["median_ms"] / k["forced_alignment"]["median_ms"]
    k["ratio_posterior_to_confidence"] = k["forced_posterior"]["median_ms"] / k["forced_confidence"]["median_ms"]
    assert all(int(s.cpu().numpy().max()) == 0 for s in status.values())
    # at the peaks: the posterior is positive and at most one, the max-marginal confidence never negative
    got = {name: t.cpu().numpy() for name, t in zip(forced.POSTERIOR_OUTPUTS, post)}
    value = forced.posterior_values(got["own_m"], got["own_x"], np.repeat(got["z_m"], L), np.repeat(got["z_x"], L))
    assert (value > 0).all() and (value <= 1 + 1e-11).all() and int(conf.cpu().numpy().min()) >= 0
    out["loglik_bits_per_frame_mean"] = float((forced.loglik_bits(got["z_m"], got["z_x"]) / T).mean())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    strip = lambda d: {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "ms"}     # noqa: E731
    print(json.dumps(strip(out)))


if __name__ == "__main__":
    main()
