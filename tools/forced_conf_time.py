"""What the per-character confidence costs beside the alignment it belongs to, on a real MI355X:
`ta_forced_align` and `ta_forced_confidence` on the benchmark's 1 920 synthetic lines (bench.synthetic_lines: 800 .. 2000
columns) with random texts of 50 .. 70 characters -- tools/forced_time.py's lines and texts -- HIP events around each call
on resident probabilities, both in the same run, the confidence queried at the alignment's own t_peak.  Medians of
--passes repeats after a warm-up each, and their ratio -- once around the Python calls (forced.forced_alignment /
forced.forced_confidence: workspace sizing, one packed upload and the launch, what tools/forced_time.py times) and once
around the two C entry points alone on arguments that already lie on the device ("kernels").  Writes
profiles/forced_conf_time.json; no threshold is set here.

    python tools/forced_conf_time.py [--lines 1920] [--passes 10] [--out profiles/forced_conf_time.json]
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "forced_conf_time.json"))
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
    lab_off = np.concatenate([[0], np.cumsum(L)[:-1]])
    st = rec.prepare(lines)
    rec.run(st, want_probs=True)
    torch.cuda.synchronize()
    T, row_off = np.asarray(st["T_host"])[:args.lines], np.asarray(st["row_start_host"])[:args.lines]
    d_labels = torch.from_numpy(labels).to(rec.device)
    kept = {}

    def align():
        kept["align"] = forced.forced_alignment(st["probs"], row_off, T, d_labels, lab_off, L)
    align()
    assert int(kept["align"][2].cpu().numpy().max()) == 0
    t_peak = kept["align"][0][:, 2].contiguous()

    def confidence():
        kept["conf"] = forced.forced_confidence(st["probs"], row_off, T, d_labels, lab_off, L, t_peak)
    lib = _native.lib
    out = {"device": torch.cuda.get_device_name(0), "precision": ocr.DEFAULT_PRECISION, "passes": args.passes,
           "lines": args.lines, "timesteps": int(T.sum()), "labels": int(L.sum()),
           "workspace_bytes": {"forced_alignment": int(sum(lib.ta_forced_workspace_bytes(int(t), int(l)) for t, l in zip(T, L))),
                               "forced_confidence": int(sum(lib.ta_forced_confidence_workspace_bytes(int(t), int(l))
                                                            for t, l in zip(T, L)))},
           "forced_alignment": events(align), "forced_confidence": events(confidence)}
    # ---- the launches alone: every argument uploaded and both workspaces allocated before the clock starts ----------------
    def pieces(size_of):
        size = np.asarray([size_of(int(t), int(l)) for t, l in zip(T, L)], dtype=np.int64)
        return np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64), int(size.sum())
    T32, L32 = np.ascontiguousarray(T, dtype=np.int32), np.ascontiguousarray(L, dtype=np.int32)
    (off_a, bytes_a), (off_c, bytes_c) = pieces(lib.ta_forced_workspace_bytes), pieces(lib.ta_forced_confidence_workspace_bytes)
    d = _native.upload_packed([np.ascontiguousarray(row_off, dtype=np.int64), T32, lab_off.astype(np.int64), L32, off_a, off_c],
                              rec.device)
    dev = dict(device=rec.device)
    work_a = torch.empty(bytes_a, dtype=torch.uint8, **dev)
    work_c = torch.empty(bytes_c, dtype=torch.uint8, **dev)
    frames = torch.empty((len(labels), 3), dtype=torch.int32, **dev)
    score = torch.empty(args.lines, dtype=torch.int64, **dev)
    conf_k = torch.empty(len(labels), dtype=torch.int64, **dev)
    rival_k = torch.empty(len(labels), dtype=torch.int32, **dev)
    status_k = torch.empty(args.lines, dtype=torch.int32, **dev)
    probs = st["probs"]
    p = lambda t: t.data_ptr()                                                                     # noqa: E731
    head = (p(probs), p(d[0]), p(d[1]), p(d_labels), p(d[2]), p(d[3]))
    sizes = (args.lines, int(probs.shape[1]), int(probs.shape[0]), len(labels), T32.ctypes.data, L32.ctypes.data)
    stream = torch.cuda.current_stream(rec.device).cuda_stream

    def align_kernel():
        _native.check(lib.ta_forced_align(*(head + (p(d[4]),) + sizes + (p(work_a), bytes_a, p(frames), p(score), p(status_k),
                                                                         stream))), "ta_forced_align")

    def confidence_kernel():
        _native.check(lib.ta_forced_confidence(*(head + (p(d[5]), p(t_peak)) + sizes + (p(work_c), bytes_c, p(conf_k), p(rival_k),
                                                                                      p(status_k), stream))),
                      "ta_forced_confidence")
    out["kernels"] = {"forced_alignment": events(align_kernel), "forced_confidence": events(confidence_kernel)}
    out["kernels"]["ratio_confidence_to_alignment"] = (out["kernels"]["forced_confidence"]["median_ms"] /
                                                       out["kernels"]["forced_alignment"]["median_ms"])
    assert int(status_k.cpu().numpy().max()) == 0 and torch.equal(conf_k, kept["conf"][0]) and torch.equal(rival_k, kept["conf"][1])
    assert torch.equal(frames, kept["align"][0])
    conf, _, status = kept["conf"]
    assert int(status.cpu().numpy().max()) == 0 and int(conf.cpu().numpy().min()) >= 0     # at the peaks: never negative
    out["ratio_confidence_to_alignment"] = out["forced_confidence"]["median_ms"] / out["forced_alignment"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    strip = lambda d: {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "ms"}     # noqa: E731
    print(json.dumps(strip(out)))


if __name__ == "__main__":
    main()
