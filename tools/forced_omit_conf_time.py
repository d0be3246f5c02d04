"""What the per-character confidence on the lattice with omission costs beside its two yardsticks (DESIGN.md section
14.18), on a real MI355X: `ta_forced_align_omit`, `ta_forced_confidence` and `ta_forced_omit_confidence` on the
benchmark's 1 920 synthetic lines (bench.synthetic_lines: 800 .. 2000 columns) with random texts of 50 .. 70 characters --
tools/forced_time.py's lines and texts -- in the same run, at 4 bits per omitted character.  HIP events go around the C
entry points alone, on arguments that already lie on the device and workspaces allocated before the clock starts; the
strict confidence is queried at the strict aligner's own t_peak, the new entry with forced.omit_queries' queries on the
frames `ta_forced_align_omit` wrote.  Medians of --passes repeats after a warm-up each, and the ratios of the new entry to
both yardsticks.  Writes profiles/forced_omit_conf_time.json; no threshold is set here.

    python tools/forced_omit_conf_time.py [--lines 1920] [--passes 10] [--omit 4] [--out profiles/forced_omit_conf_time.json]
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
    ap.add_argument("--omit", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "forced_omit_conf_time.json"))
    args = ap.parse_args()
    import torch
    import bench
    from text_alignment_amd import _native, forced, ocr
    model = ocr.LineModel.random(7001, no=96)
    rec = ocr.LineRecognizer(model)
    lib = _native.lib
    omit_q = forced.omit_units(args.omit)

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
    probs = st["probs"]
    d_labels = torch.from_numpy(labels).to(rec.device)
    # ---- what the queries are made of: the two aligners' frames, through the Python calls, untimed -----------------------
    strict = forced.forced_alignment(probs, row_off, T, d_labels, lab_off, L)
    assert int(strict[2].cpu().numpy().max()) == 0
    t_peak = strict[0][:, 2].contiguous()
    with_omit = forced.forced_alignment(probs, row_off, T, d_labels, lab_off, L, host=True, omit_q=omit_q)
    assert not with_omit["status"].any()
    qs = [forced.omit_queries(with_omit["frames"][a:a + l], t) for a, l, t in zip(lab_off, L, T)]
    nq = np.asarray([len(qc) for qc, _ in qs], dtype=np.int32)
    q_off = np.concatenate([[0], np.cumsum(nq)[:-1]]).astype(np.int64)
    q_char, q_frame = np.concatenate([qc for qc, _ in qs]), np.concatenate([qf for _, qf in qs])
    want = forced.forced_omit_confidence(probs, row_off, T, d_labels, lab_off, L, q_char, q_frame, q_off, nq, omit_q)
    assert int(want[2].cpu().numpy().max()) == 0

    # ---- the launches alone: every argument uploaded and the workspaces allocated before the clock starts ----------------
    def pieces(size_of):
        size = np.asarray([size_of(b) for b in range(args.lines)], dtype=np.int64)
        return np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64), int(size.sum())
    T32, L32 = np.ascontiguousarray(T, dtype=np.int32), np.ascontiguousarray(L, dtype=np.int32)
    (off_a, bytes_a) = pieces(lambda b: lib.ta_forced_omit_workspace_bytes(int(T[b]), int(L[b])))
    (off_c, bytes_c) = pieces(lambda b: lib.ta_forced_confidence_workspace_bytes(int(T[b]), int(L[b])))
    (off_o, bytes_o) = pieces(lambda b: lib.ta_forced_omit_confidence_workspace_bytes(int(T[b]), int(L[b]), int(nq[b])))
    d = _native.upload_packed([np.ascontiguousarray(row_off, dtype=np.int64), T32, lab_off, L32, off_a, off_c, off_o, q_off, nq,
                               q_char, q_frame], rec.device)
    dev = dict(device=rec.device)
    work = {k: torch.empty(max(b, 16), dtype=torch.uint8, **dev) for k, b in (("a", bytes_a), ("c", bytes_c), ("o", bytes_o))}
    frames = torch.empty((len(labels), 3), dtype=torch.int32, **dev)
    score = torch.empty(args.lines, dtype=torch.int64, **dev)
    conf_c, rival_c = torch.empty(len(labels), dtype=torch.int64, **dev), torch.empty(len(labels), dtype=torch.int32, **dev)
    conf_o, rival_o = torch.empty(len(q_char), dtype=torch.int64, **dev), torch.empty(len(q_char), dtype=torch.int32, **dev)
    status = {k: torch.empty(args.lines, dtype=torch.int32, **dev) for k in "aco"}
    p = lambda t: t.data_ptr()                                                                     # noqa: E731
    head = (p(probs), p(d[0]), p(d[1]), p(d_labels), p(d[2]), p(d[3]))
    n, no, rows = args.lines, int(probs.shape[1]), int(probs.shape[0])
    stream = torch.cuda.current_stream(rec.device).cuda_stream

    def align_omit():
        _native.check(lib.ta_forced_align_omit(*(head + (p(d[4]), n, no, rows, len(labels), T32.ctypes.data, L32.ctypes.data, omit_q,
                                                         p(work["a"]), bytes_a, p(frames), p(score), p(status["a"]), stream))),
                      "ta_forced_align_omit")

    def confidence():
        _native.check(lib.ta_forced_confidence(*(head + (p(d[5]), p(t_peak), n, no, rows, len(labels), T32.ctypes.data,
                                                         L32.ctypes.data, p(work["c"]), bytes_c, p(conf_c), p(rival_c),
                                                         p(status["c"]), stream))), "ta_forced_confidence")

    def omit_confidence():
        _native.check(lib.ta_forced_omit_confidence(*(head + (p(d[6]), p(d[9]), p(d[10]), p(d[7]), p(d[8]), n, no, rows, len(labels),
                                                              len(q_char), T32.ctypes.data, L32.ctypes.data, nq.ctypes.data, omit_q,
                                                              p(work["o"]), bytes_o, p(conf_o), p(rival_o), p(status["o"]), stream))),
                      "ta_forced_omit_confidence")
    out = {"device": torch.cuda.get_device_name(0), "precision": ocr.DEFAULT_PRECISION, "passes": args.passes,
           "lines": args.lines, "timesteps": int(T.sum()), "labels": int(L.sum()), "omit_bits": args.omit,
           "queries": int(nq.sum()), "omitted_characters": int((with_omit["frames"][:, 0] < 0).sum()),
           "workspace_bytes": {"forced_align_omit": bytes_a, "forced_confidence": bytes_c, "forced_omit_confidence": bytes_o},
           "kernels": {"forced_align_omit": events(align_omit), "forced_confidence": events(confidence),
                       "forced_omit_confidence": events(omit_confidence)}}
    k = out["kernels"]
    k["ratio_omit_confidence_to_align_omit"] = k["forced_omit_confidence"]["median_ms"] / k["forced_align_omit"]["median_ms"]
    k["ratio_omit_confidence_to_confidence"] = k["forced_omit_confidence"]["median_ms"] / k["forced_confidence"]["median_ms"]
    for s in status.values():
        assert int(s.cpu().numpy().max()) == 0
    assert torch.equal(conf_o, want[0]) and torch.equal(rival_o, want[1])
    assert np.array_equal(frames.cpu().numpy(), with_omit["frames"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    strip = lambda d: {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "ms"}     # noqa: E731
    print(json.dumps(strip(out)))


if __name__ == "__main__":
    main()
