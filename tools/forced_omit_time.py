"""What the omission-tolerant forced alignment costs beside the strict one, on a real MI355X:
`ta_forced_align_omit` at omit_q = 4 * 65536 and `ta_forced_align` on the SAME lines in the SAME run -- the benchmark's
1 920 synthetic lines (bench.synthetic_lines: 800 .. 2000 columns) with random texts of 50 .. 70 characters, HIP events
around forced.forced_alignment on resident probabilities and labels, as tools/forced_time.py (a) times the strict call.
Medians of --passes repeats after a warm-up each.  Writes profiles/forced_omit_time.json with both times and their
ratio; no threshold is set here.  The model is random: this is the cost of the lattice, not a statement about accuracy.

    python tools/forced_omit_time.py [--lines 1920] [--passes 10] [--omit-bits 4] [--out profiles/forced_omit_time.json]
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
    ap.add_argument("--omit-bits", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "forced_omit_time.json"))
    args = ap.parse_args()
    import torch
    import bench
    from text_alignment_amd import forced, ocr
    model = ocr.LineModel.random(7001, no=96)
    rec = ocr.LineRecognizer(model)
    omit_q = forced.omit_units(args.omit_bits)
    out = {"device": torch.cuda.get_device_name(0), "precision": ocr.DEFAULT_PRECISION, "passes": args.passes,
           "omit_q": omit_q}

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

    def strict():
        kept["strict"] = forced.forced_alignment(st["probs"], row_off, T, d_labels, lab_off, L)

    def tolerant():
        kept["omit"] = forced.forced_alignment(st["probs"], row_off, T, d_labels, lab_off, L, omit_q=omit_q)
    out.update(lines=args.lines, timesteps=int(T.sum()), labels=int(L.sum()),
               lines_of_variant_K2=int((2 * L + 1 <= 128).sum()), forced_align=events(strict), forced_align_omit=events(tolerant))
    assert int(kept["strict"][2].cpu().numpy().max()) == 0 and int(kept["omit"][2].cpu().numpy().max()) == 0
    out["omitted_characters"] = int((kept["omit"][0][:, 0] == forced.OMITTED).sum().item())
    out["ratio_omit_to_strict"] = out["forced_align_omit"]["median_ms"] / out["forced_align"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    strip = lambda d: {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "ms"}     # noqa: E731
    print(json.dumps(strip(out)))


if __name__ == "__main__":
    main()
