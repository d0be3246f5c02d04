"""What omission costs at page scope, on a real MI355X, on tools/forced_page_time.py's 64
synthetic pages of 20 lines: `ta_forced_align_pages` and `ta_forced_align_pages_omit` at --bits per character on the SAME
pages and the SAME resident probabilities in the SAME run, with the whole text as every line's window, so that every page
has a strict path and both kernels fill, walk and find peaks.  HIP events around forced.forced_page_alignment, medians of
--passes repeats after a warm-up each, and their ratio.  The yardstick is the strict page kernel of this run, not an
earlier file.  Writes profiles/forced_page_omit_time.json; no threshold is set here.  The model is random: what its pages
say about the share of real pages this refines, the right page_omit or the right margin is nothing, and none of the three
has been measured.

    python tools/forced_page_omit_time.py [--pages 64] [--passes 10] [--bits 4] [--out profiles/forced_page_omit_time.json]
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
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--bits", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "forced_page_omit_time.json"))
    args = ap.parse_args()
    import torch
    from text_alignment_amd import _native, forced, harvest, ocr
    from tools.harvest_time import synthetic_pages
    model = ocr.LineModel.random(7001, no=96)
    rec = ocr.LineRecognizer(model)
    pages, trs = synthetic_pages(args.pages, 20, 4100)
    omit_q = forced.omit_units(args.bits)
    out = {"device": torch.cuda.get_device_name(0), "precision": ocr.DEFAULT_PRECISION, "passes": args.passes,
           "pages": args.pages, "lines_per_page": 20, "omit_bits": args.bits, "windows": "the whole text on every line"}
    kept = {}

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

    # the recogniser's probabilities of all lines, resident; the pages whose text fits one window
    strips = [[s.prepared for s in pg.strips] for pg in pages]
    classes = [harvest.transcript_classes(model.codec, tr) for tr in trs]
    take = [p for p in range(len(pages)) if 1 <= len(classes[p]) <= forced.MAX_TARGET and strips[p] and
            not (np.asarray(classes[p]) == 0).any()]
    st = rec.prepare([ln for p in take for ln in strips[p]])
    rec.run(st, want_probs=True, decode=False)
    nl = np.asarray([len(strips[p]) for p in take], dtype=np.int64)
    nc = np.asarray([len(classes[p]) for p in take], dtype=np.int64)
    nlines = int(nl.sum())
    T = np.asarray(st["T_host"], dtype=np.int64)[:nlines]
    row = np.asarray(st["row_start_host"], dtype=np.int64)[:nlines]
    cum = lambda xs: np.concatenate([[0], np.cumsum(xs)]).astype(np.int64)                        # noqa: E731
    lo, hi = np.zeros(nlines, np.int64), np.repeat(nc, nl)
    labels = np.concatenate([classes[p] for p in take])
    lf = cum(nl)
    out.update(pages_timed=len(take), frames=int(T.sum()), characters=int(nc.sum()), widest_window=int(nc.max()),
               frames_longest_page=int(max(T[a:b].sum() for a, b in zip(lf[:-1], lf[1:]))),
               variants=sorted({int(_native.lib.ta_forced_page_variant(int(w))) for w in nc}))

    def align(q):
        kept["got"] = forced.forced_page_alignment(st["probs"], row, T, lf, lo, hi, labels, cum(nc), omit_q=q)

    for name, q in (("strict", None), ("omit", omit_q)):
        out[name] = events(lambda: align(q))
        frames, score, status = (t.cpu().numpy() for t in kept["got"])
        out[name]["status"] = {forced.PAGE_STATUS[int(k)]: int((status == k).sum()) for k in np.unique(status)}
        if q is not None:
            out[name]["characters_omitted"] = int((frames[:, 0] == forced.OMITTED).sum())
    out["ratio_omit_to_strict"] = out["omit"]["median_ms"] / out["strict"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    strip = lambda d: {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "ms"}     # noqa: E731
    print(json.dumps(strip(out)))


if __name__ == "__main__":
    main()
