"""What the confidence costs at page scope, on a real MI355X, on tools/forced_page_time.py's 64
synthetic pages of 20 lines: `ta_forced_align_pages` and `ta_forced_page_confidence` on the SAME pages and the SAME
resident probabilities in the SAME run, with the whole text as every line's window, so that every page has a path; the
confidence is queried at the aligner's own (line, t_peak), the frames handed over on the device.  HIP events around
forced.forced_page_alignment and forced.forced_page_confidence, medians of --passes repeats after a warm-up each, and
their ratio.  The yardstick is the page aligner of this run, not an earlier file.  Writes
profiles/forced_page_conf_time.json; no threshold is set here.  The model is random: its pages say nothing about which
confidence marks a wrong box on a real page, and no threshold has been validated.

    python tools/forced_page_conf_time.py [--pages 64] [--passes 10] [--out profiles/forced_page_conf_time.json]
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "forced_page_conf_time.json"))
    args = ap.parse_args()
    import torch
    from text_alignment_amd import _native, forced, harvest, ocr
    from tools.harvest_time import synthetic_pages
    model = ocr.LineModel.random(7001, no=96)
    rec = ocr.LineRecognizer(model)
    pages, trs = synthetic_pages(args.pages, 20, 4100)
    out = {"device": torch.cuda.get_device_name(0), "precision": ocr.DEFAULT_PRECISION, "passes": args.passes,
           "pages": args.pages, "lines_per_page": 20, "windows": "the whole text on every line",
           "queries": "the aligner's own line and t_peak, handed over on the device"}
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

    def align():
        kept["aligned"] = forced.forced_page_alignment(st["probs"], row, T, lf, lo, hi, labels, cum(nc))

    def confidence():
        kept["conf"] = forced.forced_page_confidence(st["probs"], row, T, lf, lo, hi, labels, cum(nc), kept["aligned"][0])

    out["align"] = events(align)
    out["confidence"] = events(confidence)
    for name, got in (("align", kept["aligned"]), ("confidence", kept["conf"])):
        status = got[2].cpu().numpy()
        out[name]["status"] = {forced.PAGE_CONF_STATUS[int(k)]: int((status == k).sum()) for k in np.unique(status)}
    conf = kept["conf"][0].cpu().numpy()
    ok = np.repeat(kept["conf"][2].cpu().numpy() == forced.OK, nc)
    out["confidence"].update(characters=int(ok.sum()), zero=int((conf[ok] == 0).sum()), negative=int((conf[ok] < 0).sum()),
                             median_bits=float(np.median(forced.confidence_bits(conf[ok]))) if ok.any() else None)
    out["ratio_confidence_to_align"] = out["confidence"]["median_ms"] / out["align"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    strip = lambda d: {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "ms"}     # noqa: E731
    print(json.dumps(strip(out)))


if __name__ == "__main__":
    main()
