"""What the posteriors cost at page scope, on a real MI355X, on tools/forced_page_time.py's 64
synthetic pages of 20 lines: `ta_forced_align_pages`, `ta_forced_page_confidence` and `ta_forced_page_posterior` on the
SAME pages and the SAME resident probabilities in the SAME run, with the whole text as every line's window, so that every
page has a path; confidence and posterior are queried at the aligner's own (line, t_peak), the frames handed over on the
device.  HIP events around forced.forced_page_alignment, forced.forced_page_confidence and forced.forced_page_posterior,
medians of --passes repeats after a warm-up each, and the ratios.  The yardsticks are the aligner and the confidence of
this run, not an earlier file.  Writes profiles/forced_page_post_time.json with the workspace bytes and the compiler's
resource table of the variants that ran; no threshold is set here.  The model is random: its pages say nothing about
which posterior marks a wrong box or which likelihood a wrong transcript on a real page.

    python tools/forced_page_post_time.py [--pages 64] [--passes 10] [--out profiles/forced_page_post_time.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# profiles/forced_page_post_resources.txt, per variant: VGPR, AGPR, SGPR, scratch bytes per lane, LDS bytes
RESOURCES = {2: (79, 0, 106, 0, 11408), 4: (101, 0, 106, 0, 12944), 8: (157, 0, 106, 0, 16016), 16: (256, 1, 106, 0, 22160),
             32: (256, 17, 106, 0, 34448)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "forced_page_post_time.json"))
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
    K = [int(_native.lib.ta_forced_page_variant(int(w))) for w in nc]
    out.update(pages_timed=len(take), frames=int(T.sum()), characters=int(nc.sum()), widest_window=int(nc.max()),
               frames_longest_page=int(max(T[a:b].sum() for a, b in zip(lf[:-1], lf[1:]))), variants=sorted(set(K)))
    out["workspace_bytes"] = {
        "confidence": int(sum(_native.lib.ta_forced_page_confidence_workspace_bytes(int(n), k) for n, k in zip(nc, K))),
        "posterior": int(sum(_native.lib.ta_forced_page_posterior_workspace_bytes(int(n), k) for n, k in zip(nc, K)))}
    out["resources"] = {"K = %d" % k: dict(zip(("vgpr", "agpr", "sgpr", "scratch_bytes_per_lane", "lds_bytes"), RESOURCES[k]))
                        for k in sorted(set(K))}

    def align():
        kept["aligned"] = forced.forced_page_alignment(st["probs"], row, T, lf, lo, hi, labels, cum(nc))

    def confidence():
        kept["conf"] = forced.forced_page_confidence(st["probs"], row, T, lf, lo, hi, labels, cum(nc), kept["aligned"][0])

    def posterior():
        kept["post"] = forced.forced_page_posterior(st["probs"], row, T, lf, lo, hi, labels, cum(nc), kept["aligned"][0])

    out["align"] = events(align)
    out["confidence"] = events(confidence)
    out["posterior"] = events(posterior)
    for name, status in (("align", kept["aligned"][2]), ("confidence", kept["conf"][2]), ("posterior", kept["post"]["status"])):
        status = status.cpu().numpy()
        out[name]["status"] = {forced.PAGE_CONF_STATUS[int(k)]: int((status == k).sum()) for k in np.unique(status)}
    post = {name: t.cpu().numpy() for name, t in kept["post"].items()}
    ok = post["status"] == forced.OK
    at = np.repeat(ok, nc)
    values = forced.posterior_values(post["own_m"][at], post["own_x"][at], np.repeat(post["z_m"], nc)[at], np.repeat(post["z_x"], nc)[at])
    bits = forced.loglik_bits(post["z_m"][ok], post["z_x"][ok]) / np.add.reduceat(T, lf[:-1])[ok]
    out["posterior"].update(characters=int(at.sum()), median=float(np.median(values)) if at.any() else None,
                            above_one=int((values > 1 + 8 * out["frames_longest_page"] * 2.0 ** -53).sum()),
                            median_loglik_bits_per_frame=float(np.median(bits)) if ok.any() else None)
    out["ratio_confidence_to_align"] = out["confidence"]["median_ms"] / out["align"]["median_ms"]
    out["ratio_posterior_to_align"] = out["posterior"]["median_ms"] / out["align"]["median_ms"]
    out["ratio_posterior_to_confidence"] = out["posterior"]["median_ms"] / out["confidence"]["median_ms"]
    out["not_tuned"] = ("the chunk length, the place of the renormalisation, the K = 32 variant's register pressure "
                        "(256 VGPRs + 17 AGPRs, one wave per SIMD) and the combine are as first written")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    strip = lambda d: {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "ms"}     # noqa: E731
    print(json.dumps(strip(out)))


if __name__ == "__main__":
    main()
