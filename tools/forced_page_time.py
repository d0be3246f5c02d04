"""What page-scope forced alignment costs, on a real MI355X, on tools/forced_time.py's 64 synthetic
pages of 20 lines, both measured in the same run:

(a) `ta_forced_align_pages` alone (forced.forced_page_alignment on resident probabilities, the windows page_windows makes
    of the run's own harvest table), HIP events around the call, beside the recogniser's own time for the same lines;
    and once more with the whole text as every line's window, which has a path whatever the harvest table says;
(b) `forced.refine_pages(scope="page")` against `forced.refine_pages(scope="line")`, wall milliseconds.
Medians of --passes repeats after a warm-up each.  Writes profiles/forced_page_time.json; no threshold is set here.  The
call is latency-shaped: one wave per page walks a chain of (frames of the page) dependent steps, so its time is set by the
longest page, not by the number of pages.  The model is random: what its pages say about the corridor real pages need
(`margin`) or about the share of real pages that are eligible is nothing, and neither has been measured.

    python tools/forced_page_time.py [--pages 64] [--passes 10] [--margin 16] [--out profiles/forced_page_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--margin", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "forced_page_time.json"))
    args = ap.parse_args()
    import torch
    from text_alignment_amd import _native, forced, harvest, ocr
    from tools.harvest_time import synthetic_pages
    model = ocr.LineModel.random(7001, no=96)
    rec = ocr.LineRecognizer(model)
    pages, trs = synthetic_pages(args.pages, 20, 4100)
    params = [8, -1, -9, -9, -4, -4]
    out = {"device": torch.cuda.get_device_name(0), "precision": ocr.DEFAULT_PRECISION, "passes": args.passes,
           "pages": args.pages, "lines_per_page": 20, "margin": args.margin}
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

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.passes):
            t0 = time.perf_counter()
            kept["res"] = fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        return {"ms": ms, "median_ms": statistics.median(ms)}

    # ---- (b) first: its result carries the probabilities, the harvest table and the windows (a) runs on -------------------
    b = {"line": wall(lambda: forced.refine_pages(pages, trs, rec, params, 0.9, scope="line"))}
    b["refined_lines_at_line_scope"] = int(np.sum(kept["res"].refined))
    b["page"] = wall(lambda: forced.refine_pages(pages, trs, rec, params, 0.9, scope="page", margin=args.margin))
    res = kept["res"]
    b["difference_ms"] = b["page"]["median_ms"] - b["line"]["median_ms"]
    scope = np.asarray(res.page_scope)
    b["page_scope_of_this_noise_model"] = {forced.PAGE_SCOPE[int(k)]: int((scope == k).sum()) for k in np.unique(scope)}
    out["b"] = b

    # ---- (a) the call alone on the eligible pages, beside the recogniser ------------------------------------------------------
    h = res.harvest
    lf = np.asarray(h.line_first, dtype=np.int64)
    take = [p for p in range(len(pages)) if res.windows[p] is not None]
    a = {"eligible_pages": len(take)}
    if take:
        qs = np.concatenate([np.arange(lf[p], lf[p + 1]) for p in take])
        cum = lambda xs: np.concatenate([[0], np.cumsum(xs)]).astype(np.int64)                    # noqa: E731
        classes = [harvest.transcript_classes(model.codec, trs[p]) for p in take]
        lo = np.concatenate([res.windows[p][0] for p in take])
        hi = np.concatenate([res.windows[p][1] for p in take])
        T, row = res.T[qs], res.row_off[qs]
        width = (hi - lo).astype(np.int64)
        per_page = [int(width[a0:b0].max()) for a0, b0 in zip(cum([lf[p + 1] - lf[p] for p in take])[:-1],
                                                              cum([lf[p + 1] - lf[p] for p in take])[1:])]
        a.update(frames_longest_page=int(max(res.T[lf[p]:lf[p + 1]].sum() for p in take)), frames=int(T.sum()),
                 characters=int(sum(len(c) for c in classes)), widest_window=max(per_page),
                 variants=sorted({int(_native.lib.ta_forced_page_variant(w)) for w in per_page}))

        def align():
            kept["got"] = forced.forced_page_alignment(res.probs, row, T, cum([lf[p + 1] - lf[p] for p in take]), lo, hi,
                                                       np.concatenate(classes), cum([len(c) for c in classes]))
        a["forced_page_alignment"] = events(align)
        status = kept["got"][2].cpu().numpy()
        a["status"] = {forced.PAGE_STATUS[int(k)]: int((status == k).sum()) for k in np.unique(status)}
        # the same pages with the whole text as every line's window (pages of at most 1 023 characters): a path exists
        # whatever the harvest table of the noise model says, so the walk and the peaks are in the interval too
        nl = np.asarray([lf[p + 1] - lf[p] for p in take])
        nc = np.asarray([len(c) for c in classes])
        if (nc <= forced.MAX_TARGET).all():
            lo[:], hi[:] = 0, np.repeat(nc, nl)
            a["whole_text_windows"] = events(align)
            status = kept["got"][2].cpu().numpy()
            a["whole_text_windows"]["status"] = {forced.PAGE_STATUS[int(k)]: int((status == k).sum()) for k in np.unique(status)}
            a["whole_text_windows"]["widest_window"] = int(nc.max())
        st = rec.prepare([ln for pg in pages for ln in [s.prepared for s in pg.strips]])
        rec.run(st)
        torch.cuda.synchronize()
        a["recogniser_all_pages"] = events(lambda: rec.run(st))
    out["a"] = a
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    strip = lambda d: {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "ms"}     # noqa: E731
    print(json.dumps(strip(out)))


if __name__ == "__main__":
    main()
