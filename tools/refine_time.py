"""What the refinement inside the page pipeline costs, on a real MI355X:

64 synthetic pages of 20 lines, read by a synthetic model that emits letters and spaces, with SECOND-PASS transcripts
(every page's transcript is its own OCR text, cleaned to letters and single spaces) so that most lines are accepted at
min_agreement 4/5; the accepted fraction is recorded.  Wall milliseconds, medians of --passes repeats after a warm-up:
(a) process_batch without refine;
(b) process_batch(..., refine=True);
(c) forced.refine_pages over the same pages in calls of 16 -- the only way to refine before the switch existed.
Beside them the workspace and probability bytes of one 16-page chunk, and the HIP-event times of ta_forced_align_lines
and of ta_refine_columns alone on such a chunk's resident data.
--parent PATH: leg (a) is also run, first and in a process of its own, on the package of the checkout at PATH (the
commit before the switch), and the ratio of the two (a) is recorded: the switch must not cost the path that does not
use it.  Writes profiles/refine_pipeline_time.json; no threshold is set here.

    python tools/refine_time.py [--pages 64] [--passes 10] [--parent PATH] [--out profiles/refine_pipeline_time.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [8, -12, -6, -6, -2, -2]


def model_and_pages(npages, nlines, seed):
    """(recogniser, pages): lines of oracle.ocr_ref_f64.synthetic_line, a model whose output layer prefers blanks,
    spaces and letters (tests/test_forced_gpu.py's)"""
    from oracle import ocr_ref_f64 as OR
    from text_alignment_amd import ocr, page as page_mod
    om = OR.synthetic_model(7001, no=40)
    om.W2[:, 1:] *= 3.0
    om.W2[0, 0] += 4.0
    om.W2[1, 0] += 2.0
    om.W2[2, 0] -= 30.0
    om.W2[29:, 0] -= 30.0
    rec = ocr.LineRecognizer(ocr.LineModel(om.fwd, om.rev, om.W2, om.codec))
    rng = np.random.default_rng(seed)
    pages = []
    for p in range(npages):
        strips = []
        for k in range(nlines):
            w = int(rng.integers(150, 421))
            strips.append(page_mod.Strip(offset_x=40 + int(rng.integers(0, 30)), offset_y=100 + 120 * k, height=60, width=2 * w,
                                         prepared=OR.synthetic_line(seed * 1000 + p * nlines + k, width=w)))
        pages.append(page_mod.PreparedPage((2200, 3300), (2200, 3300), 0, strips, [130 + 120 * k for k in range(nlines + 1)]))
    return rec, pages


def second_pass(result, page):
    """a page's transcript from its own OCR text: letters and single spaces, the lines joined by a space"""
    rows = {s.offset_y: k for k, s in enumerate(page.strips)}
    lines = [""] * len(page.strips)
    for ch, box in zip(result[3].chars, result[3].boxes):
        lines[rows[int(box[1])]] += ch
    clean = [" ".join("".join(ch if "a" <= ch <= "z" else " " for ch in tx).split()) for tx in lines]
    return " ".join(c for c in clean if c) or "a"


def wall(fn, passes, sync):
    fn()
    sync()
    ms = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"ms": ms, "median_ms": statistics.median(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--lines", type=int, default=20)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--repo", default=HERE, help="the checkout whose package is timed")
    ap.add_argument("--leg", default="all", choices=("all", "a"))
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "refine_pipeline_time.json"))
    args = ap.parse_args()
    out = {}
    if args.parent:                                      # first, alone on the device, in a process of its own
        tmp = args.out + ".parent"
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--repo", os.path.abspath(args.parent), "--leg", "a",
                               "--pages", str(args.pages), "--lines", str(args.lines), "--passes", str(args.passes),
                               "--out", tmp], timeout=600)
        with open(tmp) as f:
            out["a_parent"] = json.load(f)["a"]
        os.remove(tmp)
    sys.path.insert(0, os.path.abspath(args.repo))
    import torch
    from text_alignment_amd import alignToOCR as atocr, forced, ocr
    rec, pages = model_and_pages(args.pages, args.lines, 4100)
    first = atocr.process_batch(pages, ["amen"] * len(pages), rec, PARAMS)
    trs = [second_pass(r, pg) for r, pg in zip(first, pages)]
    sync = torch.cuda.synchronize
    out.update(device=torch.cuda.get_device_name(0), precision=ocr.DEFAULT_PRECISION, passes=args.passes, pages=args.pages,
               lines_per_page=args.lines, chunk_pages=atocr.PIPELINE_CHUNK_PAGES)
    out["a"] = wall(lambda: atocr.process_batch(pages, trs, rec, PARAMS), args.passes, sync)
    if args.leg == "all":
        refined = []
        atocr.process_batch(pages, trs, rec, PARAMS, refine=True, min_agreement=(4, 5), refined_out=refined)
        out["accepted_fraction"] = float(np.concatenate(refined).mean())
        out["b"] = wall(lambda: atocr.process_batch(pages, trs, rec, PARAMS, refine=True, min_agreement=(4, 5)), args.passes, sync)
        step = 16
        out["c"] = wall(lambda: [forced.refine_pages(pages[a:a + step], trs[a:a + step], rec, PARAMS, (4, 5))
                                 for a in range(0, len(pages), step)], args.passes, sync)
        out["c"]["pages_per_call"] = step
        out["b_over_c"] = out["b"]["median_ms"] / out["c"]["median_ms"]
        # ---- one 16-page chunk: its bytes, and the two kernels alone on its resident data ----------------------------------
        chunk = atocr.PageChunk(rec, pages[:step], trs[:step], PARAMS, atocr.parallel, refine=(4, 5))
        chunk.launch()
        chunk.host_ahead()
        real = forced.Refining
        kept = {}
        forced.Refining = lambda *a, **k: kept.setdefault("r", real(*a, keep=True, **k))
        try:
            chunk.align()
        finally:
            forced.Refining = real
        r = kept["r"]
        sync()

        def events(fn):
            ms = []
            with torch.cuda.stream(r.stream):
                for k in range(args.passes + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if k:
                        ms.append(e0.elapsed_time(e1))
            return {"ms": ms, "median_ms": statistics.median(ms)}
        out["chunk"] = {"pages": step, "lines": r.nlines, "timesteps": int(r.T.sum()),
                        "workspace_bytes": int(forced.Refining.last_bytes[0]), "probability_bytes": int(forced.Refining.last_bytes[1]),
                        "ta_forced_align_lines": events(r.forced), "ta_refine_columns": events(r.columns)}
        chunk.finish(None, None)
    if "a_parent" in out:
        out["a_over_parent"] = out["a"]["median_ms"] / out["a_parent"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    strip = lambda d: {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "ms"}     # noqa: E731
    print(json.dumps(strip(out)))


if __name__ == "__main__":
    main()
