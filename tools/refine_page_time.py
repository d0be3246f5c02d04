"""What page scope inside the page pipeline costs, on a real MI355X, in ONE run:

tools/refine_time.py's 64 synthetic pages of 20 lines and their SECOND-PASS transcripts (every page's transcript is its
own OCR text, cleaned to letters and single spaces: the pages where nearly every line is accepted, so the windows are
narrow).  Wall milliseconds, medians of --passes repeats after a warm-up:
(a) process_batch without refine;
(b) process_batch(..., refine=True)                                       -- line scope;
(c) process_batch(..., refine=True, refine_scope="page", page_margin=16)  -- page scope inside the pipeline;
(d) forced.refine_pages(scope="page", margin=16) over the same pages in four calls of 16 -- the only way before.
Beside them the share of pages (c) refined, the variants it launched and the variants its pages' windows hit, and the
workspace and probability bytes of its last chunk.  (c)/(d) and (c)/(b) are recorded as what they are; no threshold is
set here.
--parent PATH: legs (a) and (b) are also run on the package of the checkout at PATH (the commit before the switch), in a
process of its own BEFORE and another AFTER this one's -- parent / change / parent in one session -- and the three values
per leg are written into the same file: the legs that do not use the switch must not move (the host-heavy page legs
spread +-10 % from process to process, README).
Writes profiles/refine_page_pipeline_time.json.

    python tools/refine_page_time.py [--pages 64] [--passes 10] [--parent PATH] [--out profiles/refine_page_pipeline_time.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [8, -12, -6, -6, -2, -2]
MARGIN = 16


def parent_legs(args, tag):
    """legs (a) and (b) on the parent's package, in a process of its own"""
    tmp = "%s.%s" % (args.out, tag)
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--repo", os.path.abspath(args.parent), "--legs", "ab",
                           "--pages", str(args.pages), "--lines", str(args.lines), "--passes", str(args.passes),
                           "--out", tmp], timeout=900)
    with open(tmp) as f:
        got = json.load(f)
    os.remove(tmp)
    return {"a": got["a"], "b": got["b"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--lines", type=int, default=20)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--repo", default=HERE, help="the checkout whose package is timed")
    ap.add_argument("--legs", default="abcd", choices=("abcd", "ab"))
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "refine_page_pipeline_time.json"))
    args = ap.parse_args()
    out = {}
    if args.parent:
        out["parent_before"] = parent_legs(args, "before")
    sys.path.insert(0, os.path.abspath(args.repo))
    import torch
    from text_alignment_amd import alignToOCR as atocr, forced, ocr
    from tools.refine_time import model_and_pages, second_pass, wall
    rec, pages = model_and_pages(args.pages, args.lines, 4100)
    first = atocr.process_batch(pages, ["amen"] * len(pages), rec, PARAMS)
    trs = [second_pass(r, pg) for r, pg in zip(first, pages)]
    sync = torch.cuda.synchronize
    out.update(device=torch.cuda.get_device_name(0), precision=ocr.DEFAULT_PRECISION, passes=args.passes, pages=args.pages,
               lines_per_page=args.lines, chunk_pages=atocr.PIPELINE_CHUNK_PAGES, margin=MARGIN)
    out["a"] = wall(lambda: atocr.process_batch(pages, trs, rec, PARAMS), args.passes, sync)
    out["b"] = wall(lambda: atocr.process_batch(pages, trs, rec, PARAMS, refine=True, min_agreement=(4, 5)), args.passes, sync)
    if args.legs == "abcd":
        page = dict(refine=True, min_agreement=(4, 5), refine_scope="page", page_margin=MARGIN)
        refined, scope = [], []
        atocr.process_batch(pages, trs, rec, PARAMS, refined_out=refined, page_scope_out=scope, **page)
        lib = forced._native.lib
        hit = sorted({int(lib.ta_forced_page_variant(int((s.windows[1] - s.windows[0]).max()))) for s in scope if s.reason == 0})
        top = int(lib.ta_forced_page_variant(int(forced.page_caps(trs).max())))
        out["page_scope"] = {"pages_refined_fraction": float(np.mean([s.reason == 0 for s in scope])),
                             "reasons": {str(r): int(sum(s.reason == r for s in scope)) for r in sorted({s.reason for s in scope})},
                             "lines_refined_fraction": float(np.concatenate(refined).mean()),
                             "transcript_characters": [int(min(map(len, trs))), int(max(map(len, trs)))],
                             "widest_window": int(max(int((s.windows[1] - s.windows[0]).max()) for s in scope if s.windows)),
                             "variants_launched": [k for k in (2, 4, 8, 16, 32) if k <= top], "variants_hit": hit,
                             "last_chunk_workspace_bytes": int(forced.PageRefining.last_bytes[0]),
                             "last_chunk_probability_bytes": int(forced.PageRefining.last_bytes[1])}
        out["c"] = wall(lambda: atocr.process_batch(pages, trs, rec, PARAMS, **page), args.passes, sync)
        step = 16
        out["d"] = wall(lambda: [forced.refine_pages(pages[a:a + step], trs[a:a + step], rec, PARAMS, (4, 5), scope="page",
                                                     margin=MARGIN) for a in range(0, len(pages), step)], args.passes, sync)
        out["d"]["pages_per_call"] = step
        out["c_over_d"] = out["c"]["median_ms"] / out["d"]["median_ms"]
        out["c_over_b"] = out["c"]["median_ms"] / out["b"]["median_ms"]
        out["c_over_a"] = out["c"]["median_ms"] / out["a"]["median_ms"]
    if args.parent:
        out["parent_after"] = parent_legs(args, "after")
        for leg in "ab":
            out["%s_parent_change_parent_ms" % leg] = [out["parent_before"][leg]["median_ms"], out[leg]["median_ms"],
                                                       out["parent_after"][leg]["median_ms"]]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    strip = lambda d: {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "ms"}     # noqa: E731
    print(json.dumps(strip(out)))


if __name__ == "__main__":
    main()
