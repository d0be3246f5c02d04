"""What forced alignment with omission inside the page pipeline costs, on a real MI355X, in ONE
run:

tools/refine_time.py's 64 synthetic pages of 20 lines and their SECOND-PASS transcripts, chunks of 16.  Wall milliseconds,
medians of --passes repeats after a warm-up:
(a)  process_batch without refine;
(b)  process_batch(..., refine=True)                 -- the strict lattice;
(bo) process_batch(..., refine=True, line_omit=4)    -- omission inside the pipeline;
(oo) forced.refine_pages(..., omit=4) over the same pages in four calls of 16 -- the only way before the switch.
Beside them the lines refined and the characters left out under (bo), and the workspace bytes of one 16-page chunk, strict
and with omission.  (bo)/(b) and (bo)/(oo) are recorded as what they are; no threshold is set here.
--parent PATH: legs (a) and (b) are also run on the package of the checkout at PATH (the commit before the switch), in a
process of its own BEFORE and another AFTER this one's -- parent / change / parent in one session -- and the three values
per leg are written into the same file: the legs that do not use the switch must lie inside what the two parent runs
span, or the excess wants an explanation (the host-heavy page legs spread from process to process, README).
Writes profiles/refine_omit_pipeline_time.json.

    python tools/refine_omit_time.py [--pages 64] [--passes 10] [--parent PATH] [--out profiles/refine_omit_pipeline_time.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [8, -12, -6, -6, -2, -2]
OMIT = 4.0


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
    ap.add_argument("--legs", default="all", choices=("all", "ab"))
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "refine_omit_pipeline_time.json"))
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
    agree = dict(refine=True, min_agreement=(4, 5))
    out.update(device=torch.cuda.get_device_name(0), precision=ocr.DEFAULT_PRECISION, passes=args.passes, pages=args.pages,
               lines_per_page=args.lines, chunk_pages=atocr.PIPELINE_CHUNK_PAGES, omit_bits=OMIT)
    out["a"] = wall(lambda: atocr.process_batch(pages, trs, rec, PARAMS), args.passes, sync)
    out["b"] = wall(lambda: atocr.process_batch(pages, trs, rec, PARAMS, **agree), args.passes, sync)
    if args.legs == "all":
        refined, omitted = [], []
        atocr.process_batch(pages, trs, rec, PARAMS, refined_out=refined, line_omit=OMIT, omitted_out=omitted, **agree)
        gone = np.concatenate(omitted)
        out["omission"] = {"lines_refined_fraction": float(np.concatenate(refined).mean()),
                           "lines_aligned": int((gone >= 0).sum()), "lines_with_an_omitted_character": int((gone > 0).sum()),
                           "characters_omitted": int(gone[gone > 0].sum()),
                           "transcript_characters": int(sum(len(tr) for tr in trs))}
        out["bo"] = wall(lambda: atocr.process_batch(pages, trs, rec, PARAMS, line_omit=OMIT, **agree), args.passes, sync)
        step = 16
        out["oo"] = wall(lambda: [forced.refine_pages(pages[a:a + step], trs[a:a + step], rec, PARAMS, (4, 5), omit=OMIT)
                                  for a in range(0, len(pages), step)], args.passes, sync)
        out["oo"]["pages_per_call"] = step
        out["bo_over_b"] = out["bo"]["median_ms"] / out["b"]["median_ms"]
        out["bo_over_oo"] = out["bo"]["median_ms"] / out["oo"]["median_ms"]
        out["bo_minus_b_ms"] = out["bo"]["median_ms"] - out["b"]["median_ms"]
        # ---- one 16-page chunk: the bytes of its workspace, strict and with omission ------------------------------------------
        atocr.process_batch(pages[:step], trs[:step], rec, PARAMS, **agree)
        strict_bytes = int(forced.Refining.last_bytes[0])
        atocr.process_batch(pages[:step], trs[:step], rec, PARAMS, line_omit=OMIT, **agree)
        out["chunk"] = {"pages": step, "transcript_characters": int(sum(len(tr) for tr in trs[:step])),
                        "strict_workspace_bytes": strict_bytes, "omit_workspace_bytes": int(forced.Refining.last_bytes[0]),
                        "probability_bytes": int(forced.Refining.last_bytes[1])}
    if args.parent:
        out["parent_after"] = parent_legs(args, "after")
        for leg in "ab":
            three = [out["parent_before"][leg]["median_ms"], out[leg]["median_ms"], out["parent_after"][leg]["median_ms"]]
            out["%s_parent_change_parent_ms" % leg] = three
            out["%s_above_both_parent_runs" % leg] = bool(three[1] > max(three[0], three[2]))     # an excess to explain
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    strip = lambda d: {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "ms"}     # noqa: E731
    print(json.dumps(strip(out)))


if __name__ == "__main__":
    main()
