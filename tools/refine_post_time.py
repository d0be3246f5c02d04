"""What the sum-product posteriors inside the page pipeline cost, on a real MI355X:

the inputs of tools/refine_time.py -- 64 synthetic pages of 20 lines with second-pass transcripts, chunks of 16 -- and, in
ONE run, wall milliseconds as medians of --passes repeats after a warm-up:
(b)   process_batch(..., refine=True);
(bp)  process_batch(..., refine=True, posterior=True);
(bcp) process_batch(..., refine=True, confidence=True, posterior=True);
(pp)  forced.refine_pages(..., posterior=True) over the same pages in calls of 16 -- the only way to the values before
      the switch existed.
Beside them the posterior workspace of one 16-page chunk, next to its workspace of moves.

--parent TREE: a built checkout of the parent commit.  (b) is then timed on it as well, in processes of their own and in
the order parent / change / parent, and the file records all three with the verdict: the switch-off time of the change
lies inside the parent's own spread between its two runs -- from the smaller of the two runs' lower quartiles to the
larger of their upper quartiles -- or it does not.  This process itself never opens the GPU then.
Writes profiles/refine_post_pipeline_time.json; no threshold is set here.

    python tools/refine_post_time.py [--pages 64] [--passes 10] [--parent TREE] [--out profiles/refine_post_pipeline_time.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(args, tree, only_b):
    """the timings on the package of `tree`, in this process"""
    sys.path.insert(0, tree)
    from tools.refine_time import PARAMS, model_and_pages, second_pass, wall
    import torch
    from text_alignment_amd import alignToOCR as atocr, forced, ocr
    rec, pages = model_and_pages(args.pages, args.lines, 4100)
    first = atocr.process_batch(pages, ["amen"] * len(pages), rec, PARAMS)
    trs = [second_pass(r, pg) for r, pg in zip(first, pages)]
    sync = torch.cuda.synchronize
    agree = dict(refine=True, min_agreement=(4, 5))
    out = dict(device=torch.cuda.get_device_name(0), precision=ocr.DEFAULT_PRECISION, passes=args.passes, pages=args.pages,
               lines_per_page=args.lines, chunk_pages=atocr.PIPELINE_CHUNK_PAGES)
    out["b"] = wall(lambda: atocr.process_batch(pages, trs, rec, PARAMS, **agree), args.passes, sync)
    if only_b:
        return out
    refined, post = [], []
    atocr.process_batch(pages, trs, rec, PARAMS, refined_out=refined, posterior=True, posterior_out=post, **agree)
    out["accepted_fraction"] = float(np.concatenate(refined).mean())
    out["characters_with_a_value"] = int(sum((~np.isnan(c.char_posterior)).sum() for c in post))
    out["bp"] = wall(lambda: atocr.process_batch(pages, trs, rec, PARAMS, posterior=True, **agree), args.passes, sync)
    out["bcp"] = wall(lambda: atocr.process_batch(pages, trs, rec, PARAMS, confidence=True, posterior=True, **agree),
                      args.passes, sync)
    step = 16
    out["pp"] = wall(lambda: [forced.refine_pages(pages[a:a + step], trs[a:a + step], rec, PARAMS, (4, 5), posterior=True)
                              for a in range(0, len(pages), step)], args.passes, sync)
    out["pp"]["pages_per_call"] = step
    out["bp_over_b"] = out["bp"]["median_ms"] / out["b"]["median_ms"]
    out["bcp_over_b"] = out["bcp"]["median_ms"] / out["b"]["median_ms"]
    out["bp_over_pp"] = out["bp"]["median_ms"] / out["pp"]["median_ms"]
    out["pipeline_faster_than_refine_pages"] = bool(out["bp"]["median_ms"] < out["pp"]["median_ms"])
    # ---- one 16-page chunk: the bytes of its two workspaces -------------------------------------------------------------------
    atocr.process_batch(pages[:step], trs[:step], rec, PARAMS, posterior=True, **agree)
    out["chunk"] = {"pages": step, "transcript_characters": int(sum(len(tr) for tr in trs[:step])),
                    "posterior_workspace_bytes": int(forced.Refining.last_post_bytes),
                    "moves_workspace_bytes": int(forced.Refining.last_bytes[0])}
    return out


def child(args, tree, only_b):
    """measure() in a process of its own"""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", tree, "--pages", str(args.pages), "--lines", str(args.lines),
           "--passes", str(args.passes)] + (["--only-b"] if only_b else [])
    got = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=900).stdout
    return json.loads(got.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--lines", type=int, default=20)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--leg", default=None, help="(internal) measure on this tree and print the result")
    ap.add_argument("--only-b", action="store_true", help="(internal) the switch-off time alone")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "refine_post_pipeline_time.json"))
    args = ap.parse_args()
    if args.leg is not None:
        print(json.dumps(measure(args, os.path.abspath(args.leg), args.only_b)))
        return
    if args.parent is None:
        out = measure(args, HERE, False)
    else:
        before = child(args, args.parent, True)
        out = child(args, HERE, False)
        after = child(args, args.parent, True)
        q = lambda leg, pc: float(np.percentile(leg["b"]["ms"], pc))                                # noqa: E731
        low, high = min(q(before, 25), q(after, 25)), max(q(before, 75), q(after, 75))
        out["parent"] = {"order": "parent / change / parent, a process each", "b_before": before["b"], "b_after": after["b"],
                         "spread_ms": [low, high], "spread_is": "the smaller lower quartile .. the larger upper quartile of the two runs",
                         "change_b_median_inside_spread": bool(low <= out["b"]["median_ms"] <= high),
                         "change_b_median_is": ("below (faster than)" if out["b"]["median_ms"] < low else
                                                "above (slower than)" if out["b"]["median_ms"] > high else "inside") + " the spread"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    strip = lambda d: {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "ms"}     # noqa: E731
    print(json.dumps(strip(out)))


if __name__ == "__main__":
    main()
