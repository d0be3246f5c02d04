"""What the per-character confidence inside the page pipeline costs, on a real MI355X:

the inputs of tools/refine_time.py -- 64 synthetic pages of 20 lines with second-pass transcripts, chunks of 16 -- and, in
ONE run, wall milliseconds as medians of --passes repeats after a warm-up:
(b)  process_batch(..., refine=True);
(bc) process_batch(..., refine=True, confidence=True);
(cc) forced.refine_pages(..., confidence=True) over the same pages in calls of 16 -- the only way to the values before
     the switch existed.
Beside them the confidence workspace of one 16-page chunk, next to its workspace of moves.
Writes profiles/refine_conf_pipeline_time.json; no threshold is set here.

    python tools/refine_conf_time.py [--pages 64] [--passes 10] [--out profiles/refine_conf_pipeline_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

from tools.refine_time import PARAMS, model_and_pages, second_pass, wall  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--lines", type=int, default=20)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "refine_conf_pipeline_time.json"))
    args = ap.parse_args()
    import torch
    from text_alignment_amd import alignToOCR as atocr, forced, ocr
    rec, pages = model_and_pages(args.pages, args.lines, 4100)
    first = atocr.process_batch(pages, ["amen"] * len(pages), rec, PARAMS)
    trs = [second_pass(r, pg) for r, pg in zip(first, pages)]
    sync = torch.cuda.synchronize
    agree = dict(refine=True, min_agreement=(4, 5))
    out = dict(device=torch.cuda.get_device_name(0), precision=ocr.DEFAULT_PRECISION, passes=args.passes, pages=args.pages,
               lines_per_page=args.lines, chunk_pages=atocr.PIPELINE_CHUNK_PAGES)
    refined, conf = [], []
    atocr.process_batch(pages, trs, rec, PARAMS, refined_out=refined, confidence=True, confidence_out=conf, **agree)
    out["accepted_fraction"] = float(np.concatenate(refined).mean())
    out["characters_with_a_value"] = int(sum((c.char_confidence != forced.NO_CONFIDENCE).sum() for c in conf))
    out["b"] = wall(lambda: atocr.process_batch(pages, trs, rec, PARAMS, **agree), args.passes, sync)
    out["bc"] = wall(lambda: atocr.process_batch(pages, trs, rec, PARAMS, confidence=True, **agree), args.passes, sync)
    step = 16
    out["cc"] = wall(lambda: [forced.refine_pages(pages[a:a + step], trs[a:a + step], rec, PARAMS, (4, 5), confidence=True)
                              for a in range(0, len(pages), step)], args.passes, sync)
    out["cc"]["pages_per_call"] = step
    out["bc_over_b"] = out["bc"]["median_ms"] / out["b"]["median_ms"]
    out["bc_over_cc"] = out["bc"]["median_ms"] / out["cc"]["median_ms"]
    # ---- one 16-page chunk: the bytes of its two workspaces -------------------------------------------------------------------
    atocr.process_batch(pages[:step], trs[:step], rec, PARAMS, confidence=True, **agree)
    out["chunk"] = {"pages": step, "transcript_characters": int(sum(len(tr) for tr in trs[:step])),
                    "confidence_workspace_bytes": int(forced.Refining.last_conf_bytes),
                    "moves_workspace_bytes": int(forced.Refining.last_bytes[0])}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    strip = lambda d: {k: (strip(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "ms"}     # noqa: E731
    print(json.dumps(strip(out)))


if __name__ == "__main__":
    main()
